"""Generate tests/golden/radon.npz: the reference's improcess.compute_radon_transform (improcess.py:347-367), which is
skimage.transform.radon(image, theta=theta, circle=False), on small seeded cases.

Run under a Python that has scikit-image (the reference's own dependency; this fixture was made with 0.18.3):

    python tests/golden/make_radon_golden.py

Per case `<name>`: the input `<name>/x` (in the dtype the case is about), the angles `<name>/theta` (degrees, float64)
and skimage's output `<name>/y` in float64, with the dtype skimage returned in `<name>/dtype`.  `skimage_version`
records the version that made the file.  The GPU tests (tests/test_radon_gpu.py) and the emulator tests
(tests/test_emu_radon.py) compare against it.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden_npz import load, save  # noqa: E402


def smooth_image(rng, h, w):
    """Smooth background, a bright line and noise, quantised to 1/256 so that the fixture compresses."""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    img = np.sin(xx / max(w, 2) * 3.1) * np.cos(yy / max(h, 2) * 2.3) + 0.5
    img += 2.0 * (np.abs(yy - 0.4 * xx - h * 0.2) < 1.5)
    img += 0.25 * rng.standard_normal((h, w))
    return np.round(img * 256) / 256


def main():
    import skimage
    from skimage.transform import radon
    rng = np.random.default_rng(20261016)
    cases = {}
    for h, w in [(37, 52), (60, 41), (64, 64), (1, 9), (9, 1), (2, 2)]:
        cases["s%dx%d" % (h, w)] = (smooth_image(rng, h, w), None)
    cases["theta_any"] = (smooth_image(rng, 33, 47),
                          np.array([-400.0, -135.5, -1.0, 0.0, 0.25, 45.0, 90.0, 137.3, 180.0, 181.5, 270.0, 359.9, 400.0]))
    cases["s240x320"] = (smooth_image(rng, 240, 320), None)
    cases["u8"] = ((rng.random((31, 45)) * 256).astype(np.uint8), np.arange(0, 180, 7.5))
    cases["bool"] = (rng.random((40, 29)) > 0.6, np.arange(0, 180, 7.5))
    cases["f32"] = (smooth_image(rng, 28, 35).astype(np.float32), np.arange(0, 180, 7.5))
    cases["imagebin"] = (load("image_240x1600.npz")["imagebin"].astype(np.float64), None)
    out = {"skimage_version": np.array(skimage.__version__), "cases": np.array(sorted(cases))}
    for name, (x, theta) in cases.items():
        th = np.arange(180, dtype=np.float64) if theta is None else np.asarray(theta, dtype=np.float64)
        y = radon(x, theta=(None if theta is None else th), circle=False)
        out[name + "/x"] = x
        out[name + "/theta"] = th
        out[name + "/y"] = y.astype(np.float64)
        out[name + "/dtype"] = np.array(y.dtype.name)
        print("%-10s %-8s %-12s -> %s %s" % (name, x.dtype, x.shape, y.shape, y.dtype))
    print(save(os.path.join(HERE, "radon.npz"), out))


if __name__ == "__main__":
    main()
