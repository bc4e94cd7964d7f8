"""Generate tests/golden/edges.npz: the reference's improcess.gradient_oriented (improcess.py:143-169),
detect_diagonal_edges (:172-226) and diagonal_edge_detection (:229-266) on small seeded cases, run from the reference's
own code (oracle/ref_harness.import_reference; they need only NumPy, SciPy and CPU torch).

    python tests/golden/make_edges_golden.py

Per case `<name>`: the input `<name>/x` (float64), `<name>/dde` = detect_diagonal_edges(x, 0.5) (float64),
`<name>/ded` = diagonal_edge_detection(x, 0.5) (the reference's CPU float32 tensor as an array) and, per direction
`<dft>_<dfx>` of `<name>/directions`, `<name>/grad_<dft>_<dfx>` = gradient_oriented(x, (dft, dfx)).  The last direction of
every case is (0, h), which empties the output.  For (0, 0) the reference subtracts [h, w] from the empty [h, 0], which NumPy
refuses unless w = 1: `<name>/grad_0_0_raises` marks those cases, and the recorded array is the empty [h, 0] that the
mirror returns for every width.  The GPU tests (tests/test_edges_gpu.py) and the emulator tests
(tests/test_emu_edges.py) compare against it.  Only data goes into the fixture.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.ref_harness import import_reference  # noqa: E402
from tests.golden_npz import load, save  # noqa: E402

DIRECTIONS = [(1, 0), (3, 0), (0, 1), (0, 2), (1, 1), (2, 3), (0, 0)]


def smooth_image(rng, h, w):
    """Smooth background, a bright diagonal line and noise, quantised to 1/256 so that the fixture compresses."""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    img = np.sin(xx / max(w, 2) * 3.1) * np.cos(yy / max(h, 2) * 2.3) + 0.5
    img += 2.0 * (np.abs(yy - 0.4 * xx - h * 0.2) < 1.5)
    img += 0.25 * rng.standard_normal((h, w))
    return np.round(img * 256) / 256


def main():
    ref = import_reference().improcess
    rng = np.random.default_rng(20261016)
    cases = {}
    for h, w in [(37, 52), (60, 41), (1, 9), (9, 1), (2, 2), (240, 320)]:
        cases["s%dx%d" % (h, w)] = smooth_image(rng, h, w)
    cases["imagebin"] = load("image_240x1600.npz")["imagebin"].astype(np.float64)
    out = {"cases": np.array(sorted(cases))}
    for name, x in cases.items():
        dirs = DIRECTIONS + [(0, x.shape[0])]
        out[name + "/x"] = x
        out[name + "/dde"] = np.asarray(ref.detect_diagonal_edges(x, 0.5), dtype=np.float64)
        ded = ref.diagonal_edge_detection(x, 0.5)
        assert ded.dtype.is_floating_point and ded.element_size() == 4 and not ded.is_cuda
        out[name + "/ded"] = ded.numpy()
        out[name + "/directions"] = np.array(dirs, dtype=np.int64)
        for dft, dfx in dirs:
            try:
                g = ref.gradient_oriented(x, (dft, dfx))
            except ValueError:
                # (0, 0): image[:, :-0] is [h, 0] and image[:, 0:] is [h, w]; NumPy broadcasts them only for w = 1.  The
                # mirror returns the left operand's empty [h, 0] for every width.
                assert (dft, dfx) == (0, 0) and x.shape[1] != 1
                g = np.empty((x.shape[0], 0))
                out[name + "/grad_0_0_raises"] = np.array(True)
            out["%s/grad_%d_%d" % (name, dft, dfx)] = g
        print("%-10s %-12s dde %s ded %s grads %s" % (name, x.shape, out[name + "/dde"].shape, out[name + "/ded"].shape,
                                                      [out["%s/grad_%d_%d" % (name, a, b)].shape for a, b in dirs]))
    print(save(os.path.join(HERE, "edges.npz"), out))


if __name__ == "__main__":
    main()
