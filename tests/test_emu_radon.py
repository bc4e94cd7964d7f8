"""Radon transform (csrc/radon.hip) in the CPU emulator build through the C ABI, against the fixture recorded from the
reference's call (tests/golden/radon.npz: skimage.transform.radon(x, theta, circle=False)) and against a float64
restatement of that call kept in this file.  Kernel logic only; the GPU parity tests are tests/test_radon_gpu.py."""
import ctypes

import numpy as np
import pytest

from tests import golden_npz
from tests.emu_util import load_emu, vp

TOL = 1e-5


def img_as_float64(image):
    """skimage's convert_to_float(image, preserve_range=False) in float64: bool 0 / 1, unsigned / max,
    signed (2 x + 1) / (max - min), floats as they are."""
    a = np.asarray(image)
    if a.dtype.kind == "b":
        return a.astype(np.float64)
    if a.dtype.kind == "u":
        return a / float(np.iinfo(a.dtype).max)
    if a.dtype.kind == "i":
        ii = np.iinfo(a.dtype)
        return (2.0 * a.astype(np.float64) + 1.0) / float(ii.max - ii.min)
    return a.astype(np.float64)


def _bilinear(img, r, c):
    """skimage's bilinear_interpolation with mode 'constant', cval 0: floor / ceil neighbours, 0 outside."""
    rows, cols = img.shape
    minr, minc, maxr, maxc = np.floor(r), np.floor(c), np.ceil(r), np.ceil(c)
    dr, dc = r - minr, c - minc

    def px(rr, cc):
        ok = (rr >= 0) & (rr < rows) & (cc >= 0) & (cc < cols)
        return np.where(ok, img[np.clip(rr, 0, rows - 1).astype(np.int64), np.clip(cc, 0, cols - 1).astype(np.int64)], 0.0)

    top = (1 - dc) * px(minr, minc) + dc * px(minr, maxc)
    bottom = (1 - dc) * px(maxr, minc) + dc * px(maxr, maxc)
    return (1 - dr) * top + dr * bottom


def radon_f64(image, theta=None):
    """skimage.transform.radon(image, theta, circle=False) (scikit-image 0.18.3) restated in float64 NumPy."""
    img = img_as_float64(image)
    if img.ndim != 2:
        raise ValueError("The input image must be 2-D")
    theta = np.arange(180) if theta is None else np.asarray(theta)
    diagonal = np.sqrt(2) * max(img.shape)
    pad = [int(np.ceil(diagonal - s)) for s in img.shape]
    pad_before = [(s + p) // 2 - s // 2 for s, p in zip(img.shape, pad)]
    padded = np.pad(img, [(pb, p - pb) for pb, p in zip(pad_before, pad)], mode="constant", constant_values=0)
    P = padded.shape[0]
    center = P // 2
    rr, cc = np.meshgrid(np.arange(P, dtype=np.float64), np.arange(P, dtype=np.float64), indexing="ij")
    out = np.zeros((P, len(theta)))
    for i, angle in enumerate(np.deg2rad(theta)):
        cos_a, sin_a = np.cos(angle), np.sin(angle)
        x = cos_a * cc + sin_a * rr + (-center * (cos_a + sin_a - 1))        # warp's affine map of output (r, c)
        y = -sin_a * cc + cos_a * rr + (-center * (cos_a - sin_a - 1))
        out[:, i] = _bilinear(padded, y, x).sum(0)
    return out


def rel(y, ref):
    return float(np.max(np.abs(np.asarray(y, dtype=np.float64) - ref)) / max(np.max(np.abs(ref)), 1e-300))


@pytest.fixture(scope="module")
def emu():
    lib = load_emu()
    lib.d4w_radon_ws_bytes.restype = ctypes.c_size_t
    return lib


def emu_radon(lib, image, theta):
    x = np.ascontiguousarray(img_as_float64(image), dtype=np.float32)
    th = np.ascontiguousarray(theta, dtype=np.float64)
    h, w = x.shape
    P = lib.d4w_radon_size(h, w)
    assert P > 0
    out = np.full((P, th.size), np.nan, dtype=np.float32)
    ws = np.empty(max(lib.d4w_radon_ws_bytes(h, w, th.size), 1), dtype=np.uint8)
    rc = lib.d4w_radon_f32(vp(x), h, w, th.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), th.size, vp(out), vp(ws), None)
    assert rc == 0, lib.d4w_last_error()
    return out


G = golden_npz.load("radon.npz")
CASES = [str(c) for c in G["cases"]]


def test_restatement_matches_fixture():
    """The float64 restatement is skimage's radon: equal to the recorded output up to float64 rounding."""
    for name in CASES:
        ref = G[name + "/y"]
        y = radon_f64(G[name + "/x"], G[name + "/theta"])
        assert y.shape == ref.shape, name
        tol = TOL if str(G[name + "/dtype"]) == "float32" else 1e-12      # skimage sums float32 input in float32
        assert rel(y, ref) < tol, (name, rel(y, ref))


@pytest.mark.parametrize("name", [c for c in CASES if c != "s240x320"] + ["s240x320"])
def test_emu_fixture(emu, name):
    x, th, ref = G[name + "/x"], G[name + "/theta"], G[name + "/y"]
    if name == "s240x320":
        th = th[::9]                       # every 9th angle: the emulator runs every lane as a host fiber
        ref = ref[:, ::9]
    y = emu_radon(emu, x, th)
    assert y.shape == ref.shape and rel(y, ref) < TOL, (name, rel(y, ref))


def test_emu_restatement_angles(emu):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((45, 70)) + 3.0
    th = np.array([0.0, 45.0, 90.0, 137.3, -89.99, 179.999, 1e-9, 270.0, 1000.25])
    y = emu_radon(emu, x, th)
    ref = radon_f64(x, th)
    assert rel(y, ref) < TOL, rel(y, ref)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 2), (2, 1), (3, 1), (1, 17), (17, 2), (5, 5)])
def test_emu_degenerate_shapes(emu, h, w):
    rng = np.random.default_rng(h * 100 + w)
    x = rng.random((h, w)) + 0.5
    th = np.array([0.0, 17.0, 45.0, 90.0, 133.0, 180.0, 311.0])
    y = emu_radon(emu, x, th)
    ref = radon_f64(x, th)
    assert y.shape == ref.shape == (int(np.ceil(np.sqrt(2) * max(h, w))), th.size)
    assert rel(y, ref) < TOL, rel(y, ref)


def test_emu_size_and_arguments(emu):
    for h, w in [(1, 1), (37, 52), (1102, 1200), (24, 160), (9, 1)]:
        assert emu.d4w_radon_size(h, w) == int(np.ceil(np.sqrt(2) * max(h, w)))
    assert emu.d4w_radon_size(0, 5) == -1 and b"empty" in emu.d4w_last_error()
    assert emu.d4w_radon_size(5, -1) == -1
    assert emu.d4w_radon_ws_bytes(8, 8, 0) == 0 and emu.d4w_radon_ws_bytes(8, 8, 180) >= 180 * 16
    x = np.ones((8, 8), dtype=np.float32)
    out = np.full((12, 1), 7.0, dtype=np.float32)
    th = np.array([np.nan])
    ws = np.empty(256, dtype=np.uint8)
    P = ctypes.POINTER(ctypes.c_double)
    # empty theta: nothing is written, no workspace needed
    assert emu.d4w_radon_f32(vp(x), 8, 8, None, 0, vp(out), None, None) == 0 and np.all(out == 7.0)
    assert emu.d4w_radon_f32(vp(x), 8, 8, th.ctypes.data_as(P), 1, vp(out), vp(ws), None) == -1
    assert b"finite" in emu.d4w_last_error()
    th[0] = 30.0
    assert emu.d4w_radon_f32(None, 8, 8, th.ctypes.data_as(P), 1, vp(out), vp(ws), None) == -1
    assert emu.d4w_radon_f32(vp(x), 8, 8, th.ctypes.data_as(P), 1, vp(out), None, None) == -1
    assert emu.d4w_radon_f32(vp(x), 8, 8, th.ctypes.data_as(P), -1, vp(out), vp(ws), None) == -1
    assert emu.d4w_radon_f32(vp(x), 0, 8, th.ctypes.data_as(P), 1, vp(out), vp(ws), None) == -1
    assert emu.d4w_radon_f32(vp(x), 8, 8, th.ctypes.data_as(P), 1, vp(out), vp(ws), None) == 0
    assert np.all(np.isfinite(out))


def test_restatement_empty_theta():
    assert radon_f64(np.ones((5, 7)), np.array([])).shape == (10, 0)
    with pytest.raises(ValueError):
        radon_f64(np.ones((2, 3, 4)))
