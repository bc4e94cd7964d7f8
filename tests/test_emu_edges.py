"""Edge stencils, Gaussian blur and bilateral filter (csrc/edges.hip) in the CPU emulator build through the C ABI.

The three stencil functions are checked against the fixture recorded from the reference (tests/golden/edges.npz,
tests/golden/make_edges_golden.py); the Gaussian and the bilateral filter against OpenCV's documented definitions
(tests/known_answers_smooth.py -- unpinned, cv2 is not installed).  This file also holds the vectorised float64
restatements that the GPU tests (tests/test_edges_gpu.py) import, checked here against the fixture and the loop forms.
Kernel logic only; the taps and tables come from the product's host code (das4whales_amd.improcess)."""
import ctypes

import numpy as np
import pytest

from tests import golden_npz
from tests import known_answers_smooth as ka
from tests.emu_util import load_emu, vp

TOL = 1e-5
G = golden_npz.load("edges.npz")
CASES = [str(c) for c in G["cases"]]
P_DOUBLE = ctypes.POINTER(ctypes.c_double)

# D + fliplr(D) of the reference's 5 x 5 diagonal kernel, and W + flipud(W) of its 3 x 3 one
DIAG5 = np.array([[1, 2, 2, 2, 1], [0, 1, 2, 1, 0], [0, 0, 0, 0, 0], [0, -1, -2, -1, 0], [-1, -2, -2, -2, -1]], dtype=np.float64)
DIAG3 = np.array([[1, -2, 1], [-2, 4, -2], [1, -2, 1]], dtype=np.float64)


def rel(y, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(y, dtype=np.float64) - ref)) / max(float(np.max(np.abs(ref))), 1e-300)) if ref.size else 0.0


# ------------------------------------------------------------------------------------------
# float64 restatements (vectorised)
# ------------------------------------------------------------------------------------------
def correlate_zero_f64(img, k, anchor):
    """out[y, x] = sum_ij k[i, j] img[y + i - ay, x + j - ax], zeros outside the image."""
    img, k = np.asarray(img, dtype=np.float64), np.asarray(k, dtype=np.float64)
    h, w = img.shape
    kh, kw = k.shape
    ay, ax = anchor
    p = np.pad(img, ((ay, kh - 1 - ay), (ax, kw - 1 - ax)))
    out = np.zeros((h, w))
    for i in range(kh):
        for j in range(kw):
            if k[i, j] != 0.0:
                out += k[i, j] * p[i:i + h, j:j + w]
    return out


def detect_diagonal_edges_f64(img):
    """fftconvolve(img, D, 'same') + fftconvolve(img, fliplr(D), 'same'): a convolution, so the summed kernel is flipped."""
    return correlate_zero_f64(img, DIAG5[::-1, ::-1], (2, 2))


def diagonal_edge_detection_f64(img):
    return correlate_zero_f64(img, DIAG3, (1, 1))


def gradient_oriented_f64(img, direction):
    """The reference's slices written with explicit ends (dft, dfx >= 0); (0, 0) is the empty [h, 0]."""
    img = np.asarray(img, dtype=np.float64)
    h, w = img.shape
    dft, dfx = direction
    if dfx == 0:
        return -(img[:, :max(w - dft, 0)] - img[:, dft:]) if dft else np.empty((h, 0))
    if dft == 0:
        return -(img[dfx:, :] - img[:max(h - dfx, 0), :])
    oh, ow = max(h - 2 * dfx, 0), max(w - dft, 0)
    return -(img[dfx:dfx + oh, :ow] - 0.5 * img[2 * dfx:2 * dfx + oh, dft:] - 0.5 * img[:oh, dft:])


def _correlate_axis_reflect101(img, taps, axis):
    a = len(taps) // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (a, a)
    p = np.pad(img, pad, mode="reflect") if a else img
    n = img.shape[axis]
    out = np.zeros(img.shape)
    for t, v in enumerate(taps):
        out += v * (p[t:t + n, :] if axis == 0 else p[:, t:t + n])
    return out


def gaussian_f64(img, size, sigma):
    """cv2.GaussianBlur(img, (size, size), sigma) by its documented definition, vectorised."""
    img = np.asarray(img, dtype=np.float64)
    taps = ka.gaussian_kernel_loops(size, sigma)
    return _correlate_axis_reflect101(_correlate_axis_reflect101(img, taps, 1), taps, 0)


def bilateral_f64(img, diameter, sigma_color, sigma_space):
    """cv2.bilateralFilter by its documented definition, vectorised over the image (one pass per tap)."""
    img = np.asarray(img, dtype=np.float64)
    h, w = img.shape
    sc = sigma_color if sigma_color > 0 else 1.0
    ss = sigma_space if sigma_space > 0 else 1.0
    r = ka.bilateral_radius_loops(diameter, ss)
    p = np.pad(img, r, mode="reflect") if r else img
    num, den = np.zeros((h, w)), np.zeros((h, w))
    for i in range(-r, r + 1):
        for j in range(-r, r + 1):
            if i * i + j * j > r * r:
                continue
            q = p[r + i:r + i + h, r + j:r + j + w]
            wt = np.exp(-(i * i + j * j) / (2 * ss * ss) - (q - img) ** 2 / (2 * sc * sc))
            num += wt * q
            den += wt
    return num / den


# ------------------------------------------------------------------------------------------
# the emulator build through the C ABI
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    lib = load_emu()
    lib.d4w_gaussian_blur_ws_bytes.restype = ctypes.c_size_t
    lib.d4w_bilateral_f32.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_double,
                                      ctypes.c_void_p, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def ip():
    from das4whales_amd import improcess
    return improcess


def f32(img):
    return np.ascontiguousarray(img, dtype=np.float32)


def emu_stencil(lib, img, k, anchor):
    x = f32(img)
    k = np.ascontiguousarray(k, dtype=np.float64)
    out = np.full(x.shape, np.nan, dtype=np.float32)
    rc = lib.d4w_stencil_zero_f32(vp(x), x.shape[0], x.shape[1], k.ctypes.data_as(P_DOUBLE), k.shape[0], k.shape[1], anchor[0],
                                  anchor[1], vp(out), None)
    assert rc == 0, lib.d4w_last_error()
    return out


def emu_gradient(lib, img, direction):
    x = f32(img)
    ref = gradient_oriented_f64(x, direction)
    out = np.full(ref.shape, np.nan, dtype=np.float32)
    rc = lib.d4w_gradient_oriented_f32(vp(x), x.shape[0], x.shape[1], direction[0], direction[1], vp(out) if out.size else None, None)
    assert rc == 0, lib.d4w_last_error()
    return out


def emu_gaussian(lib, ip, img, size, sigma):
    x = f32(img)
    h, w = x.shape
    taps = ip.get_gaussian_kernel(size, sigma)
    out = np.full(x.shape, np.nan, dtype=np.float32)
    nws = lib.d4w_gaussian_blur_ws_bytes(h, w, size, size)
    assert (nws == 0) == (size <= 31)
    ws = np.empty(max(nws, 1), dtype=np.uint8)
    rc = lib.d4w_gaussian_blur_f32(vp(x), h, w, taps.ctypes.data_as(P_DOUBLE), taps.ctypes.data_as(P_DOUBLE), size, size, vp(out),
                                   vp(ws) if nws else None, None)
    assert rc == 0, lib.d4w_last_error()
    return out


def emu_bilateral(lib, ip, img, diameter, sigma_color, sigma_space):
    x = f32(img)
    sc = sigma_color if sigma_color > 0 else 1.0
    ss = sigma_space if sigma_space > 0 else 1.0
    r = ip.bilateral_radius(diameter, ss)
    sw = f32(ip.bilateral_space_weights(r, ss))
    out = np.full(x.shape, np.nan, dtype=np.float32)
    rc = lib.d4w_bilateral_f32(vp(x), x.shape[0], x.shape[1], r, vp(sw), sc, vp(out), None)
    assert rc == 0, lib.d4w_last_error()
    return out


# ------------------------------------------------------------------------------------------
# restatements against the fixture and the loop forms
# ------------------------------------------------------------------------------------------
def test_restatements_match_fixture():
    for name in CASES:
        x = G[name + "/x"]
        assert rel(detect_diagonal_edges_f64(x), G[name + "/dde"]) < 1e-12, name          # fftconvolve's own rounding
        # the reference computes this one in float32 (inputs rounded to float32, nine float32 products summed): its own
        # rounding is of the order 16 max|x| 2^-24 against outputs that cancel, so it is held to the project's bar
        assert rel(diagonal_edge_detection_f64(x), G[name + "/ded"]) < TOL, name
        for dft, dfx in G[name + "/directions"]:
            ref = G["%s/grad_%d_%d" % (name, dft, dfx)]
            y = gradient_oriented_f64(x, (int(dft), int(dfx)))
            assert y.shape == ref.shape and np.array_equal(y, ref), (name, dft, dfx)


def test_restatements_match_loops():
    rng = np.random.default_rng(3)
    for shape, n, sigma in [((9, 13), 5, 0), ((4, 3), 9, 1.7), ((11, 6), 7, 2.2), ((1, 5), 3, 0.5), ((2, 2), 5, 0)]:
        img = rng.standard_normal(shape) * 30 + 90
        assert rel(gaussian_f64(img, n, sigma), ka.gaussian_blur_loops(img, n, sigma)) < 1e-13, (shape, n, sigma)
    for shape, d, sc, ss in [((9, 13), 5, 30.0, 30.0), ((4, 3), 9, 12.0, 2.0), ((7, 8), 3, 5.0, 0.7), ((6, 9), 0, 40.0, 1.4),
                             ((1, 5), 5, 0, 0)]:
        img = np.round(rng.random(shape) * 255)
        assert rel(bilateral_f64(img, d, sc, ss), ka.bilateral_loops(img, d, sc, ss)) < 1e-13, (shape, d, sc, ss)
    ka.check_gaussian(gaussian_f64, 1e-13)
    ka.check_bilateral(bilateral_f64, 1e-13)


def test_host_tables(ip):
    for n in (1, 3, 5, 7, 9, 21, 31, 33, 101):
        for sigma in (0, -1.0, 0.6, 1.3, 4.5, 20.0):
            t = ip.get_gaussian_kernel(n, sigma)
            assert t.dtype == np.float64 and np.allclose(t, ka.gaussian_kernel_loops(n, sigma), rtol=1e-14, atol=0), (n, sigma)
    for d, ss, r in [(5, 3.0, 2), (9, 1.0, 4), (1, 2.0, 0), (0, 1.4, 2), (-3, 0.1, 1), (0, 3.0, 4), (0, 5.0, 8), (0, 1.0, 2)]:
        assert ip.bilateral_radius(d, ss) == r == ka.bilateral_radius_loops(d, ss), (d, ss)
    sw = ip.bilateral_space_weights(2, 1.5)
    assert sw.shape == (5, 5) and sw[2, 2] == 1.0 and sw[0, 0] == 0.0 and sw[0, 1] == 0.0 and sw[0, 2] == np.exp(-4 / 4.5)
    assert np.count_nonzero(sw) == 13


# ------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_emu_stencils_fixture(emu, name):
    x = G[name + "/x"]
    y = emu_stencil(emu, x, DIAG5[::-1, ::-1], (2, 2))
    assert rel(y, G[name + "/dde"]) < TOL, (name, rel(y, G[name + "/dde"]))
    y = emu_stencil(emu, x, DIAG3, (1, 1))
    assert rel(y, G[name + "/ded"]) < TOL, (name, rel(y, G[name + "/ded"]))


@pytest.mark.parametrize("name", CASES)
def test_emu_gradient_fixture(emu, name):
    x = G[name + "/x"]
    for dft, dfx in G[name + "/directions"]:
        ref = G["%s/grad_%d_%d" % (name, dft, dfx)]
        y = emu_gradient(emu, x, (int(dft), int(dfx)))
        assert y.shape == ref.shape and rel(y, ref) < TOL, (name, dft, dfx, rel(y, ref))


@pytest.mark.parametrize("shape,kshape,anchor", [((45, 70), (7, 7), (3, 3)), ((33, 130), (7, 7), (0, 6)), ((5, 4), (7, 7), (6, 0)),
                                                 ((40, 65), (1, 1), (0, 0)), ((2, 2), (5, 5), (2, 2)), ((70, 9), (2, 3), (1, 0)),
                                                 ((1, 200), (3, 7), (1, 3)), ((64, 64), (4, 4), (3, 3))])
def test_emu_stencil_any_kernel(emu, shape, kshape, anchor):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    x = np.round(rng.standard_normal(shape) * 64) / 16
    k = np.round(rng.standard_normal(kshape) * 8) / 4
    y = emu_stencil(emu, x, k, anchor)
    ref = correlate_zero_f64(x, k, anchor)
    assert rel(y, ref) < TOL, rel(y, ref)


def test_emu_gradient_large_shifts(emu):
    rng = np.random.default_rng(9)
    x = np.round(rng.standard_normal((40, 300)) * 256) / 256
    for d in [(257, 0), (0, 19), (20, 9), (299, 19), (300, 1), (1, 20), (0, 40), (7, 7)]:
        y = emu_gradient(emu, x, d)
        ref = gradient_oriented_f64(x, d)
        assert y.shape == ref.shape and rel(y, ref) < TOL, d


def test_emu_gaussian_known_answers(emu, ip):
    """Sizes 1 .. 31 take the fused LDS form, 33 the two-launch form; widths that are no multiple of the 64-pixel tile and
    images smaller than the halo are among the shapes."""
    ka.check_gaussian(lambda img, n, s: emu_gaussian(emu, ip, img, n, s), TOL)


@pytest.mark.parametrize("shape,size,sigma", [((45, 70), 9, 2.0), ((33, 130), 31, 4.5), ((3, 4), 31, 6.0), ((40, 65), 33, 5.0),
                                              ((70, 31), 5, 0), ((65, 129), 21, -1.0)])
def test_emu_gaussian_restatement(emu, ip, shape, size, sigma):
    rng = np.random.default_rng(size)
    x = f32(rng.random(shape) * 255)
    y = emu_gaussian(emu, ip, x, size, sigma)
    assert rel(y, gaussian_f64(x, size, sigma)) < TOL


def test_emu_bilateral_known_answers(emu, ip):
    """Diameters 3 (r = 1) .. 31 (r = 15, the largest tiled radius) take the LDS form, 33 (r = 16) the untiled one."""
    assert emu.d4w_bilateral_max_tiled_radius() == 15
    ka.check_bilateral(lambda img, d, sc, ss: emu_bilateral(emu, ip, img, d, sc, ss), TOL)


@pytest.mark.parametrize("shape,d,sc,ss", [((45, 70), 5, 30.0, 30.0), ((21, 130), 9, 12.0, 3.0), ((3, 4), 31, 50.0, 8.0),
                                           ((20, 65), 31, 25.0, 6.0), ((20, 65), 33, 25.0, 6.0), ((17, 66), 3, 8.0, 1.0),
                                           ((19, 40), 0, 20.0, 2.5)])
def test_emu_bilateral_restatement(emu, ip, shape, d, sc, ss):
    rng = np.random.default_rng(d + shape[0])
    x = f32(np.round(rng.random(shape) * 255))
    y = emu_bilateral(emu, ip, x, d, sc, ss)
    assert rel(y, bilateral_f64(x, d, sc, ss)) < TOL


def test_emu_uint8_rule(emu, ip):
    rng = np.random.default_rng(2026)
    u = (rng.random((60, 80)) * 256).astype(np.uint8)
    for n, s in [(5, 1.3), (9, 2.0)]:
        ka.check_uint8_rule(ka.round_u8(emu_gaussian(emu, ip, u, n, s)), gaussian_f64(u, n, s), ("gaussian", n, s))
    ka.check_uint8_rule(ka.round_u8(emu_bilateral(emu, ip, u, 5, 30.0, 30.0)), bilateral_f64(u, 5, 30.0, 30.0), "bilateral")
    # the dyadic fixed tables put many pixels exactly on a tie; float32 is exact there
    for n in (3, 5, 7):
        assert np.array_equal(ka.round_u8(emu_gaussian(emu, ip, u, n, 0)), ka.round_u8(gaussian_f64(u, n, 0))), n


def test_emu_bad_arguments(emu):
    x = np.ones((8, 8), dtype=np.float32)
    out = np.full((8, 8), 7.0, dtype=np.float32)
    k = np.ones((8, 8), dtype=np.float64)
    kp = k.ctypes.data_as(P_DOUBLE)
    assert emu.d4w_stencil_zero_f32(vp(x), 8, 8, kp, 8, 3, 0, 0, vp(out), None) == -1 and b"kernel" in emu.d4w_last_error()
    assert emu.d4w_stencil_zero_f32(vp(x), 8, 8, kp, 3, 3, 3, 0, vp(out), None) == -1 and b"anchor" in emu.d4w_last_error()
    assert emu.d4w_stencil_zero_f32(vp(x), 0, 8, kp, 3, 3, 1, 1, vp(out), None) == -1
    assert emu.d4w_stencil_zero_f32(vp(x), 8, 8, None, 3, 3, 1, 1, vp(out), None) == -1
    assert emu.d4w_stencil_zero_f32(vp(x), 8, 8, kp, 3, 3, 1, 1, vp(x), None) == -1
    k[0, 0] = np.nan
    assert emu.d4w_stencil_zero_f32(vp(x), 8, 8, kp, 3, 3, 1, 1, vp(out), None) == -1 and b"finite" in emu.d4w_last_error()
    assert emu.d4w_gradient_oriented_f32(vp(x), 8, 8, -1, 0, vp(out), None) == -1
    assert emu.d4w_gradient_oriented_f32(vp(x), 8, 0, 1, 0, vp(out), None) == -1
    assert emu.d4w_gradient_oriented_f32(vp(x), 8, 8, 0, 0, None, None) == 0            # empty output: nothing written
    assert emu.d4w_gradient_oriented_f32(vp(x), 8, 8, 9, 2, None, None) == 0
    assert emu.d4w_gradient_oriented_f32(vp(x), 8, 8, 1, 0, None, None) == -1
    t = np.ones(64, dtype=np.float64) / 3
    tp = t.ctypes.data_as(P_DOUBLE)
    assert emu.d4w_gaussian_blur_f32(vp(x), 8, 8, tp, tp, 4, 3, vp(out), None, None) == -1 and b"odd" in emu.d4w_last_error()
    assert emu.d4w_gaussian_blur_f32(vp(x), 8, 8, tp, None, 3, 3, vp(out), None, None) == -1
    assert emu.d4w_gaussian_blur_f32(vp(x), 8, 8, tp, tp, 33, 3, vp(out), None, None) == -1 and b"workspace" in emu.d4w_last_error()
    assert emu.d4w_gaussian_blur_f32(vp(x), 8, -1, tp, tp, 3, 3, vp(out), None, None) == -1
    assert emu.d4w_gaussian_blur_ws_bytes(8, 8, 31, 31) == 0 and emu.d4w_gaussian_blur_ws_bytes(8, 8, 33, 3) >= 8 * 8 * 4 + 36 * 4
    sw = np.ones(9, dtype=np.float32)
    assert emu.d4w_bilateral_f32(vp(x), 8, 8, -1, vp(sw), 1.0, vp(out), None) == -1 and b"radius" in emu.d4w_last_error()
    assert emu.d4w_bilateral_f32(vp(x), 8, 8, 1, vp(sw), 0.0, vp(out), None) == -1 and b"sigma_color" in emu.d4w_last_error()
    assert emu.d4w_bilateral_f32(vp(x), 8, 8, 1, None, 1.0, vp(out), None) == -1
    assert np.all(out == 7.0)
    assert emu.d4w_bilateral_f32(vp(x), 8, 8, 1, vp(sw), 1.0, vp(out), None) == 0 and np.all(out == 1.0)
