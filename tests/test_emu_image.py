"""Image operators (image.hip) in the CPU emulator build against the oracle -- kernel logic only;
the GPU parity tests are tests/test_image_gpu.py."""
import ctypes

import numpy as np
import pytest

from oracle import d4w_oracle as orc
from tests import image_cases as ic
from tests.emu_util import load_emu, vp

TOL = 1e-5
sz = ctypes.c_size_t


@pytest.fixture(scope="module")
def emu():
    return load_emu()


def rel(y, ref):
    return float(np.max(np.abs(np.asarray(y, dtype=np.float64) - ref)) / max(np.max(np.abs(ref)), 1e-300))


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def test_minmax_scale_threshold_mask(emu):
    rng = np.random.default_rng(0)
    x = f32(rng.standard_normal(5003) * 7 - 2)
    mm = np.zeros(2, dtype=np.float32)
    assert emu.d4w_minmax_f32(vp(x), sz(x.size), vp(mm), None) == 0
    assert mm[0] == x.min() and mm[1] == x.max()
    y = np.empty_like(x)
    assert emu.d4w_scale_pixels_f32(vp(x), vp(y), sz(x.size), vp(mm), ctypes.c_double(255.0), None) == 0
    assert rel(y, orc.scale_pixels(x.astype(np.float64)) * 255) < TOL
    assert emu.d4w_threshold_f32(vp(x), vp(y), sz(x.size), ctypes.c_double(0.25), None) == 0
    assert np.array_equal(y != 0, x.astype(np.float64) > 0.25)
    m = f32(rng.random(x.size) > 0.5)
    assert emu.d4w_mask_mul_f32(vp(x), vp(m), vp(y), sz(x.size), None) == 0
    assert np.array_equal(y, x * m)
    neg = f32([-3.0, -1.0, -2.0])
    assert emu.d4w_minmax_f32(vp(neg), sz(3), vp(mm), None) == 0 and mm[0] == -3 and mm[1] == -1
    # np.min / np.max propagate NaN (the threshold 0.45 * np.max(corr) of scripts/main_mfdetect.py:82 is NaN then, and picks nothing):
    # both forms of the reduction (one workgroup for small inputs, the three-launch form) do too
    for n in (700, 300 * 1200):
        bad = rng.random(n).astype(np.float32) - 0.5
        bad[n // 3] = np.nan
        assert emu.d4w_minmax_f32(vp(bad), sz(n), vp(mm), None) == 0 and np.isnan(mm[0]) and np.isnan(mm[1]), (n, mm)
        bad[n // 3] = 2.0
        assert emu.d4w_minmax_f32(vp(bad), sz(n), vp(mm), None) == 0 and mm[0] == bad.min() and mm[1] == 2.0


@pytest.mark.parametrize("h,w,oh,ow", [(40, 120, 4, 12), (37, 101, 3, 10), (4, 12, 40, 120), (50, 33, 17, 80), (9, 300, 9, 30)])
def test_resize_bilinear_aa(emu, h, w, oh, ow):
    rng = np.random.default_rng(h * w)
    x = f32(rng.standard_normal((h, w)))
    y = np.empty((oh, ow), dtype=np.float32)
    emu.d4w_resize_ws_bytes.restype = sz
    ws = np.empty(emu.d4w_resize_ws_bytes(h, w, oh, ow), dtype=np.uint8)
    assert emu.d4w_resize_bilinear_aa_f32(vp(x), h, w, vp(y), oh, ow, vp(ws), None) == 0, emu.d4w_last_error()
    assert rel(y, orc.resize_bilinear_aa(x.astype(np.float64), oh, ow)) < TOL


@pytest.mark.parametrize("h,w,kh,kw", [(24, 160, 101, 101), (70, 130, 5, 9), (3, 4, 7, 7), (33, 65, 1, 1), (40, 70, 4, 6), (9, 600, 3, 113),
                                       (21, 300, 5, 115), (6, 2100, 2, 33)])
def test_filter2d(emu, h, w, kh, kw):
    """Kernels of <= 113 columns run on the matrix cores (filter2d_mm.hip: one wave per 256 columns, 4 output rows per
    workgroup, ragged tiles, more than 8 tiles per row -> several workgroups per row block), wider ones the direct form."""
    rng = np.random.default_rng(kh * 100 + kw)
    img = f32(rng.standard_normal((h, w)))
    ker = f32(rng.standard_normal((kh, kw)))
    if (kh, kw) == (101, 101):
        up, down = orc.gabor_filt_design(42.56)
        ker = f32(up)
    out = np.empty_like(img)
    emu.d4w_filter2d_ws_bytes.restype = sz
    ws = np.empty(emu.d4w_filter2d_ws_bytes(kh, kw), dtype=np.uint8)
    assert emu.d4w_filter2d_f32(vp(img), h, w, vp(ker), kh, kw, vp(out), 0, vp(ws), None) == 0, emu.d4w_last_error()
    ref = orc.filter2d(img.astype(np.float64), ker.astype(np.float64))
    assert rel(out, ref) < TOL
    assert emu.d4w_filter2d_f32(vp(img), h, w, vp(ker), kh, kw, vp(out), 1, vp(ws), None) == 0      # accumulate
    assert rel(out, 2 * ref) < TOL


def run_filter2d(emu):
    emu.d4w_filter2d_ws_bytes.restype = sz

    def run(img, ker, accumulate=0, out=None):
        img, ker = f32(img), f32(ker)
        (h, w), (kh, kw) = img.shape, ker.shape
        out = np.empty_like(img) if out is None else out
        ws = np.empty(emu.d4w_filter2d_ws_bytes(kh, kw), dtype=np.uint8)
        assert emu.d4w_filter2d_f32(vp(img), h, w, vp(ker), kh, kw, vp(out), accumulate, vp(ws), None) == 0, emu.d4w_last_error()
        return out
    return run


@pytest.mark.parametrize("h,w,kh,kw", ic.DIRECT)
def test_filter2d_direct_form(emu, h, w, kh, kw):
    """filter2d_tile: the smallest kernel without a matrix-core form, patches above 64 KiB and just under the 160 KiB
    limit, ragged tiles, an even kernel height, a Gabor kernel of ksize 120 on a 0-255 image (tests/image_cases.py)."""
    assert emu.d4w_filter2d_mm_eligible(kh, kw) == 0
    e = ic.filter2d_rel(run_filter2d(emu), *ic.direct_case(h, w, kh, kw))
    print("direct %s rel %.2e" % ((h, w, kh, kw), e))
    assert e < TOL


def test_filter2d_direct_form_accumulates(emu):
    run = run_filter2d(emu)
    img, k1 = ic.noise_case(10, 70, 3, 114)
    k2 = ic.noise_case(11, 70, 3, 114)[1]
    out = run(img, k1)
    out = run(img, k2, accumulate=1, out=out)
    ref = orc.filter2d(img.astype(np.float64), k1.astype(np.float64)) + orc.filter2d(img.astype(np.float64), k2.astype(np.float64))
    assert rel(out, ref) < TOL


@pytest.mark.parametrize("h,w,kh,kw", ic.WIDE[:2] + ic.TILE_EDGES + ic.RING_EDGES + ic.SHORT_IMAGES)
def test_filter2d_matrix_core_edges(emu, h, w, kh, kw):
    """filter2d_mm_rows: several workgroups per row block with kernels as deep as the prefetch ring, images that end on,
    before and after a 256-column tile, kernel heights around the prefetch ring and the row ring, images shorter than the
    kernel and than a row group."""
    assert emu.d4w_filter2d_mm_eligible(kh, kw) == 1
    e = ic.filter2d_rel(run_filter2d(emu), *ic.noise_case(h, w, kh, kw))
    print("matrix cores %s rel %.2e" % ((h, w, kh, kw), e))
    assert e < TOL


def test_filter2d_value_ranges(emu):
    print(ic.check_values(run_filter2d(emu)))


@pytest.mark.parametrize("kh,kw", ic.NONFINITE)
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_filter2d_one_nonfinite_pixel(emu, kh, kw, bad):
    """One NaN or inf pixel spreads beyond its kh x kw window in both forms; what stays finite is right."""
    n, e = ic.check_nonfinite(run_filter2d(emu), kh, kw, bad)
    print("%s pixel, kernel %d x %d: %d of 8000 outputs non-finite, finite ones rel %.2e" % (bad, kh, kw, n, e))


@pytest.mark.parametrize("h,w,oh,ow", ic.RESIZE)
def test_resize_unstaged_branch_and_neighbours(emu, h, w, oh, ow):
    """resize_rows reads global memory directly when a workgroup's 256 outputs span more than 4096 inputs; the span of
    every case is taken from the oracle's weight table to prove which side of that threshold it is on."""
    spans = ic.check_resize_side(w, ow)
    rng = np.random.default_rng(w + ow)
    x = f32(rng.standard_normal((h, w)))
    emu.d4w_resize_ws_bytes.restype = sz

    def resize(a):
        y = np.empty((oh, ow), dtype=np.float32)
        ws = np.empty(emu.d4w_resize_ws_bytes(h, w, oh, ow), dtype=np.uint8)
        assert emu.d4w_resize_bilinear_aa_f32(vp(a), h, w, vp(y), oh, ow, vp(ws), None) == 0, emu.d4w_last_error()
        return y
    e = rel(resize(x), orc.resize_bilinear_aa(x.astype(np.float64), oh, ow))
    print("resize %s spans %s rel %.2e" % ((h, w, oh, ow), spans[:3], e))
    assert e < TOL
    m = rng.random((h, w)) > 0.97
    assert np.array_equal(resize(f32(m)) != 0, orc.resize_bilinear_aa(m.astype(np.float64), oh, ow) != 0)


@pytest.mark.parametrize("n", ic.MINMAX_N)
def test_minmax_forms_and_nonfinite_values(emu, n):
    mm = np.zeros(2, dtype=np.float32)
    for name, x in ic.minmax_cases(n):
        assert emu.d4w_minmax_f32(vp(x), sz(n), vp(mm), None) == 0
        ic.check_minmax(name, x, mm)


def test_scale_constant_image_and_threshold_in_float64(emu):
    x = np.full(700, 3.5, dtype=np.float32)
    mm = np.zeros(2, dtype=np.float32)
    y = np.zeros_like(x)
    assert emu.d4w_minmax_f32(vp(x), sz(x.size), vp(mm), None) == 0
    assert emu.d4w_scale_pixels_f32(vp(x), vp(y), sz(x.size), vp(mm), ctypes.c_double(255.0), None) == 0
    with np.errstate(invalid="ignore"):
        ref = orc.scale_pixels(x.astype(np.float64)) * 255
    assert np.array_equal(np.isnan(y), np.isnan(ref)) and np.isnan(ref).all()
    x, want = ic.threshold_inputs(0.1)
    y = np.empty_like(x)
    assert emu.d4w_threshold_f32(vp(x), vp(y), sz(x.size), ctypes.c_double(0.1), None) == 0
    assert np.array_equal(y != 0, want)


def test_filter2d_refuses_kernels_beyond_the_lds_before_any_launch(emu):
    emu.d4w_filter2d_ws_bytes.restype = sz
    img = f32(np.random.default_rng(3).standard_normal((8, 40)))
    for kh, kw in ic.REFUSED:
        ker = np.ones((kh, kw), dtype=np.float32)
        out = np.full_like(img, 7.0)
        ws = np.full(emu.d4w_filter2d_ws_bytes(kh, kw), 0x5a, dtype=np.uint8)
        assert emu.d4w_filter2d_f32(vp(img), 8, 40, vp(ker), kh, kw, vp(out), 0, vp(ws), None) == -1
        assert b"bytes of LDS" in emu.d4w_last_error()
        assert np.all(out == 7.0) and np.all(ws == 0x5a)               # nothing ran: neither the padded kernel nor an output
    assert ic.filter2d_rel(run_filter2d(emu), *ic.noise_case(8, 40, 3, 114)) < TOL


def test_filter2d_rejects_oversized_kernel_and_inplace(emu):
    img = np.zeros((8, 8), dtype=np.float32)
    ker = np.zeros((301, 301), dtype=np.float32)
    ws = np.empty(4 * 301 * 320, dtype=np.uint8)
    assert emu.d4w_filter2d_f32(vp(img), 8, 8, vp(ker), 301, 301, vp(np.empty_like(img)), 0, vp(ws), None) != 0
    assert emu.d4w_filter2d_f32(vp(img), 8, 8, vp(ker), 3, 3, vp(img), 0, vp(ws), None) != 0


def test_analytic_env_over_std(emu):
    rng = np.random.default_rng(5)
    x = f32(rng.standard_normal((5, 400)) * rng.uniform(0.5, 3, (5, 1)))
    var = np.empty(5, dtype=np.float32)
    y = np.empty_like(x)
    assert emu.d4w_row_var_f32(vp(x), 5, 400, vp(var), None) == 0
    assert emu.d4w_analytic_f32(vp(x), vp(y), 5, 400, 4, vp(var), ctypes.c_double(0.0), None) == 0, emu.d4w_last_error()
    x64 = x.astype(np.float64)
    assert rel(y, np.abs(orc.hilbert(x64)) / np.std(x64, axis=1, keepdims=True)) < TOL
