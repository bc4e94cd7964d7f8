"""GPU tests of csrc/resample.hip through the Python interface: dsp.resample_poly, dsp.decimate, dsp.resample_reach and the
fused ingest (data_handle.load_das_data_array / PinnedIngest.strain with decimate=q), against scipy.signal in float64 with the
cases and the tolerance of tests/resample_cases.py (1e-5 of every row's maximum)."""
import ctypes

import numpy as np
import pytest
import scipy.signal as sps
import torch

from tests import resample_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import das4whales_amd as dw_
    from das4whales_amd import _lib
    assert "gfx950" in _lib.version()
    return dw_


@pytest.mark.parametrize("name", sorted(rc.GPU_CASES))
def test_resample_poly_matches_scipy(dw, name):
    nx, ns, up, down, win, padtype, cval = rc.GPU_CASES[name]
    y = dw.dsp.resample_poly(rc.make_input(name), up, down, window=rc.window_of(win), padtype=padtype, cval=cval)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32
    rc.check_rows(y, rc.reference(name), name)


def test_reduced_to_one_is_a_copy(dw):
    nx, ns, up, down = rc.COPY_CASE
    x = rc.rows(nx, ns, 310)
    assert np.array_equal(dw.dsp.resample_poly(x, up, down), x)
    assert np.array_equal(dw.dsp.resample_poly(x, up, down, padtype="mean"), x)


def test_unaligned_base_and_row_subset(dw):
    """The block starts 4, 8 and 12 bytes into a 16-byte slot; every second row of a resident block is read in place."""
    name = "1001_1_5"
    nx, ns, up, down = rc.GPU_CASES[name][:4]
    want = dw.dsp.resample_poly(rc.make_input(name), up, down)
    buf = torch.zeros(nx * ns + 4, dtype=torch.float32, device="cuda")
    for shift in (1, 2, 3):
        x = buf[shift:shift + nx * ns].view(nx, ns)
        x.copy_(torch.from_numpy(np.array(rc.make_input(name))))
        assert x.data_ptr() % 16 == 4 * shift
        y = dw.dsp.resample_poly(x, up, down).cpu().numpy()
        rc.check_rows(y, rc.reference(name), "%s + %d floats" % (name, shift))
        assert np.array_equal(y, want)
    big = torch.zeros((2 * nx, ns), dtype=torch.float32, device="cuda")
    big[::2] = torch.from_numpy(np.array(rc.make_input(name))).cuda()
    assert np.array_equal(dw.dsp.resample_poly(big[::2], up, down).cpu().numpy(), want)


@pytest.mark.parametrize("name", sorted(rc.DECIMATE_CASES))
def test_decimate_matches_scipy(dw, name):
    ns, q, n = rc.DECIMATE_CASES[name]
    y = dw.dsp.decimate(rc.decimate_input(name), q, n=n)
    rc.check_rows(y, rc.decimate_reference(name), "decimate " + name)


def test_refused_forms(dw):
    x = rc.rows(2, 1001, 311)
    with pytest.raises(ValueError):
        dw.dsp.decimate(x, 5, ftype="iir")
    with pytest.raises(ValueError):
        dw.dsp.decimate(x, 5, zero_phase=False)
    with pytest.raises(ValueError, match="'constant' and 'mean'"):
        dw.dsp.resample_poly(x, 1, 5, padtype="line")
    with pytest.raises(ValueError, match="taps"):
        dw.dsp.resample_poly(x, 1, 5, window=np.ones(2049))
    with pytest.raises(ValueError, match="taps"):
        dw.dsp.resample_poly(x, 1, 103)                                  # 20 x 103 + 1 designed taps
    with pytest.raises(ValueError, match="line up"):
        dw.dsp.resample_poly(x, 1, 5, prev_tail=np.zeros((2, 50), dtype=np.float32))      # 1001 is no multiple of 5
    with pytest.raises(ValueError, match="line up"):
        dw.dsp.resample_poly(x[:, :1000], 2, 3, next_head=np.zeros((2, 50), dtype=np.float32))
    for up, down in ((0, 5), (1, 0), (-1, 2)):
        with pytest.raises(ValueError):
            dw.dsp.resample_poly(x, up, down)
    with pytest.raises(ValueError):
        dw.dsp.resample_poly(x, 1, 5, axis=0)
    assert dw.dsp.resample_poly(x, 1, 5, window=np.ones(2048)).shape == (2, 201)        # the longest accepted
    assert dw.dsp.resample_poly(x, 1, 5, axis=1).shape == (2, 201)


def test_containers_and_stream(dw):
    """float64 NumPy in -> float64 out, the float32 result cast; a device tensor in -> a device tensor out, computed on the
    current (non-default) stream, the same bits; 1-D in -> 1-D out."""
    name = "777_2_5"
    nx, ns, up, down = rc.GPU_CASES[name][:4]
    x32 = rc.make_input(name)
    y32 = dw.dsp.resample_poly(x32, up, down)
    y64 = dw.dsp.resample_poly(x32.astype(np.float64), up, down)
    assert y64.dtype == np.float64 and np.array_equal(y64, y32.astype(np.float64))
    xt = torch.from_numpy(np.array(x32)).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        yt = dw.dsp.resample_poly(xt, up, down)
        dt = dw.dsp.decimate(xt, 5)
    side.synchronize()
    assert isinstance(yt, torch.Tensor) and yt.is_cuda and yt.dtype == torch.float32
    assert np.array_equal(yt.cpu().numpy(), y32)
    assert np.array_equal(dt.cpu().numpy(), dw.dsp.decimate(x32, 5))
    rc.check_rows(yt.cpu().numpy(), rc.reference(name), name + " (tensor, side stream)")
    y1 = dw.dsp.resample_poly(x32[1], up, down)
    assert y1.shape == (y32.shape[1],) and np.array_equal(y1, y32[1])
    assert np.array_equal(dw.dsp.resample_poly(x32[1], up, down, axis=0), y1)
    d1 = dw.dsp.decimate(xt[2], 5)
    assert d1.shape == (dt.shape[1],) and torch.equal(d1, dt[2])


@pytest.mark.parametrize("name", sorted(rc.CONTINUATION))
def test_continuation_is_bit_exact(dw, name):
    """Each of the three files of a record, with resample_reach samples of its neighbours, equals its columns of the whole
    record's result bit for bit; one sample short of the reach it does not (99-tap cases, see resample_cases)."""
    up, down, win = rc.CONTINUATION[name]
    window = rc.continuation_window(win)
    whole = rc.record()
    ns = rc.RECORD_FILE_NS
    n_out = ns * up // down
    nl, nr = dw.dsp.resample_reach(up, down, window)
    full = dw.dsp.resample_poly(whole, up, down, window=window)
    rc.check_rows(full, sps.resample_poly(whole.astype(np.float64), up, down, axis=-1, window=window), "record " + name)
    dev_whole = torch.from_numpy(np.array(whole)).cuda()
    for f in range(rc.RECORD_FILES):
        a, b = f * ns, (f + 1) * ns
        want = full[:, f * n_out:(f + 1) * n_out]
        left = whole[:, a - nl:a] if f > 0 else None
        right = whole[:, b:b + nr] if f + 1 < rc.RECORD_FILES else None
        assert np.array_equal(dw.dsp.resample_poly(whole[:, a:b], up, down, window=window, prev_tail=left, next_head=right), want)
        # the same on slices of a resident record, read in place
        yt = dw.dsp.resample_poly(dev_whole[:, a:b], up, down, window=window,
                                  prev_tail=None if f == 0 else dev_whole[:, a - nl:a],
                                  next_head=None if right is None else dev_whole[:, b:b + nr])
        assert np.array_equal(yt.cpu().numpy(), want)
        for short_left, short_right in ((1, 0), (0, 1)):
            if (short_left and left is None) or (short_right and right is None):
                continue
            y = dw.dsp.resample_poly(whole[:, a:b], up, down, window=window,
                                     prev_tail=None if left is None else left[:, short_left:],
                                     next_head=None if right is None else right[:, :nr - short_right])
            differs = not np.array_equal(y, want)
            print("continuation %s file %d, %s one sample short: differs = %s" % (name, f, "left" if short_left else "right", differs))
            if win == "taps99":
                assert differs, (name, f, short_left, short_right)
    assert not np.array_equal(dw.dsp.resample_poly(whole[:, ns:2 * ns], up, down, window=window), full[:, n_out:2 * n_out])


def check_ingest(out, dtype):
    y, tx, dist = out
    c0, c1, step = rc.INGEST_SEL
    nx, n_out = len(range(c0, c1, step)), -(-4000 // rc.INGEST_Q)
    assert isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (nx, n_out)
    assert np.array_equal(tx, np.arange(n_out) * rc.INGEST_Q / rc.INGEST_META["fs"])
    assert np.array_equal(dist, (np.arange(nx) * step + c0) * rc.INGEST_META["dx"])
    rc.check_rows(y.cpu().numpy(), rc.ingest_reference(dtype), "ingest " + dtype)


@pytest.mark.parametrize("dtype", sorted(rc.INGEST_OFFSETS))
def test_fused_ingest(dw, dtype):
    from das4whales_amd import _device as dev
    from das4whales_amd._lib import lib
    raw = rc.ingest_raw(dtype)
    meta = dict(rc.INGEST_META)
    check_ingest(dw.data_handle.load_das_data_array(raw, rc.INGEST_SEL, meta, decimate=rc.INGEST_Q), dtype)
    assert meta == rc.INGEST_META                                       # the caller's rate is now fs / q; metadata is the caller's
    # decimate=None: today's path, bit for bit what d4w_raw2strain_f32 gives on the same input
    y, tx, dist = dw.data_handle.load_das_data_array(raw, rc.INGEST_SEL, meta)
    t = torch.from_numpy(np.array(raw)).cuda()
    c0, c1, step = rc.INGEST_SEL
    nx, ns = len(range(c0, c1, step)), raw.shape[1]
    direct = torch.empty((nx, ns), dtype=torch.float32, device="cuda")
    assert lib.d4w_raw2strain_f32(dev.ptr(t), {"int32": 0, "int16": 1, "float32": 2}[dtype], ns, c0, step, nx,
                                  ctypes.c_double(meta["scale_factor"]), dev.ptr(direct), dev.stream_ptr(t)) == 0
    assert tuple(y.shape) == (nx, ns) and torch.equal(y, direct) and np.array_equal(tx, np.arange(ns) / meta["fs"])
    y1, tx1, _ = dw.data_handle.load_das_data_array(raw, rc.INGEST_SEL, meta, decimate=1)
    assert torch.equal(y1, y) and np.array_equal(tx1, tx)
    # the same through the pinned ingest
    ing = dw.data_handle.PinnedIngest(raw.shape, np.dtype(dtype))
    np.copyto(ing.host_array(0), raw)
    ing.upload(0)
    check_ingest(ing.strain(0, rc.INGEST_SEL, meta, decimate=rc.INGEST_Q), dtype)
    ing.upload(0)
    y2, _, _ = ing.strain(0, rc.INGEST_SEL, meta)
    assert torch.equal(y2, y)
    torch.cuda.synchronize()


def test_fused_ingest_equals_ingest_then_decimate_closely(dw):
    """The fused path against load_das_data_array followed by dsp.decimate: the same taps on the same strain, the mean
    removed before instead of after the rounding to float32."""
    raw = rc.ingest_raw("int32")
    fused = dw.data_handle.load_das_data_array(raw, rc.INGEST_SEL, rc.INGEST_META, decimate=rc.INGEST_Q)[0].cpu().numpy()
    strain = dw.data_handle.load_das_data_array(raw, rc.INGEST_SEL, rc.INGEST_META)[0]
    two_step = dw.dsp.decimate(strain, rc.INGEST_Q).cpu().numpy()
    rc.check_rows(two_step, rc.ingest_reference("int32"), "ingest, then decimate")
    # both lie within TOL of the same reference row by row, so they lie within 2 TOL of each other
    assert np.all(np.abs(fused - two_step).max(axis=1) <= 2 * rc.TOL * np.abs(rc.ingest_reference("int32")).max(axis=1))
