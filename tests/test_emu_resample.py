"""Polyphase resampler LOGIC (csrc/resample.hip) on the CPU emulator build: same HIP source, same C ABI, host pointers,
against scipy.signal.resample_poly / decimate in float64 on the float32-rounded input (cases and tolerance:
tests/resample_cases.py).  The taps come from the product's host code (das4whales_amd.dsp)."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import scipy.signal as sps

from tests import resample_cases as rc
from tests.emu_util import load_emu, vp

DTYPE_CODE = {"int32": 0, "int16": 1, "float32": 2, "float64": 3}


@pytest.fixture(scope="module")
def emu():
    return load_emu()


@pytest.fixture(scope="module")
def dsp():
    from das4whales_amd import dsp as dsp_
    return dsp_


def pitch(a):
    return ctypes.c_size_t(a.strides[0] // 4)


def resample(lib, x, up, down, h, off=None, off_const=0.0, scale=1.0, add_back=1, left=None, right=None, expect=0):
    """d4w_resample_f32 on host arrays; x, left and right may be column slices of a larger block (read in place)."""
    nx, ns = x.shape
    y = np.full((nx, lib.d4w_resample_out_len(ns, up, down)), np.nan, dtype=np.float32)
    h32 = np.ascontiguousarray(h, dtype=np.float32)                   # rounded to float32 once
    rcode = lib.d4w_resample_f32(vp(x), pitch(x), nx, ns,
                                 None if left is None else vp(left), pitch(left) if left is not None else ctypes.c_size_t(0),
                                 0 if left is None else left.shape[1],
                                 None if right is None else vp(right), pitch(right) if right is not None else ctypes.c_size_t(0),
                                 0 if right is None else right.shape[1],
                                 vp(h32), h32.size, up, down, None if off is None else vp(off), ctypes.c_double(off_const),
                                 ctypes.c_double(scale), add_back, vp(y), None)
    assert rcode == expect, lib.d4w_last_error()
    return y


def run_case(lib, dsp, x, up, down, win, padtype, cval):
    upr, downr, h = dsp._resample_taps(up, down, rc.window_of(win))
    assert (upr, downr) == (up // math.gcd(up, down), down // math.gcd(up, down))
    off = None
    if padtype == "mean":
        nx, ns = x.shape
        off = np.full(nx, np.nan)
        mx = np.zeros(nx, dtype=np.float32)
        assert lib.d4w_row_stats_f32(vp(x), nx, ns, vp(off), vp(mx), None) == 0
    return resample(lib, x, up, down, h, off=off, off_const=0.0 if cval is None else cval, add_back=1 if padtype == "mean" else 2)


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_resample_matches_scipy(emu, dsp, name):
    nx, ns, up, down, win, padtype, cval = rc.CASES[name]
    ref = rc.reference(name)
    assert emu.d4w_resample_out_len(ns, up, down) == ref.shape[1]
    rc.check_rows(run_case(emu, dsp, rc.make_input(name), up, down, win, padtype, cval), ref, name)


def test_resample_reduced_to_one_is_a_copy(emu, dsp):
    nx, ns, up, down = rc.COPY_CASE
    x = rc.rows(nx, ns, 310)
    _, _, h = dsp._resample_taps(up, down, rc.DEFAULT_WINDOW)
    assert np.array_equal(resample(emu, x, up, down, h), x)
    wide = np.zeros((nx, ns + 7), dtype=np.float32)                   # rows with a pitch
    wide[:, 3:3 + ns] = x
    assert np.array_equal(resample(emu, wide[:, 3:3 + ns], up, down, h), x)


def test_resample_unaligned_base(emu, dsp):
    """The block itself starts 4, 8 and 12 bytes into a 16-byte slot."""
    name = "1001_1_5"
    nx, ns, up, down, win, padtype, cval = rc.CASES[name]
    buf = np.zeros(nx * ns + 4, dtype=np.float32)
    first = None
    for shift in (1, 2, 3):
        x = buf[shift:shift + nx * ns].reshape(nx, ns)
        x[:] = rc.make_input(name)
        y = run_case(emu, dsp, x, up, down, win, padtype, cval)
        rc.check_rows(y, rc.reference(name), "%s + %d floats" % (name, shift))
        first = y if first is None else first
        assert np.array_equal(y, first)


@pytest.mark.parametrize("name", sorted(rc.DECIMATE_CASES))
def test_decimate_taps_match_scipy(emu, dsp, name):
    ns, q, n = rc.DECIMATE_CASES[name]
    h = dsp._decimate_taps(q, n)
    assert h.size == (20 * q if n is None else n) + 1
    rc.check_rows(resample(emu, rc.decimate_input(name), 1, q, h), rc.decimate_reference(name), "decimate " + name)


def test_signatures_are_scipys(dsp):
    """Parameter names and defaults equal SciPy's, except resample_poly's axis (time is last here) and decimate's ftype (only
    'fir' is built); the continuation blocks are keyword-only additions."""
    ours, theirs = inspect.signature(dsp.resample_poly), inspect.signature(sps.resample_poly)
    mine = [(p.name, p.default) for p in ours.parameters.values() if p.kind != p.KEYWORD_ONLY]
    assert [n for n, _ in mine][1:] == [p.name for p in theirs.parameters.values()][1:]
    assert {n: v for n, v in mine if n not in ("x", "trace", "axis")} == \
        {p.name: p.default for p in theirs.parameters.values() if p.name not in ("x", "axis")}
    assert ours.parameters["axis"].default == -1
    assert [p.name for p in ours.parameters.values() if p.kind == p.KEYWORD_ONLY] == ["prev_tail", "next_head"]
    ours, theirs = inspect.signature(dsp.decimate), inspect.signature(sps.decimate)
    assert [p.name for p in ours.parameters.values()][1:] == [p.name for p in theirs.parameters.values()][1:]
    assert {p.name: p.default for p in ours.parameters.values() if p.name not in ("trace", "ftype")} == \
        {p.name: p.default for p in theirs.parameters.values() if p.name not in ("x", "ftype")}
    assert ours.parameters["ftype"].default == "fir"


def test_refused_forms_need_no_device(dsp):
    x = np.zeros((2, 100), dtype=np.float32)
    with pytest.raises(ValueError, match="fir"):
        dsp.decimate(x, 5, ftype="iir")
    with pytest.raises(ValueError, match="zero_phase"):
        dsp.decimate(x, 5, zero_phase=False)
    for padtype in ("line", "median", "maximum", "minimum", "symmetric", "reflect", "edge", "wrap"):
        with pytest.raises(ValueError, match="'constant' and 'mean'"):
            dsp.resample_poly(x, 1, 5, padtype=padtype)
    with pytest.raises(ValueError):
        dsp.resample_poly(x, 1, 5, axis=0)
    for up, down in ((0, 5), (1, 0), (-1, 2)):
        with pytest.raises(ValueError):
            dsp.resample_poly(x, up, down)
    with pytest.raises(ValueError, match="padtype='constant'"):
        dsp.resample_poly(x, 1, 5, padtype="mean", prev_tail=np.zeros((2, 50), dtype=np.float32))


def test_helpers(emu, dsp):
    assert emu.d4w_resample_max_taps() >= 641
    assert [emu.d4w_resample_out_len(*a) for a in ((1000, 1, 5), (1001, 1, 5), (777, 2, 5), (500, 5, 1), (1, 1, 5), (0, 1, 5))] \
        == [200, 201, 311, 2500, 1, 0]
    nl, nr = ctypes.c_int(-1), ctypes.c_int(-1)
    for ntaps, up, down, want in ((101, 1, 5, (50, 46)), (101, 2, 5, (25, 23)), (101, 4, 10, (25, 23)), (40, 1, 4, (20, 16)),
                                  (3, 1, 5, (1, 0)), (1, 1, 2, (0, 0))):
        assert emu.d4w_resample_reach(ntaps, up, down, ctypes.byref(nl), ctypes.byref(nr)) == 0
        assert (nl.value, nr.value) == want, (ntaps, up, down)


def test_argument_errors(emu):
    x = np.zeros((2, 1001), dtype=np.float32)
    h = np.ones(11)
    for up, down in ((0, 5), (1, 0), (-2, 3)):
        y = np.zeros((2, 4096), dtype=np.float32)
        assert emu.d4w_resample_f32(vp(x), pitch(x), 2, 1001, None, ctypes.c_size_t(0), 0, None, ctypes.c_size_t(0), 0,
                                    vp(np.ones(11, dtype=np.float32)), 11, up, down, None, ctypes.c_double(0), ctypes.c_double(1), 0,
                                    vp(y), None) == -1
        assert b"positive" in emu.d4w_last_error() and not y.any()
    too_long = np.ones(emu.d4w_resample_max_taps() + 1)
    resample(emu, x, 1, 5, too_long, expect=-1)
    assert b"taps" in emu.d4w_last_error()
    resample(emu, x, 1, 5, np.ones(emu.d4w_resample_max_taps()))      # the longest accepted
    resample(emu, x, 257, 1, h, expect=-1)
    resample(emu, x, 1, 257, h, expect=-1)
    nb = np.zeros((2, 5), dtype=np.float32)
    resample(emu, x, 1, 5, h, left=nb, expect=-1)                     # 1001 is no multiple of 5
    assert b"line up" in emu.d4w_last_error()
    resample(emu, x, 2, 5, h, right=nb, expect=-1)
    resample(emu, x[:, :1000], 1, 5, h, left=nb, right=nb)            # 1000 is


@pytest.mark.parametrize("name", sorted(rc.CONTINUATION))
def test_continuation_is_bit_exact(emu, dsp, name):
    """Each of the three files of a record, with resample_reach samples of its neighbours read in place, equals its columns
    of the whole record's result bit for bit; one sample short of the reach it does not (99-tap cases, see resample_cases)."""
    up, down, win = rc.CONTINUATION[name]
    window = rc.continuation_window(win)
    _, _, h = dsp._resample_taps(up, down, window)
    whole = rc.record()
    ns = rc.RECORD_FILE_NS
    n_out = ns * up // down
    nl, nr = dsp.resample_reach(up, down, window)
    assert 0 < nl < ns and 0 < nr < ns
    full = resample(emu, whole, up, down, h)
    rc.check_rows(full, sps.resample_poly(whole.astype(np.float64), up, down, axis=-1, window=window), "record " + name)
    for f in range(rc.RECORD_FILES):
        a, b = f * ns, (f + 1) * ns
        want = full[:, f * n_out:(f + 1) * n_out]
        left = whole[:, a - nl:a] if f > 0 else None
        right = whole[:, b:b + nr] if f + 1 < rc.RECORD_FILES else None
        assert np.array_equal(resample(emu, whole[:, a:b], up, down, h, left=left, right=right), want), (name, f)
        for short_left, short_right in ((1, 0), (0, 1)):
            l2 = left[:, short_left:] if left is not None else None
            r2 = right[:, :nr - short_right] if right is not None else None
            if (short_left and l2 is None) or (short_right and r2 is None):
                continue
            differs = not np.array_equal(resample(emu, whole[:, a:b], up, down, h, left=l2, right=r2), want)
            print("continuation %s file %d, %s one sample short: differs = %s" % (name, f, "left" if short_left else "right", differs))
            if win == "taps99":
                assert differs, (name, f, short_left, short_right)
    alone = resample(emu, whole[:, ns:2 * ns], up, down, h)
    assert not np.array_equal(alone, full[:, n_out:2 * n_out])


@pytest.mark.parametrize("dtype", sorted(rc.INGEST_OFFSETS))
def test_fused_ingest(emu, dsp, dtype):
    raw = rc.ingest_raw(dtype)
    ref = rc.ingest_reference(dtype)
    c0, c1, step = rc.INGEST_SEL
    nx, ns, q = len(range(c0, c1, step)), raw.shape[1], rc.INGEST_Q
    mean = np.full(nx, np.nan)
    assert emu.d4w_raw_row_mean_f64(vp(raw), DTYPE_CODE[dtype], ns, c0, step, nx, vp(mean), None) == 0, emu.d4w_last_error()
    sel = raw[c0:c1:step]
    want = sel.astype(np.float64).mean(axis=1)
    assert np.max(np.abs(mean - want)) <= 1e-15 * np.max(np.abs(want)) + 1e-13
    h32 = np.ascontiguousarray(dsp._decimate_taps(q), dtype=np.float32)
    y = np.full((nx, emu.d4w_resample_out_len(ns, 1, q)), np.nan, dtype=np.float32)
    assert emu.d4w_resample_raw_f32(vp(raw), DTYPE_CODE[dtype], ns, c0, step, nx, vp(h32), h32.size, 1, q, vp(mean),
                                    ctypes.c_double(rc.INGEST_META["scale_factor"]), vp(y), None) == 0, emu.d4w_last_error()
    assert y.shape == (nx, 800)
    rc.check_rows(y, ref, "ingest " + dtype)
    assert emu.d4w_resample_raw_f32(vp(raw), DTYPE_CODE[dtype], ns, c0, step, nx, vp(h32), h32.size, 3, 3, vp(mean),
                                    ctypes.c_double(1.0), vp(y), None) == -1
    assert emu.d4w_resample_raw_f32(vp(raw), 7, ns, c0, step, nx, vp(h32), h32.size, 1, q, vp(mean), ctypes.c_double(1.0), vp(y), None) == -1


def test_raw_row_mean_is_exact_for_long_int32_rows(emu):
    """600 000 int32 samples at an offset of 2e9: the sum (1.2e15) is formed in integers."""
    rng = np.random.default_rng(77)
    raw = (2_000_000_000 + rng.integers(-1000, 1000, size=(3, 600_000))).astype(np.int32)
    mean = np.full(2, np.nan)
    assert emu.d4w_raw_row_mean_f64(vp(raw), 0, 600_000, 0, 2, 2, vp(mean), None) == 0
    want = [int(raw[r].astype(np.int64).sum()) / 600_000 for r in (0, 2)]
    assert mean.tolist() == want
