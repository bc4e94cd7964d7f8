"""Row quantiles, the per-channel noise floor and per-row pick thresholds (csrc/row_select.h, csrc/noise.hip, csrc/peaks.hip) in the CPU
emulator build through the C ABI on host pointers, against the float64 restatement of tests/known_answers_noise.py.  Kernel
logic only; the cases and bars are those of tests/noise_cases.py, which the hardware runs as well (tests/test_noise_gpu.py).
Every output lies between guards that must come back untouched.  No case is skipped or excluded."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import known_answers_noise as kn
from tests import noise_cases as nc
from tests.emu_util import load_emu, vp

SZ = ctypes.c_size_t
GUARD = 64


@pytest.fixture(scope="module")
def lib():
    lib = load_emu()
    lib.d4w_channel_noise_ws_bytes.restype = SZ
    return lib


def max_q(lib):
    m = ctypes.c_int()
    assert lib.d4w_row_quantile_limits(ctypes.byref(m)) == 0
    return m.value


def guarded(shape):
    n = int(np.prod(shape))
    whole = np.full(n + 2 * GUARD, -7, dtype=np.float32)
    return whole, whole[GUARD:GUARD + n].reshape(shape)


def intact(whole):
    return np.all(whole[:GUARD] == -7) and np.all(whole[len(whole) - GUARD:] == -7)


def dbl(q):
    return (ctypes.c_double * max(len(q), 1))(*q)


def quantile(lib, rows, q, pad=0):
    """rows [nx, n] -> [nx, nq]; pad > 0: the rows sit in a wider block (ld = n + pad) whose other columns are NaN."""
    nx, n = rows.shape
    block = np.full((nx, n + pad), np.nan, dtype=np.float32)
    block[:, :n] = rows
    whole, out = guarded((nx, len(q)))
    rc = lib.d4w_row_quantile_f32(vp(block), nx, SZ(n), SZ(n + pad), dbl(q), len(q), vp(out), None)
    assert rc == 0, lib.d4w_last_error()
    assert intact(whole)
    return out.copy()


def test_limits(lib):
    assert max_q(lib) >= 8


@pytest.mark.parametrize("n", nc.LENGTHS)
def test_row_quantile(lib, n):
    rows = np.stack([nc.row(kind, n) for kind in nc.ROW_KINDS])
    for q in nc.quantile_sets(max_q(lib)):
        nc.check_quantiles(quantile(lib, rows, q), rows, q)


@pytest.mark.parametrize("n", (5, 2049))
def test_row_quantile_reads_a_window_in_place(lib, n):
    rows = np.stack([nc.row(kind, n, seed=1) for kind in nc.ROW_KINDS])
    q = nc.quantile_sets(max_q(lib))[1]
    got = quantile(lib, rows, q, pad=3)
    nc.check_quantiles(got, rows, q)
    assert np.array_equal(got, quantile(lib, rows, q), equal_nan=True)


def test_row_quantile_rows_are_independent(lib):
    rows = np.stack([nc.row(kind, 2049, seed=2) for kind in nc.ROW_KINDS])
    q = [0.5, 0.25]
    both = quantile(lib, rows, q)
    for c in (0, 5, len(rows) - 1):
        assert np.array_equal(quantile(lib, rows[c:c + 1], q), both[c:c + 1], equal_nan=True)


# ------------------------------------------------------------------------------------------
# channel noise
# ------------------------------------------------------------------------------------------
def noise(lib, block, a, b, q, how, which=(True, True, True, True)):
    """The call on block[:, a:b], read in place; outputs not in `which` are NULL (and come back as None)."""
    nx, ld = block.shape
    ns = b - a
    outs = [guarded((nx,)), guarded((nx,)), guarded((nx,)), guarded((nx, max(len(q), 1)))]
    if not len(q):
        which = which[:3] + (False,)
    ws = np.empty(max(lib.d4w_channel_noise_ws_bytes(nx, ns), 8), dtype=np.uint8)
    ptr = [vp(o[1]) if w else None for o, w in zip(outs, which)]
    x = block.reshape(-1)[a:]
    rc = lib.d4w_channel_noise_f32(vp(x), nx, ns, SZ(ld), dbl(q), len(q), ptr[0], ptr[1], ptr[2], ptr[3], vp(ws), how, None)
    assert rc == 0, lib.d4w_last_error()
    for (whole, view), w in zip(outs, which):
        assert intact(whole)
        if not w:
            assert np.all(view == -7)
    res = [o[1].copy() if w else None for o, w in zip(outs, which)]
    if res[3] is not None:
        res[3] = res[3][:, :len(q)]
    return res


@pytest.mark.parametrize("ns", (480, 2018, 4095))
@pytest.mark.parametrize("how", (1, 2))
def test_channel_noise(lib, ns, how):
    assert lib.d4w_channel_noise_fits_lds(ns) == 1
    x = nc.noise_block(3, ns)
    got = noise(lib, x, 0, ns, nc.NOISE_Q, how)
    print(how, ns, nc.check_noise(got, x, nc.NOISE_Q))
    again = noise(lib, x, 0, ns, nc.NOISE_Q, how)
    assert all(np.array_equal(g, h) for g, h in zip(got, again))
    one = noise(lib, x[1:2].copy(), 0, ns, nc.NOISE_Q, how)                 # a row alone: the same bits
    assert all(np.array_equal(g[1:2], h) for g, h in zip(got, one))
    auto = noise(lib, x, 0, ns, nc.NOISE_Q, 0)                               # these lengths fit: auto is the one-read form
    if how == 1:
        assert all(np.array_equal(g, h) for g, h in zip(got, auto))


@pytest.mark.parametrize("how", (1, 2))
def test_channel_noise_null_outputs_in_every_combination(lib, how):
    ns = 480
    x = nc.noise_block(3, ns)
    full = noise(lib, x, 0, ns, nc.NOISE_Q, how)
    for which in itertools.product((False, True), repeat=4):
        got = noise(lib, x, 0, ns, nc.NOISE_Q, how, which)
        for g, f, w in zip(got, full, which):
            assert (g is None) if not w else np.array_equal(g, f)
    got = noise(lib, x, 0, ns, (), how)                                      # nq = 0
    assert got[3] is None and all(np.array_equal(g, f) for g, f in zip(got[:3], full[:3]))


@pytest.mark.parametrize("how", (1, 2))
@pytest.mark.parametrize("a,b", ((1, 481), (3, 2021), (2, 481)))
def test_channel_noise_of_a_window(lib, how, a, b):
    """Odd start and even length: rows that are only 4-byte aligned (the packed form's 8-byte loads are not allowed); an even
    start and an odd length as well.  The Hilbert transform is that of the window."""
    x = nc.noise_block(3, 2100)
    got = noise(lib, x, a, b, nc.NOISE_Q, how)
    nc.check_noise(got, x, nc.NOISE_Q, (a, b))
    alone = noise(lib, np.ascontiguousarray(x[:, a:b]), 0, b - a, nc.NOISE_Q, how)
    assert all(np.array_equal(g, h) for g, h in zip(got, alone))


@pytest.mark.parametrize("how", (1, 2))
def test_channel_noise_special_rows(lib, how):
    ns = 480
    x = nc.noise_block(3, ns)
    x[0] = 0.0
    x[2, 17] = np.inf
    msq, sd, em, eq = noise(lib, x, 0, ns, nc.NOISE_Q, how)
    assert msq[0] == 0 and sd[0] == 0 and em[0] == 0 and np.all(eq[0] == 0)
    assert np.isnan(em[2]) and np.all(np.isnan(eq[2]))
    nc.check_noise([a[1:2] for a in (msq, sd, em, eq)], x[1:2], nc.NOISE_Q)


def test_fits_lds_is_stricter_than_the_transform(lib):
    fits = [ns for ns in range(2, 40000, 2) if lib.d4w_channel_noise_fits_lds(ns)]
    assert all(lib.d4w_analytic_row_fits_lds(ns) for ns in fits)
    assert any(lib.d4w_analytic_row_fits_lds(ns) and not lib.d4w_channel_noise_fits_lds(ns) for ns in range(2, 40000, 2))
    assert lib.d4w_channel_noise_fits_lds(12000) == 1 and lib.d4w_channel_noise_fits_lds(120000) == 0
    assert lib.d4w_channel_noise_fits_lds(1) == 0 and lib.d4w_channel_noise_fits_lds(0) == 0


# ------------------------------------------------------------------------------------------
# per-row thresholds
# ------------------------------------------------------------------------------------------
def test_find_peaks_rowthr_against_scipy(lib):
    nx, ns, cap = 7, 600, 301
    x = nc.peaks_block(nx, ns)
    for scale in (1.0, 0.5):
        thr = np.array(nc.PEAK_BARS, dtype=np.float32)
        idx = np.full((nx, cap), -1, dtype=np.int32)
        cnt = np.full(nx, -1, dtype=np.int32)
        rc = lib.d4w_find_peaks_rowthr_f32(vp(x), nx, ns, vp(thr), ctypes.c_double(scale), vp(idx), vp(cnt), cap, None)
        assert rc == 0, lib.d4w_last_error()
        ref = kn.find_peaks_rows(x, scale * thr.astype(np.float64))
        assert [len(r) for r in ref][2:5] == [0, 0, 0] and len(ref[0]) > 20 and 0 < len(ref[6]) < len(ref[5]) < len(ref[0])
        for c in range(nx):
            assert cnt[c] == len(ref[c]) and np.array_equal(idx[c, :cnt[c]], ref[c]), c
    # the scalar and the one-value forms are what they were: the same picks as a row bar of that value on every row
    thr = np.full(nx, 0.8, dtype=np.float32)
    idx2, cnt2 = np.full((nx, cap), -1, dtype=np.int32), np.full(nx, -1, dtype=np.int32)
    idx, cnt = np.full((nx, cap), -1, dtype=np.int32), np.full(nx, -1, dtype=np.int32)
    assert lib.d4w_find_peaks_rowthr_f32(vp(x), nx, ns, vp(thr), ctypes.c_double(1.0), vp(idx), vp(cnt), cap, None) == 0
    assert lib.d4w_find_peaks_f32(vp(x), nx, ns, ctypes.c_double(float(thr[0])), vp(idx2), vp(cnt2), cap, None) == 0
    assert np.array_equal(cnt, cnt2) and all(np.array_equal(idx[c, :cnt[c]], idx2[c, :cnt[c]]) for c in range(nx))


# ------------------------------------------------------------------------------------------
# bad arguments
# ------------------------------------------------------------------------------------------
def test_bad_arguments(lib):
    mq = max_q(lib)
    x = np.ones((3, 64), dtype=np.float32)
    out = np.zeros((3, mq + 1), dtype=np.float32)
    ws = np.empty(lib.d4w_channel_noise_ws_bytes(3, 64), dtype=np.uint8)

    def bad(rc, what):
        assert rc == -1, what
        assert len(lib.d4w_last_error()) > 0

    bad(lib.d4w_row_quantile_limits(None), "limits")

    def rq(v=x, nx=3, n=64, ld=64, q=(0.5,), nq=None, out=out):
        return lib.d4w_row_quantile_f32(vp(v) if v is not None else None, nx, SZ(n), SZ(ld), dbl(q) if q is not None else None,
                                        len(q) if nq is None else nq, vp(out) if out is not None else None, None)
    assert rq() == 0 and rq(q=[0.5] * mq) == 0 and rq(q=(0.0, 1.0)) == 0
    for kw in (dict(v=None), dict(out=None), dict(nx=0), dict(n=0), dict(ld=63), dict(q=(-0.01,)), dict(q=(1.0000001,)), dict(q=(float("nan"),)),
               dict(q=(0.5, 2.0)), dict(nq=0), dict(q=[0.5] * (mq + 1)), dict(nq=-1), dict(q=None, nq=1)):
        bad(rq(**kw), kw)

    def cn(v=x, nx=3, ns=64, ld=64, q=(0.5,), nq=None, outs=(out, out, out, out), ws=ws, how=0):
        p = [vp(o) if o is not None else None for o in outs]
        return lib.d4w_channel_noise_f32(vp(v) if v is not None else None, nx, ns, SZ(ld), dbl(q) if q is not None else None,
                                         len(q) if nq is None else nq, p[0], p[1], p[2], p[3], vp(ws) if ws is not None else None, how, None)
    assert cn() == 0 and cn(how=1, ws=None) == 0 and cn(how=2) == 0 and cn(q=(), outs=(out, out, out, None)) == 0
    assert cn(how=2, ws=None, outs=(out, out, None, None), q=()) == 0       # the moments alone need no workspace
    for kw in (dict(v=None), dict(nx=0), dict(ns=1), dict(ld=63), dict(q=(1.5,)), dict(q=(float("nan"),)), dict(q=[0.5] * (mq + 1)), dict(nq=-1),
               dict(q=None, nq=1), dict(how=3), dict(how=-1), dict(how=2, ws=None)):
        bad(cn(**kw), kw)
    long = np.ones((1, 40000), dtype=np.float32)
    assert lib.d4w_channel_noise_fits_lds(40000) == 0
    bad(cn(v=long, nx=1, ns=40000, ld=40000, how=1), "one-read form of a row that does not fit")

    idx, cnt, thr = np.zeros((3, 8), dtype=np.int32), np.zeros(3, dtype=np.int32), np.ones(3, dtype=np.float32)
    one = ctypes.c_double(1.0)
    assert lib.d4w_find_peaks_rowthr_f32(vp(x), 3, 64, vp(thr), one, vp(idx), vp(cnt), 8, None) == 0
    bad(lib.d4w_find_peaks_rowthr_f32(vp(x), 3, 64, None, one, vp(idx), vp(cnt), 8, None), "thr")
    bad(lib.d4w_find_peaks_rowthr_f32(None, 3, 64, vp(thr), one, vp(idx), vp(cnt), 8, None), "x")
    bad(lib.d4w_find_peaks_rowthr_f32(vp(x), 0, 64, vp(thr), one, vp(idx), vp(cnt), 8, None), "nx")
    bad(lib.d4w_find_peaks_rowthr_f32(vp(x), 3, 64, vp(thr), one, vp(idx), vp(cnt), 0, None), "cap")
