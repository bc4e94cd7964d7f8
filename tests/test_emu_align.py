"""Alignment against the beam (csrc/align.hip) in the CPU emulator build through the C ABI, against the float64 restatement of
tests/known_answers_align.py.  Kernel logic only, host pointers; the cases are those of tests/align_cases.py, which the
hardware runs as well (tests/test_align_gpu.py).

Tolerance, derived: |rho - rho_ref| <= (L + 8) 2^-24 (A / sqrt(tn en) + |rho_ref|) with A = sum |t| |x| (known_answers_align);
invalid lags NaN exactly, zero-energy entries 0 exactly; the lag, the coefficient and the arrival time exactly those the
pick rule gives on the returned table.  No case is skipped or excluded.
"""
import ctypes

import numpy as np
import pytest

from tests import align_cases as ac
from tests import beam_cases as bc
from tests import known_answers_align as ka
from tests import known_answers_beam as kb
from tests.emu_util import load_emu, vp
from tests.known_answers_loc import C0

D = ctypes.c_double
I64 = ctypes.c_int64
GUARD = 64


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def limits(lib):
    a, b, m, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.d4w_align_limits(ctypes.byref(a), ctypes.byref(b), ctypes.byref(m), ctypes.byref(w)) == 0
    return a.value, b.value, m.value, w.value


def p(a):
    return vp(a) if a is not None else None


def guarded(shape, dtype):
    """An output between two guards: (the whole buffer, the view the call writes)."""
    n = int(np.prod(shape))
    whole = np.full(n + 2 * GUARD, -7, dtype=dtype)
    return whole, whole[GUARD:GUARD + n].reshape(shape)


def emu_run(lib, return_all=True):
    def run(buf, ns, nxt, ns2, template, r, start, M, weights, fs, min_coef, subsample):
        buf = np.ascontiguousarray(buf, dtype=np.float32)
        nxt = np.ascontiguousarray(nxt, dtype=np.float32) if nxt is not None else None
        t = np.ascontiguousarray(template, dtype=np.float32)
        r = np.ascontiguousarray(r, dtype=np.int32)
        ncalls, nch = r.shape
        assert buf.shape[0] == nch and t.shape[0] == ncalls
        start = np.ascontiguousarray(start, dtype=np.int64)
        w = np.ascontiguousarray(weights, dtype=np.float32) if weights is not None else None
        outs = [guarded((ncalls, nch), np.float64), guarded((ncalls, nch), np.float32), guarded((ncalls, nch), np.int32),
                guarded((ncalls, nch, 2 * M + 1), np.float32)]
        Ti, coef, lag, rho = (o[1] for o in outs)
        rc = lib.d4w_align_f32(vp(buf), I64(buf.shape[1]), nch, ns, p(nxt), I64(nxt.shape[1] if nxt is not None else 0), ns2, vp(t), t.shape[1],
                               vp(r), vp(start), ncalls, M, p(w), D(fs), D(min_coef), int(subsample), vp(Ti), vp(coef),
                               vp(lag) if return_all else None, vp(rho) if return_all else None, None)
        assert rc == 0, lib.d4w_last_error()
        for whole, _ in outs:                                # the call wrote its outputs and nothing around them
            assert np.all(whole[:GUARD] == -7) and np.all(whole[len(whole) - GUARD:] == -7)
        if not return_all:
            assert np.all(lag == -7) and np.all(rho == -7)
        return Ti.copy(), coef.copy(), lag.copy(), rho.copy()
    return run


def test_limits(lib):
    max_calls, max_length, max_lag, W = limits(lib)
    assert max_calls >= 64 and max_length >= 4096 and max_lag >= 255 and W >= 2


def test_every_axis_value_occurs(lib):
    cases = ac.parity_cases()
    assert 30 <= len(cases) <= 40 and len(set(cases)) == len(cases)
    for axis, values in enumerate(ac.AXES):
        assert {c[axis] for c in cases} == set(values), (axis, values)
    W = limits(lib)[3]
    mixed = 0                                                # cases in which a live channel has valid and invalid lags side by side
    for case in cases:
        w, ref = ac.reference(case, W)[8:]
        live = np.ones(ref.valid.shape[1], dtype=bool) if w is None else w != 0
        mixed += bool(np.any(ref.valid[:, live].any(-1) & ~ref.valid[:, live].all(-1)))
    assert mixed >= 8, mixed


@pytest.mark.parametrize("case", ac.parity_cases(), ids=ac.case_id)
def test_parity(lib, case):
    ac.check_parity(emu_run(lib), case, limits(lib)[3])


def test_planted_template(lib):
    ac.check_planted(emu_run(lib), limits(lib)[3])


def test_bit_identity(lib):
    ac.check_bit_identity(emu_run(lib), limits(lib)[3])


def test_next_block_is_the_concatenation(lib):
    ac.check_next_block(emu_run(lib), limits(lib)[3])


def test_nan_sample(lib):
    ac.check_nan_sample(emu_run(lib), limits(lib)[3])


def test_zero_block_and_zero_template(lib):
    ac.check_zeros(emu_run(lib), limits(lib)[3])


def test_min_coef_and_subsample(lib):
    ac.check_min_coef_and_subsample(emu_run(lib), limits(lib)[3])


def test_without_the_optional_outputs(lib):
    """lag = rho = NULL: the same Ti and coef, and nothing else written."""
    case = ac.parity_cases()[0]
    buf, ns, nbuf, ns2, t, r, start, M, w, _ = ac.reference(case, limits(lib)[3])
    full = emu_run(lib)(buf, ns, nbuf, ns2, t, r, start, M, w, ac.FS, 0.0, True)
    bare = emu_run(lib, False)(buf, ns, nbuf, ns2, t, r, start, M, w, ac.FS, 0.0, True)
    assert ka.same(full[0], bare[0]) and ka.same(full[1], bare[1])


def test_the_limits_run(lib):
    """L = 4096 with M = 255 (the largest LDS image) on one channel more than a workgroup, windows across the seam."""
    _, max_length, max_lag, W = limits(lib)
    L, M, nch, ns = max_length, max_lag, W + 1, max_length + 500
    rng = np.random.default_rng(3)
    x, nb = rng.standard_normal((nch, ns)).astype(np.float32), rng.standard_normal((nch, 100)).astype(np.float32)
    t = rng.standard_normal((1, L)).astype(np.float32)
    r = (300 + 17 * np.arange(nch)[None, :]).astype(np.int32)
    start = np.zeros(1, dtype=np.int64)
    got = emu_run(lib)(x, ns, nb, 100, t, r, start, M, None, ac.FS, 0.0, True)
    ref = ka.align_ref(x, t, r, start, M, None, nb)
    assert ref.valid.any() and not ref.valid.all() and ka.worst_ratio(got[3], ref) <= 1.0
    ac.check_picks(got, ref.n0, M, ac.FS)


def test_extreme_starts_give_no_pick(lib):
    x, t = np.ones((3, 50), dtype=np.float32), np.ones((2, 8), dtype=np.float32)
    r = np.zeros((2, 3), dtype=np.int32)
    for s in (np.iinfo(np.int64).min, np.iinfo(np.int64).max, -(1 << 40), 1 << 40):
        Ti, coef, lag, rho = emu_run(lib)(x, 50, None, 0, t, r, np.array([s, 0], dtype=np.int64), 2, None, 50.0, 0.0, True)
        assert np.all(np.isnan(Ti[0])) and np.all(np.isnan(coef[0])) and not lag[0].any() and np.all(np.isnan(rho[0]))
        assert np.array_equal(lag[1], [0, 0, 0]) and np.array_equal(Ti[1], [0.0, 0.0, 0.0]) and np.all(np.abs(coef[1] - 1) <= 1e-6)


def test_table_of_beam_delays(lib):
    """The table d4w_beam_delays builds for a geometry is the one the restatement rounds: aligned with it, a burst planted at
    the rounded moveout is found at lag 0 on every channel."""
    nch, L, M, fs = 9, 64, 3, 200.0
    cable = np.ascontiguousarray(bc.make_cable("bent", nch))
    pos = bc.positions(cable, fs, 2, 1)
    r = np.full((2, nch), -7, dtype=np.int32)
    assert lib.d4w_beam_delays(vp(cable), nch, D(C0), D(fs), vp(np.ascontiguousarray(pos)), 2, None, None, vp(r), None) == 0, lib.d4w_last_error()
    assert np.array_equal(r, kb.rounded(kb.tau(cable, C0, fs, pos)))
    rng = np.random.default_rng(1)
    t = rng.standard_normal((2, L)).astype(np.float32)
    start = (10 - r.min(1)).astype(np.int64)
    ns = int((start[:, None] + r).max()) + L + M + 1
    x = np.zeros((nch, ns), dtype=np.float32)
    for ch in range(nch):
        x[ch, start[0] + r[0, ch]:start[0] + r[0, ch] + L] = t[0]
    Ti, coef, lag, _ = emu_run(lib)(x, ns, None, 0, t, r, start, M, None, fs, 0.9, False)
    assert not lag[0].any() and np.all(coef[0] > 0.99) and np.array_equal(Ti[0], (start[0] + r[0]) / fs)


# ------------------------------------------------------------------------------------------
# bad arguments
# ------------------------------------------------------------------------------------------
def test_bad_arguments(lib):
    max_calls, max_length, max_lag, _ = limits(lib)
    nch, ns, L, M = 5, 64, 8, 2
    x, nb = np.ones((nch, ns), dtype=np.float32), np.ones((nch, 7), dtype=np.float32)
    t, r = np.ones((1, L), dtype=np.float32), np.zeros((1, nch), dtype=np.int32)
    start = np.zeros(1, dtype=np.int64)
    Ti, coef = np.zeros((1, nch)), np.zeros((1, nch), dtype=np.float32)
    lag, rho = np.zeros((1, nch), dtype=np.int32), np.zeros((1, nch, 2 * max_lag + 3), dtype=np.float32)
    nan, inf = float("nan"), float("inf")
    i = ctypes.c_int()

    def bad(rc, what):
        assert rc == -1, what
        assert len(lib.d4w_last_error()) > 0

    for k in range(4):
        args = [ctypes.byref(i)] * 4
        args[k] = None
        bad(lib.d4w_align_limits(*args), "limits %d" % k)

    def align(x=x, pitch=ns, nch=nch, ns=ns, xn=None, pitchn=0, nsn=0, t=t, L=L, r=r, st=start, ncalls=1, M=M, fs=50.0, mc=0.0, Ti=Ti, coef=coef,
              lag=lag, rho=rho):
        return lib.d4w_align_f32(p(x), I64(pitch), nch, ns, p(xn), I64(pitchn), nsn, p(t), L, p(r), p(st), ncalls, M, None, D(fs), D(mc), 1, p(Ti),
                                 p(coef), p(lag), p(rho), None)
    assert align() == 0 and align(lag=None, rho=None) == 0 and align(xn=nb, pitchn=7, nsn=7) == 0 and align(M=0) == 0 and align(mc=-2.0) == 0
    for kw in (dict(x=None), dict(t=None), dict(r=None), dict(st=None), dict(Ti=None), dict(coef=None), dict(nch=0), dict(ns=0), dict(pitch=ns - 1),
               dict(ncalls=0), dict(ncalls=-1), dict(ncalls=max_calls + 1), dict(L=0), dict(L=-4), dict(L=max_length + 1), dict(M=-1), dict(M=max_lag + 1),
               dict(fs=0.0), dict(fs=-1.0), dict(fs=nan), dict(fs=inf), dict(mc=nan), dict(mc=inf), dict(mc=-inf),
               dict(xn=nb, pitchn=7, nsn=0), dict(xn=nb, pitchn=6, nsn=7), dict(xn=None, nsn=7)):
        bad(align(**kw), kw)
