"""Received levels (csrc/levels.hip) in the CPU emulator build through the C ABI, against the float64 restatement of
tests/known_answers_levels.py.  Kernel logic only, host pointers; the cases are those of tests/levels_cases.py, which the
hardware runs as well (tests/test_levels_gpu.py).

Tolerance, derived: |signal - ref| <= (L + 8) 2^-24 ref and |noise - ref| <= (N + 8) 2^-24 ref (non-negative terms, one
rounding per step, one for the division); peak exactly; NaN exactly where the definition says; entries whose reference is 0
exactly 0.  No case is skipped or excluded.
"""
import ctypes

import numpy as np
import pytest

from tests import known_answers_levels as kl
from tests import levels_cases as lc
from tests.emu_util import load_emu, vp

I64 = ctypes.c_int64
GUARD = 64


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def limits(lib):
    a, b, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.d4w_level_limits(ctypes.byref(a), ctypes.byref(b), ctypes.byref(w)) == 0
    return a.value, b.value, w.value


def p(a):
    return vp(a) if a is not None else None


def guarded(shape):
    """An output between two guards: (the whole buffer, the view the call writes)."""
    n = int(np.prod(shape))
    whole = np.full(n + 2 * GUARD, -7, dtype=np.float32)
    return whole, whole[GUARD:GUARD + n].reshape(shape)


def emu_run(lib, noise_buffer=False):
    """The runner of levels_cases on the C ABI.  With N = 0 the noise pointer is NULL (and the result reported as the NaN the
    definition gives), unless noise_buffer asks for a buffer to be handed over all the same."""
    def run(buf, ns, nxt, ns2, r, start, L, gap, N, weights):
        buf = np.ascontiguousarray(buf, dtype=np.float32)
        nxt = np.ascontiguousarray(nxt, dtype=np.float32) if nxt is not None else None
        r = np.ascontiguousarray(r, dtype=np.int32)
        ncalls, nch = r.shape
        assert buf.shape[0] == nch
        start = np.ascontiguousarray(start, dtype=np.int64)
        w = np.ascontiguousarray(weights, dtype=np.float32) if weights is not None else None
        outs = [guarded((ncalls, nch)) for _ in range(3)]
        signal, noise, peak = (o[1] for o in outs)
        given = N > 0 or noise_buffer
        rc = lib.d4w_level_f32(vp(buf), I64(buf.shape[1]), nch, ns, p(nxt), I64(nxt.shape[1] if nxt is not None else 0), ns2, vp(r), vp(start),
                               ncalls, L, gap, N, p(w), vp(signal), vp(noise) if given else None, vp(peak), None)
        assert rc == 0, lib.d4w_last_error()
        for whole, _ in outs:                                # the call wrote its outputs and nothing around them
            assert np.all(whole[:GUARD] == -7) and np.all(whole[len(whole) - GUARD:] == -7)
        if not given:
            assert np.all(noise == -7)
            noise = np.full((ncalls, nch), np.nan, dtype=np.float32)
        return signal.copy(), noise.copy(), peak.copy()
    return run


def test_limits(lib):
    max_calls, max_length, W = limits(lib)
    assert max_calls >= 64 and max_length >= 1 << 20 and W >= 2


def test_every_axis_value_occurs(lib):
    cases = lc.parity_cases()
    assert 30 <= len(cases) <= 40 and len(set(cases)) == len(cases)
    for axis, values in enumerate(lc.AXES):
        assert {c[axis] for c in cases} == set(values), (axis, values)
        for v in values:
            assert sum(c[axis] == v for c in cases) >= 2, (axis, v)
    W = limits(lib)[2]
    mixed = sum(lc.mixed(case, W) for case in cases)         # a live channel with one window valid and the other not
    assert mixed >= 8, mixed


@pytest.mark.parametrize("case", lc.parity_cases(), ids=lc.case_id)
def test_parity(lib, case):
    lc.check_parity(emu_run(lib), case, limits(lib)[2])


@pytest.mark.parametrize("case", lc.parity_cases()[::3], ids=lc.case_id)
def test_poison(lib, case):
    lc.check_poison(emu_run(lib), case, limits(lib)[2])


def test_poison_reaches_live_windows(lib):
    """The poisoned cases do own samples: the test above is not vacuous."""
    assert sum(lc.check_poison(emu_run(lib), case, limits(lib)[2]) > 0 for case in lc.parity_cases()[::3]) >= 6


def test_integer_samples(lib):
    lc.check_integers(emu_run(lib), limits(lib)[2])


def test_zero_block_and_ones(lib):
    lc.check_zeros_and_ones(emu_run(lib), limits(lib)[2])


def test_nan_rows_and_samples(lib):
    lc.check_nan_rows(emu_run(lib), limits(lib)[2])


def test_bit_identity(lib):
    lc.check_bit_identity(emu_run(lib), limits(lib)[2])


def test_split_is_the_concatenation(lib):
    lc.check_split(emu_run(lib), limits(lib)[2])


def test_noise_buffer_without_a_noise_window(lib):
    """N = 0 with a noise buffer given: noise is all NaN, signal and peak as with the NULL pointer."""
    W = limits(lib)[2]
    seen = 0
    for case in lc.parity_cases():
        if case[1] != 0:
            continue
        buf, ns, nbuf, ns2, r, start, L, gap, N, w, _ = lc.reference(case, W)
        bare = emu_run(lib)(buf, ns, nbuf, ns2, r, start, L, gap, N, w)
        full = emu_run(lib, True)(buf, ns, nbuf, ns2, r, start, L, gap, N, w)
        assert np.all(np.isnan(full[1])) and kl.same(bare[0], full[0]) and kl.same(bare[2], full[2])
        seen += 1
    assert seen >= 3


def test_extreme_starts_give_nan(lib):
    x = np.ones((3, 50), dtype=np.float32)
    r = np.zeros((2, 3), dtype=np.int32)
    for s in (np.iinfo(np.int64).min, np.iinfo(np.int64).max, -(1 << 40), 1 << 40):
        got = emu_run(lib)(x, 50, None, 0, r, np.array([s, 10], dtype=np.int64), 8, 1, 4, None)
        assert all(np.all(np.isnan(a[0])) and np.all(a[1] == 1.0) for a in got)


def test_no_call_launches_nothing(lib):
    x = np.ones((3, 50), dtype=np.float32)
    assert lib.d4w_level_f32(vp(x), I64(50), 3, 50, None, I64(0), 0, None, None, 0, 8, 0, 0, None, None, None, None, None) == 0


# ------------------------------------------------------------------------------------------
# bad arguments
# ------------------------------------------------------------------------------------------
def test_bad_arguments(lib):
    max_calls, max_length, _ = limits(lib)
    nch, ns = 5, 64
    x, nb = np.ones((nch, ns), dtype=np.float32), np.ones((nch, 7), dtype=np.float32)
    r, start = np.zeros((1, nch), dtype=np.int32), np.zeros(1, dtype=np.int64)
    sig, noi, pk = (np.zeros((1, nch), dtype=np.float32) for _ in range(3))
    i = ctypes.c_int()

    def bad(rc, what):
        assert rc == -1, what
        assert len(lib.d4w_last_error()) > 0

    for k in range(3):
        args = [ctypes.byref(i)] * 3
        args[k] = None
        bad(lib.d4w_level_limits(*args), "limits %d" % k)

    def level(x=x, pitch=ns, nch=nch, ns=ns, xn=None, pitchn=0, nsn=0, r=r, st=start, ncalls=1, L=8, gap=1, N=4, sig=sig, noi=noi, pk=pk):
        return lib.d4w_level_f32(p(x), I64(pitch), nch, ns, p(xn), I64(pitchn), nsn, p(r), p(st), ncalls, L, gap, N, None, p(sig), p(noi), p(pk),
                                 None)
    assert level() == 0 and level(N=0, noi=None) == 0 and level(N=0) == 0 and level(xn=nb, pitchn=7, nsn=7) == 0 and level(gap=0) == 0
    for kw in (dict(x=None), dict(r=None), dict(st=None), dict(sig=None), dict(pk=None), dict(noi=None), dict(nch=0), dict(ns=0), dict(pitch=ns - 1),
               dict(ncalls=-1), dict(ncalls=max_calls + 1), dict(L=0), dict(L=-4), dict(L=max_length + 1), dict(N=-1), dict(N=max_length + 1), dict(gap=-1), dict(gap=max_length, N=1),
               dict(xn=nb, pitchn=7, nsn=0), dict(xn=nb, pitchn=6, nsn=7), dict(xn=None, nsn=7)):
        bad(level(**kw), kw)
