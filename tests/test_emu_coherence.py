"""Coherence of located calls (csrc/coherence.hip) in the CPU emulator build through the C ABI, against the float64
restatement of tests/known_answers_coherence.py.  Kernel logic only, host pointers; the cases are those of
tests/coherence_cases.py, which the hardware runs as well (tests/test_coherence_gpu.py).

Tolerances: derived in known_answers_coherence; the semblance bound is <= 1e-4 on every compared element (asserted by the
case file), no case or element is skipped or excluded.
"""
import ctypes

import numpy as np
import pytest

from tests import coherence_cases as cc
from tests.emu_util import load_emu, vp

I64 = ctypes.c_int64
GUARD = 64


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def limits(lib):
    a, b, h, s = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.d4w_coherence_limits(ctypes.byref(a), ctypes.byref(b), ctypes.byref(h), ctypes.byref(s)) == 0
    return a.value, b.value, h.value, s.value


def ws_bytes(lib, nch, ncalls, nt, phase):
    n = ctypes.c_size_t(12345)
    assert lib.d4w_coherence_ws_bytes(nch, ncalls, nt, int(phase), ctypes.byref(n)) == 0, lib.d4w_last_error()
    return n.value


def p(a):
    return vp(a) if a is not None else None


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32) if a is not None else None


def pitch(a):
    return I64(a.shape[1] if a is not None else 0)


def emu_run(lib, want_wsum=True):
    def run(buf, ns, nxt, ns2, ibuf, inxt, delays, order, weights, start, nt, H, peak_range=None):
        buf, nxt, ibuf, inxt, w = f32(buf), f32(nxt), f32(ibuf), f32(inxt), f32(weights)
        kr, f = (delays, None) if order == 0 else delays
        kr, f = np.ascontiguousarray(kr, dtype=np.int32), f32(f)
        ncalls, nch = kr.shape
        assert buf.shape[0] == nch
        start = np.ascontiguousarray(start, dtype=np.int64)
        nbytes = ws_bytes(lib, nch, ncalls, nt, ibuf is not None)
        # the workspace between two guards: the call may write its nbytes and nothing else
        ws = np.full(nbytes // 4 + 2 * GUARD, -7.0, dtype=np.float32)
        beam, semb, phase, wsum = (np.full((ncalls, nt), -7.0, dtype=np.float32) for _ in range(4))
        rc = lib.d4w_coherence_f32(vp(buf), pitch(buf), nch, ns, p(nxt), pitch(nxt), ns2, p(ibuf), pitch(ibuf), p(inxt), pitch(inxt), vp(kr), p(f),
                                   p(w), vp(start), ncalls, nt, order, H, vp(beam), vp(semb), vp(phase) if ibuf is not None else None,
                                   vp(wsum) if want_wsum else None, ctypes.c_void_p(ws.ctypes.data + 4 * GUARD), None)
        assert rc == 0, lib.d4w_last_error()
        assert np.all(ws[:GUARD] == -7.0) and np.all(ws[len(ws) - GUARD:] == -7.0)
        if ibuf is None:
            assert np.all(phase == -7.0)                     # a NULL output is not written (nor is anything in its place)
        if not want_wsum:
            assert np.all(wsum == -7.0)
        lo, hi = peak_range if peak_range is not None else (0, nt)
        peak, index = np.full(ncalls, -7.0, dtype=np.float32), np.full(ncalls, -7, dtype=np.int32)
        assert lib.d4w_coherence_peak_f32(vp(semb), ncalls, nt, lo, hi, vp(peak), vp(index), None) == 0, lib.d4w_last_error()
        return dict(beam=beam, semblance=semb, phase=phase if ibuf is not None else None, wsum=wsum, peak=peak, peak_index=index)
    return run


def emu_beam(lib):
    def run(buf, ns, nxt, ns2, delays, order, weights, start, nt, normalize):
        buf, nxt, w = f32(buf), f32(nxt), f32(weights)
        kr, f = (delays, None) if order == 0 else delays
        kr, f = np.ascontiguousarray(kr, dtype=np.int32), f32(f)
        ncalls, nch = kr.shape
        n = ctypes.c_size_t()
        assert lib.d4w_beam_ws_bytes(nch, ncalls, nt, ctypes.byref(n)) == 0
        ws = np.zeros(max(n.value // 4, 1), dtype=np.float32)
        out = np.full((ncalls, nt), -7.0, dtype=np.float32)
        rc = lib.d4w_beamform_f32(vp(buf), pitch(buf), nch, ns, p(nxt), pitch(nxt), ns2, vp(kr), p(f), p(w),
                                  vp(np.ascontiguousarray(start, dtype=np.int64)), ncalls, nt, order, int(normalize), vp(out), vp(ws), None)
        assert rc == 0, lib.d4w_last_error()
        return out
    return run


def test_limits_and_workspace(lib):
    max_calls, max_length, Hmax, S = limits(lib)
    b, bl, bs = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.d4w_beam_limits(ctypes.byref(b), ctypes.byref(bl), ctypes.byref(bs)) == 0
    assert (max_calls, max_length, S) == (b.value, bl.value, bs.value)         # calls and length as for the beam, its segment
    assert Hmax >= 256
    assert ws_bytes(lib, S, 3, 100, False) == 3 * 3 * 100 * 4 and ws_bytes(lib, S + 1, 3, 100, True) == 5 * 2 * 3 * 100 * 4
    assert ws_bytes(lib, 11020, 64, 12000, True) < 2 ** 31


def test_every_axis_value_occurs():
    assert len(set(cc.CASES)) == len(cc.CASES)
    for axis, values in enumerate(cc.AXES):
        if values is not None:
            assert {c[axis] for c in cc.CASES} == set(values), (axis, values)
    assert all(1500 <= c[2] <= 3000 for c in cc.CASES)


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_parity(lib, case):
    cc.check_parity(emu_run(lib), emu_beam(lib), case, limits(lib)[2])


def test_exact_one(lib):
    cc.check_exact_one(emu_run(lib))


def test_exact_zero(lib):
    cc.check_exact_zero(emu_run(lib))


def test_phase_one(lib):
    cc.check_phase_one(emu_run(lib), limits(lib)[3])


def test_bit_identity(lib):
    cc.check_bit_identity(emu_run(lib), limits(lib)[2])


def test_next_block_is_the_concatenation(lib):
    cc.check_next_block(emu_run(lib), limits(lib)[2])


def test_peak_range(lib):
    cc.check_peak_range(emu_run(lib))


def test_null_wsum_is_not_written(lib):
    cc.check_exact_one(lambda *a, **k: dict(emu_run(lib, want_wsum=False)(*a, **k), wsum=np.full((1, a[10]), 128.0, dtype=np.float32)))


def test_extreme_starts_add_nothing(lib):
    x = np.ones((3, 50), dtype=np.float32)
    r = np.zeros((2, 3), dtype=np.int32)
    for s in (np.iinfo(np.int64).min, np.iinfo(np.int64).max, -(1 << 40), 1 << 40):
        got = emu_run(lib)(x, 50, None, 0, x, None, r, 0, None, np.array([s, 0], dtype=np.int64), 60, 2)
        for name in ("beam", "semblance", "phase", "wsum"):
            assert not got[name][0].any(), name
        assert np.all(got["semblance"][1, :52] == 1.0) and not got["semblance"][1, 52:].any()
        assert np.all(got["wsum"][1, :50] == 3.0) and not got["wsum"][1, 50:].any()


# ------------------------------------------------------------------------------------------
# bad arguments
# ------------------------------------------------------------------------------------------
def test_bad_arguments(lib):
    max_calls, max_length, Hmax, S = limits(lib)
    nch, ns, nt = 5, 64, 32
    k, f = np.zeros((1, nch), dtype=np.int32), np.zeros((1, nch), dtype=np.float32)
    x, nb = np.ones((nch, ns), dtype=np.float32), np.ones((nch, 7), dtype=np.float32)
    start = np.zeros(1, dtype=np.int64)
    beam, semb, phase, wsum = (np.zeros((1, nt), dtype=np.float32) for _ in range(4))
    ws = np.zeros(5 * nt, dtype=np.float32)
    ones = np.ones(nch, dtype=np.float32)
    nan, inf = float("nan"), float("inf")
    i, n = ctypes.c_int(), ctypes.c_size_t()

    def bad(rc, what):
        assert rc == -1, what
        assert len(lib.d4w_last_error()) > 0

    for hole in range(4):
        args = [ctypes.byref(i)] * 4
        args[hole] = None
        bad(lib.d4w_coherence_limits(*args), "limits")

    def wsb(nch=nch, ncalls=1, nt=nt, o=n):
        return lib.d4w_coherence_ws_bytes(nch, ncalls, nt, 1, ctypes.byref(o) if o is not None else None)
    assert wsb() == 0
    for kw in (dict(o=None), dict(nch=0), dict(ncalls=0), dict(ncalls=max_calls + 1), dict(nt=0), dict(nt=-1)):
        bad(wsb(**kw), kw)
    if max_length < 2 ** 31 - 1:
        bad(wsb(nt=max_length + 1), "length")

    def coh(x=x, pitch=ns, nch=nch, ns=ns, xn=None, pitchn=0, nsn=0, xi=None, pitchi=ns, xin=None, pitchin=0, kr=k, f=f, w=None, st=start, ncalls=1,
            nt=nt, order=1, H=2, b=beam, s=semb, ph=None, ws=ws):
        return lib.d4w_coherence_f32(p(x), I64(pitch), nch, ns, p(xn), I64(pitchn), nsn, p(xi), I64(pitchi), p(xin), I64(pitchin), p(kr), p(f), p(w),
                                     p(st), ncalls, nt, order, H, p(b), p(s), p(ph), vp(wsum), p(ws), None)
    assert coh() == 0 and coh(order=0, f=None) == 0 and coh(xn=nb, pitchn=7, nsn=7) == 0 and coh(w=ones) == 0 and coh(H=Hmax) == 0 and coh(H=0) == 0
    assert coh(xi=x, ph=phase) == 0 and coh(xn=nb, pitchn=7, nsn=7, xi=x, xin=nb, pitchin=7, ph=phase) == 0
    for kw in (dict(x=None), dict(kr=None), dict(st=None), dict(b=None), dict(s=None), dict(ws=None), dict(f=None), dict(order=3, f=None),
               dict(order=2), dict(order=-1), dict(order=4), dict(H=-1), dict(H=Hmax + 1),
               dict(nch=0), dict(ns=0), dict(pitch=ns - 1), dict(ncalls=0), dict(ncalls=max_calls + 1), dict(nt=0), dict(nt=-5),
               dict(xn=nb, pitchn=7, nsn=0), dict(xn=nb, pitchn=6, nsn=7), dict(xn=None, nsn=7),
               dict(xi=x), dict(ph=phase), dict(xi=x, ph=phase, pitchi=ns - 1),
               dict(xi=x, ph=phase, xin=nb, pitchin=7),                                            # a next imaginary block without a next block
               dict(xn=nb, pitchn=7, nsn=7, xi=x, ph=phase),                                       # a next block without its imaginary block
               dict(xn=nb, pitchn=7, nsn=7, xi=x, ph=phase, xin=nb, pitchin=6),
               dict(xn=nb, pitchn=7, nsn=7, xin=nb, pitchin=7),                                    # a next imaginary block without an imaginary block
               dict(w=ones * -1), dict(w=ones * nan), dict(w=ones * inf),
               dict(w=np.array([1, 1, 1, 1, -0.5], dtype=np.float32))):
        before = [a.copy() for a in (beam, semb, phase, wsum, ws)]
        bad(coh(**kw), kw)
        assert all(np.array_equal(a, b) for a, b in zip(before, (beam, semb, phase, wsum, ws))), kw      # refused before any launch

    pk, ix = np.zeros(1, dtype=np.float32), np.zeros(1, dtype=np.int32)

    def peak(s=semb, ncalls=1, nt=nt, lo=0, hi=nt, pk=pk, ix=ix):
        return lib.d4w_coherence_peak_f32(p(s), ncalls, nt, lo, hi, p(pk), p(ix), None)
    assert peak() == 0 and peak(lo=nt - 1) == 0
    for kw in (dict(s=None), dict(pk=None), dict(ix=None), dict(ncalls=0), dict(ncalls=max_calls + 1), dict(nt=0), dict(lo=-1), dict(lo=5, hi=5),
               dict(lo=6, hi=5), dict(hi=nt + 1)):
        bad(peak(**kw), kw)


def test_peak_of_nan_rows(lib):
    s = np.full((2, 40), np.nan, dtype=np.float32)
    s[1, 7], s[1, 30] = 0.25, 0.25
    pk, ix = np.zeros(2, dtype=np.float32), np.zeros(2, dtype=np.int32)
    assert lib.d4w_coherence_peak_f32(vp(s), 2, 40, 0, 40, vp(pk), vp(ix), None) == 0
    assert np.isnan(pk[0]) and ix[0] == -1 and pk[1] == np.float32(0.25) and ix[1] == 7
