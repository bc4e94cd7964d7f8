"""The transpose of the beam (csrc/project.hip) in the CPU emulator build through the C ABI, against the float64 restatement of
tests/known_answers_project.py.  Kernel logic only, host pointers; the cases are those of tests/project_cases.py, which the
hardware runs as well (tests/test_project_gpu.py).

Tolerances, derived in known_answers_project: num, den, xx within (W + 16 / 28 / 4) 2^-24 sum |terms|, amp and coef propagated
from them, y within one rounding per subtracted call plus the error of amp g; NaN exactly where the definition says; entries
whose den is 0 exactly 0; samples no call reaches bit for bit.  Every output lies between guard words, and the padding of a
pitched output keeps its fill.  No case is skipped or excluded.
"""
import ctypes

import numpy as np
import pytest

from tests import known_answers_project as kp
from tests import project_cases as pc
from tests.emu_util import load_emu, vp

I64 = ctypes.c_int64
GUARD = 64
FILL = -7.25                                                 # no sample of a case has this value


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def limits(lib):
    a, b, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.d4w_project_limits(ctypes.byref(a), ctypes.byref(b), ctypes.byref(w)) == 0
    return a.value, b.value, w.value


def p(a):
    return vp(a) if a is not None else None


def guarded(shape, fill=FILL):
    """An output between two guards: (the whole buffer, the view the call writes)."""
    n = int(np.prod(shape))
    whole = np.full(n + 2 * GUARD, fill, dtype=np.float32)
    return whole, whole[GUARD:GUARD + n].reshape(shape)


def guards_intact(whole):
    return bool(np.all(whole[:GUARD] == FILL) and np.all(whole[len(whole) - GUARD:] == FILL))


def tables(delays, order):
    if order == 0:
        return np.ascontiguousarray(delays, dtype=np.int32), None
    return np.ascontiguousarray(delays[0], dtype=np.int32), np.ascontiguousarray(delays[1], dtype=np.float32)


class EmuRun:
    """The runner of project_cases on the C ABI."""

    def __init__(self, lib):
        self.lib = lib

    def fit(self, buf, ns, nxt, ns2, delays, order, beam, start, weights):
        lib = self.lib
        buf = np.ascontiguousarray(buf, dtype=np.float32)
        nxt = np.ascontiguousarray(nxt, dtype=np.float32) if nxt is not None else None
        kr, f = tables(delays, order)
        ncalls, nch = kr.shape
        beam = np.ascontiguousarray(beam, dtype=np.float32).reshape(ncalls, -1)
        start = np.ascontiguousarray(start, dtype=np.int64)
        w = np.ascontiguousarray(weights, dtype=np.float32) if weights is not None else None
        (wa, amp), (wc, coef) = guarded((ncalls, nch)), guarded((ncalls, nch))
        rc = lib.d4w_project_f32(vp(buf), I64(buf.shape[1]), nch, ns, p(nxt), I64(nxt.shape[1] if nxt is not None else 0), ns2, vp(kr), p(f),
                                 vp(beam), beam.shape[1], vp(start), ncalls, order, p(w), vp(amp), vp(coef), None)
        assert rc == 0, lib.d4w_last_error()
        assert guards_intact(wa) and guards_intact(wc)
        return amp.copy(), coef.copy()

    def sub(self, buf, ns, nxt, ns2, delays, order, beam, start, amp, inplace):
        lib = self.lib
        kr, f = tables(delays, order)
        ncalls, nch = kr.shape
        beam = np.ascontiguousarray(beam, dtype=np.float32).reshape(ncalls, -1)
        start = np.ascontiguousarray(start, dtype=np.int64)
        amp = np.ascontiguousarray(amp, dtype=np.float32)
        buf = np.ascontiguousarray(buf, dtype=np.float32)
        nxt = np.ascontiguousarray(nxt, dtype=np.float32) if nxt is not None else None
        wy, y = guarded(buf.shape)
        wn, yn = guarded(nxt.shape) if nxt is not None else (None, None)
        if inplace:                                          # on a copy of the buffers, padding and all
            y[...] = buf
            src, srcn = y, yn
            if nxt is not None:
                yn[...] = nxt
        else:
            src, srcn = buf, nxt
        rc = lib.d4w_project_subtract_f32(vp(src), I64(buf.shape[1]), nch, ns, p(srcn), I64(nxt.shape[1] if nxt is not None else 0), ns2, vp(kr), p(f),
                                          vp(beam), beam.shape[1], vp(start), vp(amp), ncalls, order, vp(y), I64(buf.shape[1]), p(yn),
                                          I64(nxt.shape[1] if nxt is not None else 0), None)
        assert rc == 0, lib.d4w_last_error()
        assert guards_intact(wy) and (wn is None or guards_intact(wn))
        # the padding beyond the row: out of place it keeps the fill, in place what the buffer held
        for out, given, n in ((y, buf, ns), (yn, nxt, ns2)):
            if out is not None:
                assert kp.same(out[:, n:], given[:, n:] if inplace else np.full_like(out[:, n:], FILL))
                if not inplace:
                    assert not np.any(out[:, :n] == FILL)    # every sample was written
        return y[:, :ns].copy() if nxt is None else np.concatenate([y[:, :ns], yn[:, :ns2]], axis=1)

    def beam(self, buf, ns, nxt, ns2, delays, order, start, nt):
        lib = self.lib
        buf = np.ascontiguousarray(buf, dtype=np.float32)
        nxt = np.ascontiguousarray(nxt, dtype=np.float32) if nxt is not None else None
        kr, f = tables(delays, order)
        ncalls, nch = kr.shape
        start = np.ascontiguousarray(start, dtype=np.int64)
        nbytes = ctypes.c_size_t()
        assert lib.d4w_beam_ws_bytes(nch, ncalls, nt, ctypes.byref(nbytes)) == 0
        ws = np.zeros(max(nbytes.value, 4) // 4, dtype=np.float32)
        out = np.zeros((ncalls, nt), dtype=np.float32)
        rc = lib.d4w_beamform_f32(vp(buf), I64(buf.shape[1]), nch, ns, p(nxt), I64(nxt.shape[1] if nxt is not None else 0), ns2, vp(kr), p(f), None,
                                  vp(start), ncalls, nt, order, 0, vp(out), vp(ws), None)
        assert rc == 0, lib.d4w_last_error()
        return out


@pytest.fixture(scope="module")
def run(lib):
    return EmuRun(lib)


@pytest.fixture(scope="module")
def W(lib):
    return limits(lib)[2]


def test_limits(lib):
    max_calls, max_length, W = limits(lib)
    assert max_calls >= 64 and max_length >= 1 << 20 and W >= 2


def test_every_axis_value_occurs(W):
    cases = pc.parity_cases()
    assert 30 <= len(cases) <= 40 and len(set(cases)) == len(cases)
    for axis, values in enumerate(pc.AXES):
        assert {c[axis] for c in cases} == set(values), (axis, values)
        for v in values:
            assert sum(c[axis] == v for c in cases) >= 2, (axis, v)
    refs = [pc.reference(case, W) for case in cases]
    assert sum(0 < k.fit.valid.sum() < k.fit.valid.size for k in refs) >= 8          # some windows valid and others not
    assert sum(bool(k.reached.any()) for k in refs) >= 20
    # supports of several calls overlap on a channel, and supports cross the seam
    assert sum(k.fit.valid.shape[0] == 3 and bool((k.fit.valid.sum(0) >= 2).any()) for k in refs) >= 8
    assert sum(bool(np.any(k.fit.valid & (k.fit.lo < k.ns) & (k.fit.lo + k.fit.W > k.ns))) for k in refs) >= 3


@pytest.mark.parametrize("case", pc.parity_cases(), ids=pc.case_id)
def test_parity(run, W, case):
    pc.check_parity(run, case, W)


@pytest.mark.parametrize("case", pc.parity_cases()[::3], ids=pc.case_id)
def test_poison(run, W, case):
    pc.check_poison(run, case, W)


def test_poison_reaches_live_windows(run, W):
    """The poisoned cases do own samples: the test above is not vacuous."""
    assert sum(pc.check_poison(run, case, W) > 0 for case in pc.parity_cases()[::3]) >= 6


def test_identical_channels(run, W):
    pc.check_identical_channels(run, W)


def test_power_of_two_scaling(run, W):
    pc.check_power_of_two(run, W)


def test_zero_beam(run, W):
    pc.check_zero_beam(run, W)


def test_nan_samples_rows_and_amplitudes(run, W):
    pc.check_nan_samples(run, W)


def test_batch_and_split_independence(run, W):
    pc.check_batch_and_split(run, W)


def test_call_order(run, W):
    pc.check_call_order(run, W)


def test_transpose_of_the_beam(run, W):
    pc.check_transpose(run, W)


def test_more_than_one_tile_and_lds_piece(run, W):
    pc.check_tiles(run, W)


def test_extreme_starts_give_nan_and_subtract_nothing(run):
    x = np.ones((3, 50), dtype=np.float32)
    r = np.zeros((2, 3), dtype=np.int32)
    beam = np.ones((2, 8), dtype=np.float32)
    for s in (np.iinfo(np.int64).min, np.iinfo(np.int64).max, -(1 << 40), 1 << 40):
        start = np.array([s, 10], dtype=np.int64)
        amp, coef = run.fit(x, 50, None, 0, r, 0, beam, start, None)
        assert np.all(np.isnan(amp[0])) and np.all(np.isnan(coef[0])) and np.all(amp[1] == 1.0) and np.all(coef[1] == 1.0)
        y = run.sub(x, 50, None, 0, r, 0, beam, start, np.ones((2, 3), dtype=np.float32), False)
        assert np.all(y[:, 10:18] == 0.0) and np.all(y[:, :10] == 1.0) and np.all(y[:, 18:] == 1.0)


def test_no_call(lib):
    """ncalls = 0: the fit and the subtraction in place launch nothing (NULL pointers are fine); out of place it is the copy."""
    x = np.arange(150, dtype=np.float32).reshape(3, 50)
    assert lib.d4w_project_f32(vp(x), I64(50), 3, 50, None, I64(0), 0, None, None, None, 8, None, 0, 1, None, None, None, None) == 0
    keep = x.copy()
    assert lib.d4w_project_subtract_f32(vp(x), I64(50), 3, 50, None, I64(0), 0, None, None, None, 8, None, None, 0, 1, vp(x), I64(50), None, I64(0),
                                        None) == 0
    assert np.array_equal(x, keep)
    y = np.zeros_like(x)
    assert lib.d4w_project_subtract_f32(vp(x), I64(50), 3, 50, None, I64(0), 0, None, None, None, 8, None, None, 0, 1, vp(y), I64(50), None, I64(0),
                                        None) == 0
    assert np.array_equal(y, x)


# ------------------------------------------------------------------------------------------
# bad arguments
# ------------------------------------------------------------------------------------------
def test_bad_arguments(lib):
    max_calls, max_length, _ = limits(lib)
    nch, ns = 5, 64
    x, nb = np.ones((nch, ns), dtype=np.float32), np.ones((nch, 7), dtype=np.float32)
    y, ynb = np.zeros_like(x), np.zeros_like(nb)
    k, f, start = np.zeros((1, nch), dtype=np.int32), np.zeros((1, nch), dtype=np.float32), np.zeros(1, dtype=np.int64)
    beam = np.ones((1, 8), dtype=np.float32)
    amp, coef = np.zeros((1, nch), dtype=np.float32), np.zeros((1, nch), dtype=np.float32)
    i = ctypes.c_int()

    def bad(rc, what):
        assert rc == -1, what
        assert len(lib.d4w_last_error()) > 0

    for j in range(3):
        args = [ctypes.byref(i)] * 3
        args[j] = None
        bad(lib.d4w_project_limits(*args), "limits %d" % j)

    def fit(x=x, pitch=ns, nch=nch, ns=ns, xn=None, pitchn=0, nsn=0, k=k, f=f, beam=beam, L=8, st=start, ncalls=1, order=1, amp=amp, coef=coef):
        return lib.d4w_project_f32(p(x), I64(pitch), nch, ns, p(xn), I64(pitchn), nsn, p(k), p(f), p(beam), L, p(st), ncalls, order, None, p(amp),
                                   p(coef), None)
    assert fit() == 0 and fit(order=0, f=None) == 0 and fit(order=3) == 0 and fit(xn=nb, pitchn=7, nsn=7) == 0
    for kw in (dict(x=None), dict(k=None), dict(f=None), dict(f=None, order=3), dict(beam=None), dict(st=None), dict(amp=None), dict(coef=None),
               dict(nch=0), dict(ns=0), dict(pitch=ns - 1), dict(ncalls=-1), dict(ncalls=max_calls + 1), dict(L=0), dict(L=-4), dict(L=max_length + 1),
               dict(order=2), dict(order=-1), dict(order=4), dict(xn=nb, pitchn=7, nsn=0), dict(xn=nb, pitchn=6, nsn=7), dict(xn=None, nsn=7)):
        bad(fit(**kw), kw)

    def sub(x=x, pitch=ns, nch=nch, ns=ns, xn=None, pitchn=0, nsn=0, k=k, f=f, beam=beam, L=8, st=start, amp=amp, ncalls=1, order=1, y=y, py=ns,
            yn=None, pyn=0):
        return lib.d4w_project_subtract_f32(p(x), I64(pitch), nch, ns, p(xn), I64(pitchn), nsn, p(k), p(f), p(beam), L, p(st), p(amp), ncalls, order,
                                            p(y), I64(py), p(yn), I64(pyn), None)
    assert sub() == 0 and sub(order=0, f=None) == 0 and sub(xn=nb, pitchn=7, nsn=7, yn=ynb, pyn=7) == 0
    xc, nc = x.copy(), nb.copy()
    assert sub(x=xc, y=xc) == 0 and sub(x=xc, y=xc, xn=nc, pitchn=7, nsn=7, yn=nc, pyn=7) == 0
    for kw in (dict(x=None), dict(y=None), dict(k=None), dict(f=None), dict(beam=None), dict(st=None), dict(amp=None), dict(nch=0), dict(ns=0),
               dict(pitch=ns - 1), dict(py=ns - 1), dict(ncalls=-1), dict(ncalls=max_calls + 1), dict(L=0), dict(L=max_length + 1), dict(order=2),
               dict(xn=nb, pitchn=7, nsn=7), dict(yn=ynb, pyn=7), dict(xn=nb, pitchn=7, nsn=7, yn=ynb, pyn=6), dict(xn=nb, pitchn=6, nsn=7, yn=ynb, pyn=7),
               dict(xn=None, nsn=7), dict(x=xc, y=xc, py=ns + 1), dict(x=xc, y=xc, xn=nc, pitchn=7, nsn=7, yn=ynb, pyn=7),
               dict(xn=nc, pitchn=7, nsn=7, yn=nc, pyn=7)):
        bad(sub(**kw), kw)
