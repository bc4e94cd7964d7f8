"""Delay-and-sum beam (csrc/beam.hip) in the CPU emulator build through the C ABI, against the float64 restatement of
tests/known_answers_beam.py.  Kernel logic only, host pointers; the cases are those of tests/beam_cases.py, which the
hardware runs as well (tests/test_beam_gpu.py).

Tolerance, derived: |beam - ref| <= (n + 16) 2^-24 A with n the contributing channels and A the sum of the absolute terms
(known_answers_beam); with normalize that bound over the weight sum plus 2 x 2^-24 |ref|.  No case is skipped or excluded.
"""
import ctypes

import numpy as np
import pytest

from tests import beam_cases as bc
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
    a, b, s, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.d4w_beam_limits(ctypes.byref(a), ctypes.byref(b), ctypes.byref(s)) == 0
    assert lib.d4w_beam_tile(ctypes.byref(t)) == 0
    return a.value, b.value, s.value, t.value


def ws_bytes(lib, nch, ncalls, nt):
    n = ctypes.c_size_t(12345)
    assert lib.d4w_beam_ws_bytes(nch, ncalls, nt, ctypes.byref(n)) == 0, lib.d4w_last_error()
    return n.value


def p(a):
    return vp(a) if a is not None else None


def emu_run(lib):
    def run(buf, ns, nxt, ns2, delays, order, weights, start, nt, normalize):
        buf = np.ascontiguousarray(buf, dtype=np.float32)
        nxt = np.ascontiguousarray(nxt, dtype=np.float32) if nxt is not None else None
        kr, f = (delays, None) if order == 0 else delays
        kr = np.ascontiguousarray(kr, dtype=np.int32)
        f = np.ascontiguousarray(f, dtype=np.float32) if f is not None else None
        ncalls, nch = kr.shape
        assert buf.shape[0] == nch
        start = np.ascontiguousarray(start, dtype=np.int64)
        w = np.ascontiguousarray(weights, dtype=np.float32) if weights is not None else None
        nbytes = ws_bytes(lib, nch, ncalls, nt)
        # the workspace between two guards: the call may write its nbytes and nothing else
        ws = np.full(nbytes // 4 + 2 * GUARD, -7.0, dtype=np.float32)
        out = np.full((ncalls, nt), -7.0, dtype=np.float32)
        rc = lib.d4w_beamform_f32(vp(buf), I64(buf.shape[1]), nch, ns, p(nxt), I64(nxt.shape[1] if nxt is not None else 0), ns2, vp(kr), p(f),
                                  p(w), vp(start), ncalls, nt, order, int(normalize),
                                  vp(out), ctypes.c_void_p(ws.ctypes.data + 4 * GUARD) if nbytes else None, None)
        assert rc == 0, lib.d4w_last_error()
        assert np.all(ws[:GUARD] == -7.0) and np.all(ws[len(ws) - GUARD:] == -7.0)
        return out
    return run


def emu_delays(lib):
    def delays(cable, c0, fs, pos, rounded):
        cable, pos = np.ascontiguousarray(cable, dtype=np.float64), np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        ncalls, nch = len(pos), len(cable)
        k, r = np.full((ncalls, nch), -7, dtype=np.int32), np.full((ncalls, nch), -7, dtype=np.int32)
        f = np.full((ncalls, nch), -7.0, dtype=np.float32)
        if rounded:
            rc = lib.d4w_beam_delays(vp(cable), nch, D(c0), D(fs), vp(pos), ncalls, None, None, vp(r), None)
        else:
            rc = lib.d4w_beam_delays(vp(cable), nch, D(c0), D(fs), vp(pos), ncalls, vp(k), vp(f), None, None)
        assert rc == 0, lib.d4w_last_error()
        return r if rounded else (k, f)
    return delays


def test_limits_and_workspace(lib):
    max_calls, max_length, S, T = limits(lib)
    assert max_calls >= 64 and max_length >= 120000 and S >= 2 and T >= 64
    assert ws_bytes(lib, S, 3, 100) == 0
    assert ws_bytes(lib, S + 1, 3, 100) >= 2 * 3 * 100 * 4
    assert ws_bytes(lib, 11020, 64, 12000) < 2 ** 31         # a file's block and 64 calls: well under the card's memory


def test_every_axis_value_occurs():
    cases = bc.parity_cases()
    assert 36 <= len(cases) <= 44 and len(set(cases)) == len(cases)
    for axis, values in enumerate(bc.AXES):
        assert {c[axis] for c in cases} == set(values), (axis, values)


@pytest.mark.parametrize("case", bc.parity_cases(), ids=bc.case_id)
def test_parity(lib, case):
    _, _, S, T = limits(lib)
    bc.check_parity(emu_run(lib), case, T, S)


def test_delay_table(lib):
    bc.check_delays(emu_delays(lib))


def test_both_tables_in_one_call_and_the_cap(lib):
    cable = np.array([[0.0, 0.0, 0.0], [1e13, 0.0, 0.0], [np.nan, 0.0, 0.0], [745.0, 0.0, 0.0]])
    pos = np.zeros((1, 3))
    k, r, f = np.zeros((1, 4), dtype=np.int32), np.zeros((1, 4), dtype=np.int32), np.ones((1, 4), dtype=np.float32)
    assert lib.d4w_beam_delays(vp(cable), 4, D(C0), D(50.0), vp(pos), 1, vp(k), vp(f), vp(r), None) == 0, lib.d4w_last_error()
    t = kb.tau(cable, C0, 50.0, pos)[0, 3]
    assert list(r[0, :3]) == [0, 1 << 30, 1 << 30] and list(k[0, :3]) == [0, 1 << 30, 1 << 30] and not f[0, :3].any()
    assert (k[0, 3], f[0, 3]) == tuple(a[()] for a in kb.split(t)) and r[0, 3] == kb.rounded(t)


@pytest.mark.parametrize("nch", [5, "S", "S+1"])
def test_rounded_delays_are_the_stack_table_and_order_0_its_columns(lib, nch):
    _, _, S, _ = limits(lib)
    nch = {"S": S, "S+1": S + 1}.get(nch, nch)
    cable, fs, xs, ys, z, env, w, (k0, k1) = bc.stack_scene(nch)
    cable = np.ascontiguousarray(cable)
    table = np.full((len(ys), len(xs), nch), -7, dtype=np.int32)
    assert lib.d4w_stack_delays_i32(vp(cable), nch, D(C0), D(fs), vp(xs), len(xs), vp(ys), len(ys), D(z), vp(table), None) == 0
    r = emu_delays(lib)(cable, C0, fs, bc.stack_nodes(xs, ys, z), True)
    assert np.array_equal(r, table.reshape(-1, nch))
    stack = np.full((len(ys), len(xs), k1 - k0), -7.0, dtype=np.float32)
    assert lib.d4w_stack_grid_f32(vp(env), I64(env.shape[1]), nch, env.shape[1], vp(table), vp(w), len(xs), len(ys), k0, k1, 0, 2, vp(stack),
                                  None, None) == 0, lib.d4w_last_error()
    bc.check_against_stack(emu_run(lib), stack, r, nch, S)


def test_ones(lib):
    bc.check_ones(emu_run(lib), limits(lib)[2])


def test_ramp(lib):
    _, _, S, T = limits(lib)
    bc.check_ramp(emu_run(lib), T, S)


def test_zeros(lib):
    _, _, S, T = limits(lib)
    bc.check_zeros(emu_run(lib), T, S)


def test_nan_rows(lib):
    _, _, S, T = limits(lib)
    bc.check_nan_rows(emu_run(lib), T, S)


def test_bit_identity(lib):
    _, _, S, T = limits(lib)
    bc.check_bit_identity(emu_run(lib), T, S)


def test_next_block_is_the_concatenation(lib):
    _, _, S, T = limits(lib)
    bc.check_next_block(emu_run(lib), T, S)


def test_extreme_starts_add_nothing(lib):
    x = np.ones((3, 50), dtype=np.float32)
    r = np.zeros((2, 3), dtype=np.int32)
    for s in (np.iinfo(np.int64).min, np.iinfo(np.int64).max, -(1 << 40), 1 << 40):
        got = emu_run(lib)(x, 50, None, 0, r, 0, None, np.array([s, 0], dtype=np.int64), 60, False)
        assert not got[0].any() and np.all(got[1, :50] == 3) and not got[1, 50:].any()


# ------------------------------------------------------------------------------------------
# bad arguments
# ------------------------------------------------------------------------------------------
def test_bad_arguments(lib):
    max_calls, max_length, S, _ = limits(lib)
    nch, ns, nt = 5, 64, 32
    cable = np.ascontiguousarray(bc.make_cable("line", nch))
    pos = np.array([[30000.0, 20000.0, -60.0]])
    k, r, f = np.zeros((1, nch), dtype=np.int32), np.zeros((1, nch), dtype=np.int32), np.zeros((1, nch), dtype=np.float32)
    x, nb = np.ones((nch, ns), dtype=np.float32), np.ones((nch, 7), dtype=np.float32)
    start, out = np.zeros(1, dtype=np.int64), np.zeros((1, nt), dtype=np.float32)
    nan, inf = float("nan"), float("inf")
    i = ctypes.c_int()
    n = ctypes.c_size_t()

    def bad(rc, what):
        assert rc == -1, what
        assert len(lib.d4w_last_error()) > 0

    bad(lib.d4w_beam_limits(None, ctypes.byref(i), ctypes.byref(i)), "limits")
    bad(lib.d4w_beam_limits(ctypes.byref(i), None, ctypes.byref(i)), "limits")
    bad(lib.d4w_beam_limits(ctypes.byref(i), ctypes.byref(i), None), "limits")
    bad(lib.d4w_beam_tile(None), "tile")

    def delays(cab=cable, nch=nch, c0=C0, fs=50.0, ps=pos, ncalls=1, k=k, f=f, r=r):
        return lib.d4w_beam_delays(p(cab), nch, D(c0), D(fs), p(ps), ncalls, p(k), p(f), p(r), None)
    assert delays() == 0 and delays(r=None) == 0 and delays(k=None, f=None) == 0
    for kw in (dict(cab=None), dict(ps=None), dict(k=None), dict(f=None), dict(k=None, f=None, r=None), dict(nch=0), dict(ncalls=0),
               dict(ncalls=max_calls + 1), dict(fs=0.0), dict(fs=nan), dict(fs=inf), dict(fs=-1.0), dict(c0=0.0), dict(c0=-C0), dict(c0=nan),
               dict(c0=inf)):
        bad(delays(**kw), kw)

    def wsb(nch=nch, ncalls=1, nt=nt, o=n):
        return lib.d4w_beam_ws_bytes(nch, ncalls, nt, ctypes.byref(o) if o is not None else None)
    assert wsb() == 0
    for kw in (dict(o=None), dict(nch=0), dict(ncalls=0), dict(ncalls=max_calls + 1), dict(nt=0), dict(nt=-1)):
        bad(wsb(**kw), kw)
    if max_length < 2 ** 31 - 1:
        bad(wsb(nt=max_length + 1), "length")

    def beam(x=x, pitch=ns, nch=nch, ns=ns, xn=None, pitchn=0, nsn=0, kr=k, f=f, st=start, ncalls=1, nt=nt, order=1, o=out, ws=None):
        return lib.d4w_beamform_f32(p(x), I64(pitch), nch, ns, p(xn), I64(pitchn), nsn, p(kr), p(f), None, p(st), ncalls, nt, order, 0, p(o), p(ws),
                                    None)
    assert beam() == 0 and beam(order=0, f=None) == 0 and beam(xn=nb, pitchn=7, nsn=7) == 0
    for kw in (dict(x=None), dict(kr=None), dict(st=None), dict(o=None), dict(f=None), dict(order=3, f=None), dict(order=2), dict(order=-1), dict(order=4),
               dict(nch=0), dict(ns=0), dict(pitch=ns - 1), dict(ncalls=0), dict(ncalls=max_calls + 1), dict(nt=0), dict(nt=-5),
               dict(xn=nb, pitchn=7, nsn=0), dict(xn=nb, pitchn=6, nsn=7), dict(xn=None, nsn=7)):
        bad(beam(**kw), kw)
    # more channels than a segment: the workspace d4w_beam_ws_bytes asks for must be given
    big, kk = np.ones((S + 1, ns), dtype=np.float32), np.zeros((1, S + 1), dtype=np.int32)
    bad(beam(x=big, nch=S + 1, kr=kk, order=0, f=None), "no workspace")
    ws = np.zeros(ws_bytes(lib, S + 1, 1, nt) // 4, dtype=np.float32)
    assert beam(x=big, nch=S + 1, kr=kk, order=0, f=None, ws=ws) == 0 and np.all(out == S + 1)
