"""STA/LTA detector and trigger (csrc/stalta.hip) in the CPU emulator build through the C ABI, against the float64 restatement of
tests/known_answers_stalta.py: the cases of tests/stalta_cases.py, which tests/test_stalta_gpu.py runs on the hardware.  Kernel
logic only, host pointers; every D4W_EINVAL of the three entry points."""
import ctypes

import numpy as np
import pytest

from tests import known_answers_stalta as ks
from tests import stalta_cases as sc
from tests.emu_util import load_emu, vp

D, Z, LL = ctypes.c_double, ctypes.c_size_t, ctypes.c_longlong


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def p(a):
    return vp(a) if a is not None else None


def pitched(a, extra, fill=np.nan):
    """A copy of the 2-D array inside a buffer with `extra` more columns per row -> (view, pitch in elements)."""
    buf = np.full((a.shape[0], a.shape[1] + extra), fill, dtype=a.dtype)
    buf[:, :a.shape[1]] = a
    return buf[:, :a.shape[1]], buf.shape[1]


def emu_call(lib, x, prev, form, nsta, nlta, gap, floor, scale, rstate, nseen, want_ratio, trig):
    nx, ns = x.shape
    xv, ld = pitched(np.asarray(x, dtype=np.float32), 3)
    pv, ldp = pitched(np.asarray(prev, dtype=np.float32), 5) if prev is not None else (None, 0)
    rv, ldr = pitched(np.full((nx, ns), np.nan, dtype=np.float32), 1) if want_ratio else (None, 0)
    rin = np.ascontiguousarray(rstate, dtype=np.float64) if rstate is not None else None
    rout = np.full((nx, 2), np.nan)
    ev = peak = counts = act = on = off = ain = None
    cap = 0
    if trig is not None:
        on, off, ain, cap = trig
        on, off = np.ascontiguousarray(on, dtype=np.float64), np.ascontiguousarray(off, dtype=np.float64)
        ain = np.ascontiguousarray(ain, dtype=np.int32) if ain is not None else None
        ev, peak = np.full((nx, cap, 3), -7, dtype=np.int32), np.full((nx, cap), np.nan, dtype=np.float32)
        counts, act = np.full(nx, -7, dtype=np.int32), np.full(nx, -7, dtype=np.int32)
    rc = lib.d4w_stalta_f32(vp(xv), Z(ld), nx, ns, p(pv), Z(ldp), pv.shape[1] if pv is not None else 0, form, nsta, nlta, gap, D(floor),
                            vp(np.ascontiguousarray(scale, dtype=np.float32)), p(rin), vp(rout), LL(nseen), p(rv), Z(ldr),
                            p(on), p(off), p(ain), p(act), p(ev), p(peak), p(counts), cap, None)
    assert rc == 0, lib.d4w_last_error()
    return (np.array(rv) if want_ratio else None), rout, (ev, peak, counts, act)


def emu_ratio(lib, x, prev, form, nsta, nlta, gap, floor, scale, rstate, nseen):
    r, rout, _ = emu_call(lib, x, prev, form, nsta, nlta, gap, floor, scale, rstate, nseen, True, None)
    return r, rout


def emu_fused(lib, x, prev, form, nsta, nlta, gap, floor, scale, rstate, nseen, on, off, active, cap):
    return emu_call(lib, x, prev, form, nsta, nlta, gap, floor, scale, rstate, nseen, False, (on, off, active, cap))[2]


def emu_trigger(lib, r, on, off, active, cap):
    nx, ns = r.shape
    rv, ld = pitched(np.asarray(r, dtype=np.float32), 3)
    on, off = np.ascontiguousarray(on, dtype=np.float64), np.ascontiguousarray(off, dtype=np.float64)
    ain = np.ascontiguousarray(active, dtype=np.int32) if active is not None else None
    ev, peak = np.full((nx, cap, 3), -7, dtype=np.int32), np.full((nx, cap), np.nan, dtype=np.float32)
    counts, act = np.full(nx, -7, dtype=np.int32), np.full(nx, -7, dtype=np.int32)
    rc = lib.d4w_trigger_onset_f32(vp(rv), Z(ld), nx, ns, vp(on), vp(off), p(ain), vp(act), vp(ev), vp(peak), vp(counts), cap, None)
    assert rc == 0, lib.d4w_last_error()
    return ev, peak, counts, act


def test_constants(lib):
    assert lib.d4w_stalta_tile() == ks.TILE
    assert lib.d4w_stalta_max_window() == ks.MAX_WINDOW >= 16384


@pytest.mark.parametrize("ns_form", list(sc.NS_FORMS))
@pytest.mark.parametrize("params", list(sc.PARAMS))
@pytest.mark.parametrize("form", (ks.CLASSIC, ks.RECURSIVE))
def test_kernel_alone(lib, form, params, ns_form):
    sc.check_kernel_alone(lambda *a: emu_ratio(lib, *a), form, params, ns_form)


def test_dead_rows_and_gain(lib):
    sc.check_dead_and_gain(lambda *a: emu_ratio(lib, *a))


def test_trigger_alone(lib):
    sc.check_trigger(lambda *a: emu_trigger(lib, *a))


@pytest.mark.parametrize("form", (ks.CLASSIC, ks.RECURSIVE))
def test_scene(lib, form):
    sc.check_scene(lambda *a: emu_ratio(lib, *a), lambda *a: emu_trigger(lib, *a), lambda *a: emu_fused(lib, *a), form)


def test_ratio_and_events_in_one_call(lib):
    """ratio != NULL together with the events: both outputs equal the separate calls'."""
    x, scale = ks.scene()[:2, :5000], sc.scene_scale()[:2]
    a = ks.CLASSIC_ARGS
    on, off = np.full(2, a["thr_on"]), np.full(2, a["thr_off"])
    r, _, evs = emu_call(lib, x, None, 0, a["nsta"], a["nlta"], a["gap"], ks.FLOOR, scale, None, 0, True, (on, off, None, 8))
    r2, _ = emu_ratio(lib, x, None, 0, a["nsta"], a["nlta"], a["gap"], ks.FLOOR, scale, None, 0)
    assert np.array_equal(r, r2)
    assert sc.event_table(*evs[:3]) == sc.event_table(*emu_trigger(lib, r2, on, off, None, 8)[:3])


def test_pack_events(lib):
    r, on, off, active = sc.trigger_rows()
    nx, ns = r.shape
    cap = ns // 2 + 1
    ev, peak, counts, _ = emu_trigger(lib, r, on, off, active, cap)
    offs, summ = np.zeros(nx, dtype=np.int64), np.zeros(2, dtype=np.int64)
    assert lib.d4w_pick_offsets_i64(vp(counts), nx, vp(offs), vp(summ), None) == 0
    total = int(summ[1])
    assert summ[0] == counts.max() and total == counts.sum()
    out, pk = np.full((4, total), -7, dtype=np.int64), np.full(total, np.nan, dtype=np.float32)
    assert lib.d4w_pack_events_i64(vp(ev), vp(peak), vp(counts), vp(offs), nx, cap, ctypes.c_int64(total), vp(out), vp(pk), None) == 0
    want = np.array([(c,) + tuple(e) for c in range(nx) for e in ev[c, :counts[c]].tolist()], dtype=np.int64).T
    assert np.array_equal(out, want)
    assert np.array_equal(pk.view(np.uint32), np.concatenate([peak[c, :counts[c]] for c in range(nx)]).view(np.uint32))
    assert lib.d4w_pack_events_i64(vp(ev), vp(peak), vp(counts), vp(offs), nx, cap, ctypes.c_int64(0), None, None, None) == 0
    for kw in (dict(ev=None), dict(peak=None), dict(counts=None), dict(offs=None), dict(nx=0), dict(cap=0), dict(total=-1), dict(out=None),
               dict(pk=None)):
        a = dict(ev=ev, peak=peak, counts=counts, offs=offs, nx=nx, cap=cap, total=total, out=out, pk=pk)
        a.update(kw)
        assert lib.d4w_pack_events_i64(p(a["ev"]), p(a["peak"]), p(a["counts"]), p(a["offs"]), a["nx"], a["cap"], ctypes.c_int64(a["total"]),
                                       p(a["out"]), p(a["pk"]), None) == -1, kw


def test_bad_arguments(lib):
    nx, ns, cap = 2, 300, 8
    x = np.ones((nx, ns), dtype=np.float32)
    prev = np.ones((nx, 40), dtype=np.float32)
    scale = np.ones(nx, dtype=np.float32)
    rin, rout = np.zeros((nx, 2)), np.zeros((nx, 2))
    ratio = np.zeros((nx, ns), dtype=np.float32)
    on, off = np.full(nx, 3.0), np.full(nx, 1.5)
    ain, act = np.zeros(nx, dtype=np.int32), np.zeros(nx, dtype=np.int32)
    ev, peak, counts = np.zeros((nx, cap, 3), dtype=np.int32), np.zeros((nx, cap), dtype=np.float32), np.zeros(nx, dtype=np.int32)
    nan, inf = float("nan"), float("inf")
    ev_args = dict(on=on, off=off, ain=ain, act=act, ev=ev, peak=peak, counts=counts, cap=cap)
    no_ev = dict(on=None, off=None, ain=None, act=None, ev=None, peak=None, counts=None, cap=0)

    def call(x=x, ld=ns, nx=nx, ns=ns, prev=prev, ldp=40, n_prev=30, form=0, nsta=5, nlta=20, gap=3, floor=1e-6, scale=scale, rin=None,
             rout=None, nseen=0, ratio=ratio, ldr=ns, on=None, off=None, ain=None, act=None, ev=None, peak=None, counts=None, cap=0):
        return lib.d4w_stalta_f32(p(x), Z(ld), nx, ns, p(prev), Z(ldp), n_prev, form, nsta, nlta, gap, D(floor), p(scale), p(rin), p(rout),
                                  LL(nseen), p(ratio), Z(ldr), p(on), p(off), p(ain), p(act), p(ev), p(peak), p(counts), cap, None)
    assert call() == 0 and call(**ev_args) == 0 and call(ratio=None, ldr=0, **ev_args) == 0 and call(prev=None, ldp=0, n_prev=0) == 0
    assert call(form=1, gap=0, rin=rin, rout=rout, nseen=7) == 0 and call(floor=0.0) == 0
    assert call(nlta=ks.MAX_WINDOW - 3) == 0 and call(nsta=ks.MAX_WINDOW) == 0
    for kw in (dict(x=None), dict(scale=None), dict(nx=0), dict(ns=0), dict(ld=ns - 1), dict(form=2), dict(form=-1), dict(nsta=0), dict(nlta=0),
               dict(gap=-1), dict(form=1), dict(nlta=ks.MAX_WINDOW - 2), dict(nlta=ks.MAX_WINDOW + 1, gap=0), dict(nsta=ks.MAX_WINDOW + 1),
               dict(floor=-1e-6), dict(floor=nan), dict(floor=inf), dict(n_prev=-1), dict(n_prev=41), dict(prev=None), dict(form=1, gap=0, nseen=-1),
               dict(ratio=None), dict(ldr=ns - 1), dict(ev_args, on=None), dict(ev_args, off=None), dict(ev_args, ev=None),
               dict(ev_args, peak=None), dict(ev_args, counts=None), dict(ev_args, cap=0), dict(no_ev, on=on)):
        assert call(**kw) == -1, kw
        assert len(lib.d4w_last_error()) > 0

    def trig(r=ratio, ld=ns, nx=nx, ns=ns, on=on, off=off, ain=ain, act=act, ev=ev, peak=peak, counts=counts, cap=cap):
        return lib.d4w_trigger_onset_f32(p(r), Z(ld), nx, ns, p(on), p(off), p(ain), p(act), p(ev), p(peak), p(counts), cap, None)
    assert trig() == 0 and trig(ain=None, act=None) == 0
    for kw in (dict(r=None), dict(ld=ns - 1), dict(nx=0), dict(ns=0), dict(on=None), dict(off=None), dict(ev=None), dict(peak=None),
               dict(counts=None), dict(cap=0)):
        assert trig(**kw) == -1, kw
        assert len(lib.d4w_last_error()) > 0
