"""Window-normalised matched filter (csrc/nmf.hip) in the CPU emulator build through the C ABI, against the float64 restatement
of tests/known_answers_nmf.py: the cases of tests/nmf_cases.py, which tests/test_nmf_gpu.py runs on the hardware.  Kernel
logic only, host pointers.  The "public call" here is the chain detect.compute_nmf_correlograms drives -- d4w_row_stats_f32,
d4w_xcorr_mm_tail_f32 with the de-meaned supports and no tail, d4w_nmf_normalise_f32 -- put together by hand."""
import ctypes

import numpy as np
import pytest
import scipy.signal as sps

from oracle import d4w_oracle as orc
from tests import known_answers_nmf as kn
from tests import nmf_cases as nc
from tests.emu_util import load_emu, vp

D = ctypes.c_double


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def p(a):
    return vp(a) if a is not None else None


def emu_kernel(lib, x, head, n_next, mean, mx, cs, ms, norms, center, floor, want_max, want_rc=0):
    nx, ns = x.shape
    outs = [np.array(c, dtype=np.float32, copy=True) for c in cs]
    rmax = [np.full(nx, np.nan, dtype=np.float32) for _ in cs] if want_max else [None, None]
    rc = lib.d4w_nmf_normalise_f32(vp(x), nx, ns, p(head), head.shape[1] if head is not None else 0, n_next,
                                   vp(np.ascontiguousarray(mean, dtype=np.float64)), vp(np.ascontiguousarray(mx, dtype=np.float32)),
                                   len(ms), ms[0], ms[-1], D(norms[0]), D(norms[-1]), int(center), D(floor),
                                   vp(outs[0]), vp(outs[1]) if len(outs) > 1 else None, p(rmax[0]), p(rmax[-1]) if len(outs) > 1 else None, None)
    assert rc == want_rc, lib.d4w_last_error()
    return outs, (rmax if want_max else None)


def emu_public(lib, x, templates, center, floor, head):
    x = np.ascontiguousarray(x, dtype=np.float32)
    nx, ns = x.shape
    taps_list = [kn.demeaned(t).astype(np.float32) for t in templates]
    mean, mx = np.empty(nx, dtype=np.float64), np.empty(nx, dtype=np.float32)
    assert lib.d4w_row_stats_f32(vp(x), nx, ns, vp(mean), vp(mx), None) == 0
    outs = []
    for i in range(0, len(taps_list), 2):
        grp = taps_list[i:i + 2]
        lt = max(4, -(-max(len(t) for t in grp) // 4) * 4)
        taps = np.zeros((len(grp), lt), dtype=np.float32)
        for k, t in enumerate(grp):
            taps[k, :len(t)] = t
        n_next = max(len(t) for t in grp) - 1 if head is not None else 0
        hd = np.ascontiguousarray(head, dtype=np.float32) if n_next > 0 else None
        ys = [np.full_like(x, np.nan) for _ in grp]
        rc = lib.d4w_xcorr_mm_tail_f32(vp(x), nx, ns, p(hd), hd.shape[1] if hd is not None else 0, n_next, vp(mean), vp(mx), vp(taps),
                                       len(grp), lt, len(grp[0]), len(grp[-1]), D(0.0), D(0.0), vp(ys[0]), vp(ys[1]) if len(ys) > 1 else None,
                                       None, None, None)
        assert rc == 0, lib.d4w_last_error()
        norms = [float(np.sqrt(np.sum(t.astype(np.float64) ** 2))) for t in grp]
        got, _ = emu_kernel(lib, x, hd, n_next, mean, mx, ys, [len(t) for t in grp], norms, center, floor, False)
        outs.extend(got)
    return outs


def test_constants(lib):
    assert lib.d4w_nmf_tile() == kn.TILE
    assert lib.d4w_nmf_max_support() == nc.MAX_SUPPORT >= lib.d4w_xcorr_mm_max_support()


@pytest.mark.parametrize("ns_form", nc.NS_FORMS)
@pytest.mark.parametrize("support", list(nc.SUPPORTS))
def test_kernel_alone(lib, support, ns_form):
    nc.check_kernel_alone(lambda *a: emu_kernel(lib, *a), support, ns_form)


def test_public_call_on_the_scene(lib):
    nc.check_public_on_scene(lambda *a: emu_public(lib, *a))


def test_properties_on_the_scene(lib):
    nc.check_properties(lambda *a: emu_public(lib, *a),
                        pick_times=lambda c, thr: [sps.find_peaks(r, prominence=thr)[0] for r in np.asarray(c, dtype=np.float64)],
                        reference_correlogram=lambda x, t: orc.compute_cross_correlogram(np.asarray(x, dtype=np.float64), t))


def test_row_maxima_epilogue_on_the_scene(lib):
    x, head = kn.scene()
    tp = kn.templates()
    mean, mx = x.astype(np.float64).mean(axis=1), np.abs(x).max(axis=1)
    rng = np.random.default_rng(4)
    cs = [rng.uniform(-1.0, 0.0, x.shape).astype(np.float32), rng.uniform(-1.0, 1.0, x.shape).astype(np.float32)]     # one negative throughout
    ms = [len(kn.support(tp["hf"])), len(kn.support(tp["lf"]))]
    outs, rmax = emu_kernel(lib, x, head, ms[1] - 1, mean, mx, cs, ms, [1.5, 2.5], True, kn.FLOOR, True)
    for o, r in zip(outs, rmax):
        assert np.array_equal(r, o.max(axis=1))
    assert rmax[0][5] == 0 and np.all(rmax[0][[0, 1, 2, 4, 7]] < 0)


def test_bad_arguments(lib):
    nx, ns = 2, 300
    x = np.ones((nx, ns), dtype=np.float32)
    mean, mx = np.ones(nx), np.ones(nx, dtype=np.float32)
    cs = [np.zeros((nx, ns), dtype=np.float32), np.zeros((nx, ns), dtype=np.float32)]
    head = np.ones((nx, 40), dtype=np.float32)
    rm = np.zeros(nx, dtype=np.float32)
    nan, inf = float("nan"), float("inf")

    def call(x=x, nx=nx, ns=ns, head=head, ld=40, n_next=30, mean=mean, mx=mx, ntpl=2, l0=31, l1=20, n0=1.0, n1=2.0, center=1, floor=1e-6,
             y0=cs[0], y1=cs[1], r0=None, r1=None):
        return lib.d4w_nmf_normalise_f32(p(x), nx, ns, p(head), ld, n_next, p(mean), p(mx), ntpl, l0, l1, D(n0), D(n1), center, D(floor),
                                         p(y0), p(y1), p(r0), p(r1), None)
    assert call() == 0 and call(r0=rm, r1=rm.copy()) == 0 and call(ntpl=1, y1=None, r0=rm) == 0 and call(head=None, ld=0, n_next=0) == 0
    assert call(n0=0.0) == 0                                   # a template without shape: zeros, not an error
    for kw in (dict(x=None), dict(y0=None), dict(y1=None), dict(mean=None), dict(mx=None), dict(nx=0), dict(ns=0), dict(ntpl=0), dict(ntpl=3),
               dict(l0=0), dict(l1=0), dict(l0=nc.MAX_SUPPORT + 1), dict(l1=nc.MAX_SUPPORT + 1), dict(n0=-1.0), dict(n1=nan), dict(n0=inf),
               dict(floor=-1e-6), dict(floor=nan), dict(floor=inf), dict(center=2), dict(center=-1), dict(n_next=-1), dict(n_next=41),
               dict(r0=rm), dict(r1=rm)):
        assert call(**kw) == -1, kw
        assert len(lib.d4w_last_error()) > 0
