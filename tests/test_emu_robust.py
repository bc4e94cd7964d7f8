"""Robust weighted relocation (csrc/robust.hip) in the CPU emulator build through the C ABI: the cases of tests/robust_cases.py
against the float64 restatement of tests/known_answers_robust.py, the exact properties the issue names, guard words around every
output, the optional outputs as NULL, every bad argument.  Kernel logic only, host pointers; the radix select's control flow
(prefix skip, digit passes, scan over the bins, the second middle statistic) runs here as on the device.  The limits and where
they come from: tests/robust_cases.py."""
import ctypes

import numpy as np
import pytest

from tests import known_answers_loc as ka
from tests import known_answers_robust as kr
from tests import robust_cases as rc
from tests.emu_util import load_emu, vp
from tests.test_emu_loc import emu_solve

C0 = rc.C0
LOSS = {"l2": 0, "huber": 1, "bisquare": 2}
GUARD = 4                                # guard words on either side of every output
D = ctypes.c_double


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def _guarded(shape, dtype=np.float64, fill=7):
    """(the whole buffer, the view of `shape` between the guard words)."""
    n = int(np.prod(shape))
    buf = np.full(n + 2 * GUARD, fill, dtype=dtype)
    return buf, buf[GUARD:GUARD + n].reshape(shape)


def emu_robust(lib, Ti, cable, weights=None, loss="huber", tuning=None, scale=None, Nbiter=10, warmup=4, fix_z=False, first_guess=None,
               c0=C0, optional=True, ws="auto"):
    """d4w_loc_robust_f64 on host arrays: dict of history, n, gtg, ssr, wsum, nused, scale, q, r.  Asserts the guard words."""
    Ti = np.ascontiguousarray(np.atleast_2d(np.asarray(Ti, dtype=np.float64)))
    cable = np.ascontiguousarray(cable, dtype=np.float64)
    ncalls, nch = Ti.shape
    p = 3 if fix_z else 4
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    fg = None if first_guess is None else np.ascontiguousarray(np.broadcast_to(np.asarray(first_guess, dtype=np.float64), (ncalls, 4)))
    shapes = dict(history=(ncalls, Nbiter, 4), n=(ncalls, 4), gtg=(ncalls, p, p), ssr=(ncalls,), wsum=(ncalls,), scale=(ncalls,),
                  q=(ncalls, nch), r=(ncalls, nch))
    bufs = {k: _guarded(s) for k, s in shapes.items()}
    bufs["nused"] = _guarded((ncalls,), np.int32, -7)
    nbytes = ctypes.c_size_t(12345)
    assert lib.d4w_loc_robust_ws_bytes(nch, ncalls, ctypes.byref(nbytes)) == 0
    assert nbytes.value == (8 * nch * ncalls if nch > rc.RESIDENT else 0)
    wsb = np.full(nbytes.value // 8 + 2 * GUARD, 7, dtype=np.uint64) if ws == "auto" else ws
    o = lambda k: vp(bufs[k][1]) if bufs[k][1].size or k != "history" else None
    opt = lambda k: o(k) if optional else None
    rcode = lib.d4w_loc_robust_f64(vp(cable), nch, vp(Ti), ncalls, vp(w) if w is not None else None, int(w is not None and w.ndim == 2),
                                   D(c0), Nbiter, warmup, int(fix_z), LOSS[loss], D(kr.TUNING[loss] if tuning is None else tuning),
                                   D(0.0 if scale is None else scale), vp(fg) if fg is not None else None, o("history"), o("n"), o("gtg"),
                                   o("ssr"), opt("wsum"), o("nused"), opt("scale"), opt("q"), opt("r"),
                                   ctypes.c_void_p(wsb.ctypes.data + 8 * GUARD) if wsb is not None else None, None)
    assert rcode == 0, lib.d4w_last_error()
    for k, (buf, view) in bufs.items():
        fill = -7 if k == "nused" else 7
        assert np.all(buf[:GUARD] == fill) and np.all(buf[-GUARD:] == fill), "guard words of %s" % k
        if not optional and k in ("wsum", "scale", "q", "r"):
            assert np.all(buf == fill), "%s was written although NULL was passed" % k
    if wsb is not None:
        assert np.all(wsb[:GUARD] == 7) and np.all(wsb[-GUARD:] == 7), "guard words of the workspace"
    return {k: v[1] for k, v in bufs.items()}


def run_case(lib, case, **kw):
    return emu_robust(lib, case["Ti"], case["cable"], weights=case["weights"], loss=case["loss"], scale=case["scale"], Nbiter=case["Nbiter"],
                      warmup=case["warmup"], fix_z=case["fix_z"], first_guess=case["first_guess"], **kw)


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


CASES = rc.parity_cases()


def test_limits(lib):
    a, b = ctypes.c_int(), ctypes.c_int()
    assert lib.d4w_loc_robust_limits(ctypes.byref(a), ctypes.byref(b)) == 0
    assert a.value == rc.RESIDENT and 1 <= b.value <= 8
    assert 8 * a.value + 4096 <= 160 * 1024                 # the keys and the kernel's own arrays fit a compute unit's LDS
    assert lib.d4w_loc_robust_limits(None, ctypes.byref(b)) == -1


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_parity_with_the_restatement(lib, case):
    o = run_case(lib, case)
    rc.check_against_restatement(case, o["history"], o["n"], o["scale"], o["q"], o["r"], o["nused"], o["gtg"], o["ssr"], o["wsum"])


def test_used_counts_are_odd_and_even():
    counts = {a["nused"] % 2 for c in CASES for a in rc.reference(c)}
    assert counts == {0, 1}


@pytest.mark.parametrize("nch,fix_z,nbiter,half", [(400, True, 10, False), (400, False, 10, True), (3000, False, 5, False), (257, True, 0, False),
                                                   (rc.RESIDENT + 1, True, 3, True)])
def test_l2_without_weights_is_solve_lq_batch_bit_for_bit(lib, nch, fix_z, nbiter, half):
    cable, Ti, _, _ = rc.scene(nch, 2, seed=nch)
    if half:
        Ti[:, ::2] = np.nan
    for fg in (None, [39000.0, 22000.0, -60.0, 10.0]):
        hist, n, gtg, ssr, npick = emu_solve(lib, Ti, cable, Nbiter=nbiter, fix_z=fix_z, first_guess=fg)
        o = emu_robust(lib, Ti, cable, loss="l2", Nbiter=nbiter, fix_z=fix_z, first_guess=fg)
        for a, b in ((hist, o["history"]), (n, o["n"]), (gtg, o["gtg"]), (ssr, o["ssr"]), (npick, o["nused"])):
            assert np.array_equal(a, b)
        assert np.array_equal(o["wsum"], npick.astype(np.float64)) and np.all(np.isnan(o["scale"]))
        # a warm-up that outlasts the iterations is l2 up to the final pass
        h = emu_robust(lib, Ti, cable, loss="huber", warmup=nbiter, Nbiter=nbiter, fix_z=fix_z, first_guess=fg)
        assert np.array_equal(h["history"], hist) and np.array_equal(h["n"], n) and np.all(h["scale"] > 0)


@pytest.mark.parametrize("loss", rc.LOSSES)
def test_weights_of_two_give_the_position_of_weights_of_one(lib, loss):
    cable, Ti, srcs, _ = rc.scene(1025, 2, seed=3)
    fg = srcs + [300.0, -200.0, 0.0, 0.05]
    # lambda = 1e-5 is not scaled with the weights (here it is 5 % of the smallest diagonal entry), so the two runs take
    # different steps to the same fixed point, sum w g r = 0: compared once both have arrived, after 60 iterations
    a = emu_robust(lib, Ti, cable, weights=np.ones(1025), loss=loss, warmup=0, Nbiter=60, fix_z=True, first_guess=fg)
    b = emu_robust(lib, Ti, cable, weights=np.full((2, 1025), 2.0), loss=loss, warmup=0, Nbiter=60, fix_z=True, first_guess=fg)
    d = np.abs(a["n"] - b["n"])
    print(loss, "largest difference: position %.3e m, t0 %.3e s" % (d[:, :3].max(), d[:, 3].max()))
    assert d[:, :3].max() <= rc.LIM_POS and d[:, 3].max() <= rc.LIM_T0, d
    assert np.array_equal(a["nused"], b["nused"])


@pytest.mark.parametrize("loss,nch", [("huber", 300), ("bisquare", rc.RESIDENT + 3), ("l2", 300)])
def test_unused_channels_may_hold_anything(lib, loss, nch):
    cable, Ti, srcs, _ = rc.scene(nch, 2, seed=11)
    fg = srcs + [300.0, -200.0, 0.0, 0.05]
    rng = np.random.default_rng(2)
    w = 0.5 + rng.random((2, nch))
    dead = rng.random((2, nch)) < 0.3
    w[dead] = rng.choice([0.0, -3.0, np.nan], int(dead.sum()))
    a = emu_robust(lib, Ti, cable, weights=w, loss=loss, warmup=1, Nbiter=4, first_guess=fg)
    Tg = np.where(dead, rng.choice([np.nan, 1e300, -1e300, 0.0], (2, nch)), Ti)
    b = emu_robust(lib, Tg, cable, weights=w, loss=loss, warmup=1, Nbiter=4, first_guess=fg)
    assert same(a, b)
    # a channel unused in every call: its cable row may be garbage too
    col = np.zeros(nch, dtype=bool)
    col[::5] = True
    w[:, col] = 0.0
    cg = cable.copy()
    cg[col] = [[np.nan, 1e300, -1e300]]
    for first_guess in (fg, None):
        a = emu_robust(lib, Ti, cable, weights=w, loss=loss, warmup=1, Nbiter=4, first_guess=first_guess)
        b = emu_robust(lib, Tg, cg, weights=w, loss=loss, warmup=1, Nbiter=4, first_guess=first_guess)
        assert same(a, b) and np.all(np.isfinite(a["n"]))


@pytest.mark.parametrize("src_xy", ka.KNOWN_SOUTH)
@pytest.mark.parametrize("loss", ["huber", "bisquare"])
def test_noise_free_known_sources_come_back_exactly(lib, src_xy, loss):
    cable = ka.make_cable("line", 11020)
    src = np.array([src_xy[0], src_xy[1], -60.0, 12.5])
    Ti = ka.arrival_times(src[3], cable, src[:3], C0)
    o = emu_robust(lib, Ti, cable, loss=loss, Nbiter=20, warmup=4, fix_z=True)
    print("known source", src_xy, loss, "n - src", o["n"][0] - src, "scale", o["scale"][0])
    assert np.array_equal(o["n"][0], src), o["n"][0] - src
    assert o["scale"][0] == 0.0 and np.all(o["q"] == 1.0) and o["ssr"][0] == 0.0 and np.all(o["r"] == 0.0)


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("loss", ["huber", "bisquare"])
def test_ties_give_numpys_median(lib, k, loss):
    cable, Ti, src = rc.tie_cases()[k]
    o = emu_robust(lib, Ti, cable, loss=loss, Nbiter=0, fix_z=True, first_guess=src)
    ar = np.abs(o["r"][0])
    assert np.array_equal(ar, np.abs(Ti[0] - ka.arrival_times(src[3], cable, src[:3], C0)))     # NumPy's roundings
    vals, counts = np.unique(ar, return_counts=True)
    assert counts.max() >= len(ar) // 2
    assert o["scale"][0] == kr.MAD * float(np.median(ar))


@pytest.mark.parametrize("m", [1, 2, 3, 4, 255, 256, 513, 514])
def test_median_of_every_small_count(lib, m):
    """m used channels among 600, their |r| spread over twelve decades with repeats: both middle statistics, every digit pass."""
    cable = ka.make_cable("bent", 600)
    src = np.array(ka.SOURCES["bent"][1])
    rng = np.random.default_rng(m)
    t = ka.arrival_times(src[3], cable, src[:3], C0)
    Ti = np.full(600, np.nan)
    pick = rng.choice(600, m, replace=False)
    Ti[pick] = t[pick] + rng.choice([-1.0, 1.0], m) * 10.0 ** rng.integers(-12, 1, m) * rng.choice([1.0, 1.5, 1.75], m)
    o = emu_robust(lib, Ti, cable, loss="huber", Nbiter=0, fix_z=True, first_guess=src)
    ar = np.abs(o["r"][0][pick])
    assert o["nused"][0] == m and o["scale"][0] == kr.MAD * float(np.median(ar))


def test_rerun_and_a_call_alone_against_the_batch(lib):
    case = next(c for c in CASES if c["id"].startswith("n%d_c3" % (rc.RESIDENT + 1)))
    a, b = run_case(lib, case), run_case(lib, case)
    assert same(a, b)
    for k in range(3):
        one = emu_robust(lib, case["Ti"][k], case["cable"], weights=case["weights"][k] if case["weights"].ndim == 2 else case["weights"],
                         loss=case["loss"], Nbiter=case["Nbiter"], warmup=case["warmup"], fix_z=case["fix_z"], first_guess=case["first_guess"][k])
        assert all(np.array_equal(one[key][0], a[key][k], equal_nan=True) for key in a), k


@pytest.mark.parametrize("loss", rc.LOSSES)
def test_call_without_a_used_channel_and_too_few_channels(lib, loss):
    cable, Ti, _, _ = rc.scene(64, 3, seed=5)
    w = np.ones((3, 64))
    w[1] = [0.0, -1.0, np.nan, 0.0] * 16
    Ti[2, 3:] = np.nan                                          # three used channels: nused <= p with either fix_z
    for fix_z in (False, True):
        for fg in (None, [38000.0, 21000.0, -60.0, 12.0]):
            o = emu_robust(lib, Ti, cable, weights=w, loss=loss, Nbiter=5, warmup=1, fix_z=fix_z, first_guess=fg)
            assert np.all(np.isnan(o["n"][1])) and np.all(np.isnan(o["history"][1])) and np.all(np.isnan(o["q"][1])) and np.all(np.isnan(o["r"][1]))
            assert o["nused"][1] == 0 and o["ssr"][1] == 0 and o["wsum"][1] == 0 and np.all(o["gtg"][1] == 0) and np.isnan(o["scale"][1])
            assert np.all(np.isfinite(o["n"][0])) and list(o["nused"]) == [64, 0, 3]
            assert o["nused"][2] <= (3 if fix_z else 4)         # what makes the variance NaN in dw.loc.solve_robust_batch


def test_optional_outputs_may_be_null(lib):
    case = CASES[5]
    a, b = run_case(lib, case), run_case(lib, case, optional=False)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("history", "n", "gtg", "ssr", "nused"))
    # no workspace is needed up to the resident limit, nor above it where no median is taken
    cable, Ti, _, _ = rc.scene(rc.RESIDENT + 1, 1, seed=1)
    emu_robust(lib, Ti, cable, loss="l2", Nbiter=1, ws=None)
    emu_robust(lib, Ti, cable, loss="huber", scale=1e-3, Nbiter=1, warmup=0, ws=None)
    emu_robust(lib, Ti[:, :300], cable[:300], loss="huber", Nbiter=1, warmup=0, ws=None)


@pytest.mark.parametrize("cable,Ti,src,moved", rc.accuracy_scenes(), ids=["bent_400", "bent_3000"])
@pytest.mark.parametrize("loss", ["huber", "bisquare"])
def test_moved_channels_are_down_weighted_and_the_position_improves(lib, cable, Ti, src, moved, loss):
    _, n_lq, _, _, _ = emu_solve(lib, Ti, cable, Nbiter=10, fix_z=True)
    o = emu_robust(lib, Ti, cable, loss=loss, Nbiter=10, fix_z=True)
    # horizontal: z is held at the first guess's -60 m, the sources lie at -35 m and -80 m
    e_lq, e_rb = float(np.linalg.norm(n_lq[0, :2] - src[:2])), float(np.linalg.norm(o["n"][0, :2] - src[:2]))
    low = o["q"][0] < 0.5
    print("%d channels, %s: position error %.3f m unweighted, %.3f m robust; t0 error %.2e / %.2e s; %d of %d moved channels and %d others below 0.5"
          % (len(cable), loss, e_lq, e_rb, abs(n_lq[0, 3] - src[3]), abs(o["n"][0, 3] - src[3]), int((low & moved).sum()), int(moved.sum()),
             int((low & ~moved).sum())))
    assert e_rb <= 0.5 * e_lq
    assert np.all(o["q"][0][moved] < 0.5)


def test_bad_arguments(lib):
    cable, Ti, _, _ = rc.scene(8, 1, seed=0)
    cable, Ti = np.ascontiguousarray(cable), np.ascontiguousarray(Ti)
    w = np.ones(8)
    hist, n, gtg, ssr, nused = np.zeros((1, 2, 4)), np.zeros((1, 4)), np.zeros((1, 4, 4)), np.zeros(1), np.zeros(1, dtype=np.int32)
    big = np.zeros((1, rc.RESIDENT + 1))

    def solve(nch=8, ncalls=1, c0=C0, nbiter=2, warmup=0, loss=1, tuning=1.345, scale=0.0, cab=cable, t=Ti, wt=None, per_call=0, h=hist,
              nn=n, g=gtg, s=ssr, nu=nused):
        p = lambda a: vp(a) if a is not None else None
        return lib.d4w_loc_robust_f64(p(cab), nch, p(t), ncalls, p(wt), per_call, D(c0), nbiter, warmup, 0, loss, D(tuning), D(scale), None,
                                      p(h), p(nn), p(g), p(s), None, p(nu), None, None, None, None, None)
    assert solve() == 0 and solve(wt=w) == 0 and solve(ncalls=0) == 0 and solve(nbiter=0, h=None) == 0 and solve(scale=1e-3) == 0
    bad = (dict(nch=0), dict(ncalls=-1), dict(c0=0.0), dict(c0=float("nan")), dict(c0=float("inf")), dict(nbiter=-1), dict(nbiter=100001),
           dict(cab=None), dict(t=None), dict(h=None), dict(nn=None), dict(g=None), dict(s=None), dict(nu=None), dict(warmup=-1),
           dict(loss=-1), dict(loss=3), dict(tuning=0.0), dict(tuning=-1.0), dict(tuning=float("nan")), dict(tuning=float("inf")),
           dict(scale=-1e-3), dict(scale=float("nan")), dict(scale=float("inf")), dict(per_call=1),
           dict(nch=rc.RESIDENT + 1, t=big))                    # a median above the resident limit without its workspace
    for kw in bad:
        assert solve(**kw) == -1, kw
        assert len(lib.d4w_last_error()) > 0
    nbytes = ctypes.c_size_t()
    assert lib.d4w_loc_robust_ws_bytes(0, 1, ctypes.byref(nbytes)) == -1 and lib.d4w_loc_robust_ws_bytes(8, -1, ctypes.byref(nbytes)) == -1
    assert lib.d4w_loc_robust_ws_bytes(8, 1, None) == -1
