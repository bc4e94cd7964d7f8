"""Robust weighted relocation on hardware: dw.loc.solve_robust_batch over the cases of tests/robust_cases.py against the float64
restatement (NumPy and tensor containers, a caller's stream), the exact properties (l2 == solve_lq_batch bit for bit, also on the
11 020-channel fixture; unused channels; NumPy's median on ties; reruns and a call alone against the batch), the accuracy
condition of the issue, and dw.loc.relocate on beam_cases.e2e_scene() against the explicit composition.  The limits and where
they come from: tests/robust_cases.py.

Measured on an MI355X (the figures the prints below give; DESIGN.md 3.9e has the tables): the largest difference from the
restatement over the parity cases is 1.08e-11 m and 1.78e-15 s against limits of 1.7e-9 m and 1.8e-13 s; the two accuracy
scenes go from 2.479 m / 0.874 m (unweighted) to 0.306 m / 0.049 m (Huber) and 0.276 m / 0.044 m (bisquare); relocate on the
end-to-end scene ends 1.377 m from the source after a first solve at 1.795 m (plain second solve 0.926 m), and at max_lag = 10
2.277 m where the plain second solve is thrown to 8.466 m.
"""
import numpy as np
import pytest
import torch

from tests import beam_cases as bc
from tests import golden_npz
from tests import known_answers_loc as ka
from tests import known_answers_robust as kr
from tests import robust_cases as rc

pytestmark = pytest.mark.gpu
C0 = rc.C0
CASES = rc.parity_cases()


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available()
    import das4whales_amd as dw
    return dw


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else x


def solve(dw, case, tensor=False, **kw):
    f = cuda if tensor else (lambda a: a)
    args = dict(weights=f(case["weights"]), loss=case["loss"], scale=case["scale"], Nbiter=case["Nbiter"], warmup=case["warmup"],
                fix_z=case["fix_z"], first_guess=f(case["first_guess"]), return_stats=True)
    args.update(kw)
    n, st = dw.loc.solve_robust_batch(f(case["Ti"]), f(case["cable"]), C0, **args)
    if tensor:
        assert n.is_cuda and all(v.is_cuda for v in st.values())
    return host(n), {k: host(v) for k, v in st.items()}


def same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and all(np.array_equal(a[1][k], b[1][k], equal_nan=True) for k in a[1])


def test_limits(dw):
    assert dw.loc.robust_limits()[0] == rc.RESIDENT


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_parity_with_the_restatement(dw, case):
    tensor = CASES.index(case) % 2 == 1                     # the containers alternate over the cases
    n, st = solve(dw, case, tensor=tensor)
    rc.check_against_restatement(case, st["history"], n, st["scale"], st["robust_weights"], st["residuals"], st["nused"], None, None,
                                 st["weight_sum"], variance=st["variance"])
    p = 3 if case["fix_z"] else 4
    ok = st["nused"] > p
    assert np.all(np.isfinite(st["uncertainty"][ok])) and np.all(np.isnan(st["variance"][~ok]))


def test_sums_at_the_returned_position_through_the_c_abi(dw):
    """G^T W G, sum w r^2 and sum w, which the Python stats fold into the covariance: one case above the resident limit."""
    from das4whales_amd import _device as dev
    from das4whales_amd import _lib
    case = next(c for c in CASES if c["id"].startswith("n%d_c3" % (rc.RESIDENT + 1)))
    ncalls, nch = case["Ti"].shape
    p = 3 if case["fix_z"] else 4
    t, cable, w, fg = cuda(case["Ti"]), cuda(case["cable"]), cuda(case["weights"]), cuda(case["first_guess"])
    f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device="cuda")
    hist, n, gtg, ssr, wsum, sc, q, r = (f64(ncalls, case["Nbiter"], 4), f64(ncalls, 4), f64(ncalls, p, p), f64(ncalls), f64(ncalls), f64(ncalls),
                                         f64(ncalls, nch), f64(ncalls, nch))
    nused = torch.full((ncalls,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(8 * ncalls * nch, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib.d4w_loc_robust_f64(dev.ptr(cable), nch, dev.ptr(t), ncalls, dev.ptr(w), int(case["weights"].ndim == 2), C0, case["Nbiter"],
                                           case["warmup"], int(case["fix_z"]), rc.LOSSES.index(case["loss"]), kr.TUNING[case["loss"]], 0.0,
                                           dev.ptr(fg), dev.out_ptr(hist), dev.out_ptr(n), dev.out_ptr(gtg), dev.out_ptr(ssr), dev.out_ptr(wsum),
                                           dev.out_ptr(nused), dev.out_ptr(sc), dev.out_ptr(q), dev.out_ptr(r), dev.out_ptr(ws),
                                           dev.stream_ptr(t)))
    rc.check_against_restatement(case, *(host(x) for x in (hist, n, sc, q, r, nused, gtg, ssr, wsum)))


def test_a_callers_stream(dw):
    case = CASES[8]
    ref = solve(dw, case, tensor=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = solve(dw, case, tensor=True)
    s.synchronize()
    assert same(ref, out)


@pytest.mark.parametrize("nch,fix_z,nbiter,half", [(400, True, 10, False), (400, False, 10, True), (3000, False, 5, False), (257, True, 0, False),
                                                   (rc.RESIDENT + 1, True, 3, True)])
def test_l2_without_weights_is_solve_lq_batch_bit_for_bit(dw, nch, fix_z, nbiter, half):
    cable, Ti, _, _ = rc.scene(nch, 2, seed=nch)
    if half:
        Ti[:, ::2] = np.nan
    for fg in (None, [39000.0, 22000.0, -60.0, 10.0]):
        n0, s0 = dw.loc.solve_lq_batch(Ti, cable, C0, Nbiter=nbiter, fix_z=fix_z, first_guess=fg, return_stats=True)
        n1, s1 = dw.loc.solve_robust_batch(Ti, cable, C0, loss="l2", Nbiter=nbiter, fix_z=fix_z, first_guess=fg, return_stats=True)
        assert np.array_equal(n0, n1) and np.array_equal(s0["history"], s1["history"]) and np.array_equal(s0["npicks"], s1["nused"])
        for k in ("variance", "covariance", "uncertainty"):                   # G^T G, ssr and the count, through the host's rule
            assert np.array_equal(s0[k], s1[k], equal_nan=True), k
        assert np.all(np.isnan(s1["scale"])) and np.array_equal(s1["weight_sum"], s0["npicks"].astype(np.float64))


def test_l2_on_the_11020_channel_fixture_is_solve_lq_batch(dw):
    G = golden_npz.load("loc.npz")
    cases = [str(c) for c in G["cases"] if str(G[str(c) + "/geom"]) == "line_11020"]
    assert cases
    for fix_z in (False, True):
        sel = [c for c in cases if bool(G[c + "/fix_z"]) == fix_z]
        Ti, cable = np.stack([G[c + "/Ti"] for c in sel]), G["line_11020/cable_pos"]
        n0, s0 = dw.loc.solve_lq_batch(Ti, cable, float(G["c0"]), fix_z=fix_z, return_stats=True)
        n1, s1 = dw.loc.solve_robust_batch(Ti, cable, float(G["c0"]), loss="l2", fix_z=fix_z, return_stats=True)
        assert np.array_equal(n0, n1) and np.array_equal(s0["history"], s1["history"])
        assert all(np.array_equal(s0[k], s1[k], equal_nan=True) for k in ("variance", "covariance", "uncertainty"))
        d = np.abs(s1["history"][0] - G[sel[0] + "/hist"])
        assert d[:, :3].max() <= 2.6e-7 and d[:, 3].max() <= 3.3e-11          # tests/test_emu_loc.py's limits against the reference


@pytest.mark.parametrize("loss", rc.LOSSES)
def test_weights_of_two_give_the_position_of_weights_of_one(dw, loss):
    cable, Ti, srcs, _ = rc.scene(1025, 2, seed=3)
    fg = srcs + [300.0, -200.0, 0.0, 0.05]
    # lambda = 1e-5 is not scaled with the weights: both runs are compared at their common fixed point, after 60 iterations
    a = dw.loc.solve_robust_batch(Ti, cable, C0, weights=np.ones(1025), loss=loss, warmup=0, Nbiter=60, fix_z=True, first_guess=fg)
    b = dw.loc.solve_robust_batch(Ti, cable, C0, weights=np.full((2, 1025), 2.0), loss=loss, warmup=0, Nbiter=60, fix_z=True, first_guess=fg)
    d = np.abs(a - b)
    print(loss, "largest difference: position %.3e m, t0 %.3e s" % (d[:, :3].max(), d[:, 3].max()))
    assert d[:, :3].max() <= rc.LIM_POS and d[:, 3].max() <= rc.LIM_T0, d


@pytest.mark.parametrize("loss,nch", [("huber", 300), ("bisquare", rc.RESIDENT + 3), ("l2", 300)])
def test_unused_channels_may_hold_anything(dw, loss, nch):
    cable, Ti, srcs, _ = rc.scene(nch, 2, seed=11)
    fg = srcs + [300.0, -200.0, 0.0, 0.05]
    rng = np.random.default_rng(2)
    w = 0.5 + rng.random((2, nch))
    dead = rng.random((2, nch)) < 0.3
    w[dead] = rng.choice([0.0, -3.0, np.nan], int(dead.sum()))
    col = np.zeros(nch, dtype=bool)
    col[::5] = True
    w[:, col] = 0.0
    dead |= col[None, :]
    Tg = np.where(dead, rng.choice([np.nan, 1e300, -1e300, 0.0], (2, nch)), Ti)
    cg = cable.copy()
    cg[col] = [[np.nan, 1e300, -1e300]]
    for first_guess in (fg, None):
        kw = dict(weights=w, loss=loss, warmup=1, Nbiter=4, first_guess=first_guess, return_stats=True)
        a, b = dw.loc.solve_robust_batch(Ti, cable, C0, **kw), dw.loc.solve_robust_batch(Tg, cg, C0, **kw)
        assert same(a, b) and np.all(np.isfinite(a[0]))


@pytest.mark.parametrize("src_xy", ka.KNOWN_SOUTH)
def test_noise_free_known_sources_come_back_exactly(dw, src_xy):
    cable = ka.make_cable("line", 11020)
    src = np.array([src_xy[0], src_xy[1], -60.0, 12.5])
    Ti = np.stack([ka.arrival_times(src[3], cable, src[:3], C0)] * 2)
    for loss in ("huber", "bisquare"):
        n, st = dw.loc.solve_robust_batch(Ti, cable, C0, loss=loss, Nbiter=20, fix_z=True, return_stats=True)
        print("known source", src_xy, loss, "n - src", n[0] - src, "scale", st["scale"][0])
        assert np.array_equal(n[0], src) and np.array_equal(n[1], src), n - src
        assert np.all(st["scale"] == 0.0) and np.all(st["robust_weights"] == 1.0) and np.all(st["residuals"] == 0.0)


def test_ties_and_small_counts_give_numpys_median(dw):
    for cable, Ti, src in rc.tie_cases():
        n, st = dw.loc.solve_robust_batch(Ti, cable, C0, loss="bisquare", Nbiter=0, fix_z=True, first_guess=src, return_stats=True)
        ar = np.abs(st["residuals"][0])
        assert np.array_equal(ar, np.abs(Ti[0] - ka.arrival_times(src[3], cable, src[:3], C0)))
        assert st["scale"][0] == kr.MAD * float(np.median(ar))
    cable = ka.make_cable("bent", 600)
    src = np.array(ka.SOURCES["bent"][1])
    t = ka.arrival_times(src[3], cable, src[:3], C0)
    counts = (1, 2, 3, 4, 255, 256, 513, 514)
    Ti = np.full((len(counts), 600), np.nan)
    for k, m in enumerate(counts):                          # |r| over twelve decades with repeats: every digit pass, both middles
        rng = np.random.default_rng(m)
        pick = rng.choice(600, m, replace=False)
        Ti[k, pick] = t[pick] + rng.choice([-1.0, 1.0], m) * 10.0 ** rng.integers(-12, 1, m) * rng.choice([1.0, 1.5, 1.75], m)
    n, st = dw.loc.solve_robust_batch(Ti, cable, C0, loss="huber", Nbiter=0, fix_z=True, first_guess=src, return_stats=True)
    for k, m in enumerate(counts):
        ar = np.abs(st["residuals"][k])
        assert st["nused"][k] == m and st["scale"][k] == kr.MAD * float(np.median(ar[~np.isnan(ar)])), m


def test_rerun_and_a_call_alone_against_the_batch(dw):
    for case in (next(c for c in CASES if c["id"].startswith("n%d_c3" % (rc.RESIDENT + 1))), next(c for c in CASES if c["id"].startswith("n1025_c3"))):
        a, b = solve(dw, case), solve(dw, case, tensor=True)
        assert same(a, b)
        for k in range(3):
            one = dict(case, Ti=case["Ti"][k:k + 1], first_guess=case["first_guess"][k:k + 1],
                       weights=case["weights"][k:k + 1] if case["weights"].ndim == 2 else case["weights"])
            o = solve(dw, one)
            assert np.array_equal(o[0][0], a[0][k], equal_nan=True)
            assert all(np.array_equal(o[1][key][0], a[1][key][k], equal_nan=True) for key in a[1]), k


@pytest.mark.parametrize("loss", rc.LOSSES)
def test_call_without_a_used_channel_and_too_few_channels(dw, loss):
    cable, Ti, _, _ = rc.scene(64, 3, seed=5)
    w = np.ones((3, 64))
    w[1] = [0.0, -1.0, np.nan, 0.0] * 16
    Ti[2, 3:] = np.nan
    for fix_z in (False, True):
        for fg in (None, [38000.0, 21000.0, -60.0, 12.0]):
            n, st = dw.loc.solve_robust_batch(Ti, cable, C0, weights=w, loss=loss, Nbiter=5, warmup=1, fix_z=fix_z, first_guess=fg, return_stats=True)
            assert np.all(np.isnan(n[1])) and np.all(np.isnan(st["history"][1])) and np.all(np.isnan(st["robust_weights"][1]))
            assert np.all(np.isnan(st["covariance"][1])) and np.isnan(st["scale"][1]) and st["weight_sum"][1] == 0
            assert list(st["nused"]) == [64, 0, 3] and np.all(np.isfinite(n[0]))
            assert np.isfinite(st["variance"][0]) and np.isnan(st["variance"][1]) and np.isnan(st["variance"][2])


@pytest.mark.parametrize("loss", ["huber", "bisquare"])
def test_moved_channels_are_down_weighted_and_the_position_improves(dw, loss):
    for cable, Ti, src, moved in rc.accuracy_scenes():
        n_lq = dw.loc.solve_lq_batch(Ti, cable, C0, Nbiter=10, fix_z=True)
        n, st = dw.loc.solve_robust_batch(Ti, cable, C0, loss=loss, Nbiter=10, fix_z=True, return_stats=True)
        # horizontal: z is held at the first guess's -60 m, the sources lie at -35 m and -80 m
        e_lq, e_rb = float(np.linalg.norm(n_lq[0, :2] - src[:2])), float(np.linalg.norm(n[0, :2] - src[:2]))
        low = st["robust_weights"][0] < 0.5
        print("%d channels, %s: position error %.3f m unweighted, %.3f m robust; t0 error %.2e / %.2e s; %d of %d moved channels and %d others below 0.5"
              % (len(cable), loss, e_lq, e_rb, abs(n_lq[0, 3] - src[3]), abs(n[0, 3] - src[3]), int((low & moved).sum()), int(moved.sum()),
                 int((low & ~moved).sum())))
        assert e_rb <= 0.5 * e_lq
        assert np.all(st["robust_weights"][0][moved] < 0.5)


# ------------------------------------------------------------------------------------------
# relocate
# ------------------------------------------------------------------------------------------
LEAD = 20


@pytest.fixture(scope="module")
def located(dw):
    """bc.e2e_scene() through locate_stack and the first solve: (scene, fs, n [1 x 4], Ti of locate_stack)."""
    sc = bc.e2e_scene()
    env = bc.matched_envelope(sc["x"], sc["burst"])
    Ti, info = dw.loc.locate_stack(env, bc.E2E_FS, sc["cable"], C0, sc["xs"], sc["ys"], sc["z"], 900.0, 30, 0.0)
    n = dw.loc.solve_lq_batch(Ti, sc["cable"], C0, fix_z=True, first_guess=info["first_guess"])
    return sc, bc.E2E_FS, n, Ti


def one_round(dw, x, fs, cable, n, length, max_lag, **kw):
    """relocate's round written out with the public calls: (n, Ti, coef, beam)."""
    start = np.round(n[:, 3] * fs).astype(np.int64) - LEAD
    beam, _ = dw.loc.beamform(x, fs, cable, C0, n[:, :3], start=start, length=length, order=3)
    Ti, coef = dw.loc.refine_arrivals(x, fs, cable, C0, n[:, :3], beam, start, max_lag)
    w = np.maximum(coef.astype(np.float64), 0.0) ** 2.0
    return dw.loc.solve_robust_batch(Ti, cable, C0, weights=w, warmup=0, fix_z=True, first_guess=n, **kw), Ti, coef, beam


def herr(n):
    return float(np.hypot(n[0, 0] - bc.E2E_SOURCE[0], n[0, 1] - bc.E2E_SOURCE[1]))


def test_relocate_is_the_composition_and_improves_the_position(dw, located):
    sc, fs, n, _ = located
    x, cable, L = sc["x"], sc["cable"], len(sc["burst"]) + 2 * LEAD
    n1, Ti1, coef1, beam1 = one_round(dw, x, fs, cable, n, L, 4)
    r1, st = dw.loc.relocate(x, fs, cable, C0, n, L, 4, lead=LEAD, return_stats=True)
    assert np.array_equal(r1, n1) and np.array_equal(st["Ti"], Ti1, equal_nan=True) and np.array_equal(st["coef"], coef1, equal_nan=True)
    assert np.array_equal(st["beam"], beam1) and st["history"].shape == (1, 10, 4) and np.array_equal(st["history"][:, -1], r1)
    assert np.array_equal(dw.loc.relocate(x, fs, cable, C0, n, L, 4, lead=LEAD), n1)
    n2 = one_round(dw, x, fs, cable, n1, L, 4)[0]
    assert np.array_equal(dw.loc.relocate(x, fs, cable, C0, n, L, 4, lead=LEAD, rounds=2), n2)
    rt = dw.loc.relocate(cuda(x), fs, cable, C0, cuda(n), L, 4, lead=LEAD, rounds=2)           # tensors: the same bits, on the device
    assert rt.is_cuda and np.array_equal(rt.cpu().numpy(), n2)
    # the measurements DESIGN.md 3.9e records
    plain = dw.loc.solve_lq_batch(Ti1, cable, C0, fix_z=True, first_guess=n)
    start = np.round(n[:, 3] * fs).astype(np.int64) - LEAD
    Ti10, _ = dw.loc.refine_arrivals(x, fs, cable, C0, n[:, :3], beam1, start, 10)
    plain10 = dw.loc.solve_lq_batch(Ti10, cable, C0, fix_z=True, first_guess=n)
    rob10 = dw.loc.relocate(x, fs, cable, C0, n, L, 10, lead=LEAD)
    bis = dw.loc.relocate(x, fs, cable, C0, n, L, 4, lead=LEAD, loss="bisquare")
    print("horizontal position error, m: first solve %.3f; max_lag 4: plain second solve %.3f, relocate %.3f (bisquare %.3f), two rounds %.3f; "
          "max_lag 10: plain %.3f, relocate %.3f" % (herr(n), herr(plain), herr(n1), herr(bis), herr(n2), herr(plain10), herr(rob10)))
    assert herr(n1) < herr(n)
