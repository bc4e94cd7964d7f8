"""GPU parity of das4whales_amd.loc (csrc/loc.hip) through the Python interface.

Every comparison is against the fixture recorded from the reference's own loc module (tests/golden/loc.npz) or against
answers known without running anything.  The limits are those of tests/test_emu_loc.py, derived there: 100 x the largest
difference the sums-then-solve restatement showed against the fixture under permuted channel orders,
LIM_POS = 2.6e-7 m and LIM_T0 = 3.3e-11 s."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

from tests import known_answers_loc as ka
from tests.test_emu_loc import C0, CASES, EPS, G, GRID_XS, GRID_YS, case_data, check_n, grid_bounds

pytestmark = pytest.mark.gpu
GEOMS = sorted({str(G[c + "/geom"]) for c in CASES})


@pytest.fixture(scope="module")
def loc():
    assert torch.cuda.is_available()
    import das4whales_amd as dw
    return dw.loc


def _group(geom, fix_z):
    cases = [c for c in CASES if str(G[c + "/geom"]) == geom and bool(G[c + "/fix_z"]) == fix_z]
    return cases, G[geom + "/cable_pos"], np.stack([G[c + "/Ti"] for c in cases])


# ------------------------------------------------------------------------------------------
# fixture parity
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fix_z", [False, True])
@pytest.mark.parametrize("geom", GEOMS)
def test_batch_fixture_parity_and_stats(loc, geom, fix_z):
    cases, cable, Ti = _group(geom, fix_z)
    Ti0, cable0 = Ti.copy(), cable.copy()
    n, st = loc.solve_lq_batch(Ti, cable, C0, Nbiter=10, fix_z=fix_z, return_stats=True)
    assert np.array_equal(Ti, Ti0) and np.array_equal(cable, cable0)
    assert isinstance(n, np.ndarray) and n.dtype == np.float64 and n.shape == (len(cases), 4)
    p = 3 if fix_z else 4
    assert st["history"].shape == (len(cases), 10, 4) and st["covariance"].shape == (len(cases), p, p)
    assert st["uncertainty"].shape == (len(cases), p) and np.all(st["npicks"] == Ti.shape[1])
    n20 = loc.solve_lq_batch(Ti, cable, C0, Nbiter=20, fix_z=fix_z)
    for k, c in enumerate(cases):
        check_n(st["history"][k], G[c + "/hist"], c)       # every recorded iterate
        assert np.array_equal(n[k], st["history"][k, -1])
        check_n(n20[k], G[c + "/n20"], c)
        if float(G[c + "/noise"]) > 0:
            # a position within LIM_POS changes no residual by more than LIM_POS / c0 = 2e-10 s against 10 ms of noise
            assert np.isclose(st["variance"][k], float(G[c + "/var"]), rtol=1e-8), (c, st["variance"][k], float(G[c + "/var"]))
            # cov = var inv(G^T G): the inverse passes a relative change of G^T G on times its condition number; the change
            # is the rounding of the sums (4 n eps, gtg_close) plus the variance's 1e-8
            A, _, cnt = ka.stats_at(Ti[k], cable, C0, n[k], fix_z)
            tol = np.linalg.cond(A) * 4 * cnt * EPS + 1e-8
            ref = G[c + "/cov"]
            err = np.linalg.norm(st["covariance"][k] - ref, 2) / np.linalg.norm(ref, 2)
            print(c, "cov rel err %.3e bound %.3e" % (err, tol))
            assert err <= tol, (c, err, tol)
            if tol < 1e-6:
                assert np.allclose(st["uncertainty"][k], G[c + "/unc"], rtol=1e-5)


def test_single_call_prints_and_returns_like_the_reference(loc):
    case = "bent_3000_s1_n10_freez"
    cable, Ti, fix_z = case_data(case)
    Ti0 = Ti.copy()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        n = loc.solve_lq(Ti, cable, 1490.)
    assert np.array_equal(Ti, Ti0)
    assert isinstance(n, np.ndarray) and n.dtype == np.float64 and n.shape == (4,)
    check_n(n, G[case + "/hist"][-1], case)
    lines = buf.getvalue().splitlines()
    assert len(lines) == 10
    for j, line in enumerate(lines):
        m = re.fullmatch(r"Iteration (\d+): x = (-?\d+\.\d{4}) m, y = (-?\d+\.\d{4}), z = (-?\d+\.\d{4}), ti = (-?\d+\.\d{4})", line)
        assert m and int(m.group(1)) == j + 1, line
        h = G[case + "/hist"][j]
        ref = f'Iteration {j+1}: x = {h[0]:.4f} m, y = {h[1]:.4f}, z = {h[2]:.4f}, ti = {h[3]:.4f}'
        # the same line unless a value sits within LIM_POS of a rounding boundary of the fourth decimal
        assert line == ref or np.allclose([float(v) for v in m.groups()[1:]], h, rtol=0, atol=1.0001e-4), (line, ref)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        nz = loc.solve_lq(Ti.reshape(-1, 1), cable, C0, 20, True, verbose=False)
    assert buf.getvalue() == ""
    check_n(nz, G["bent_3000_s1_n10_fixz/n20"])


def test_tensor_in_tensor_out_on_the_current_stream(loc):
    case = "line_3000_s0_n10_fixz"
    cable, Ti, fix_z = case_data(case)
    tc, tt = torch.from_numpy(cable).cuda(), torch.from_numpy(Ti).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        n = loc.solve_lq(tt, tc, C0, fix_z=True, verbose=False)
        nb, st = loc.solve_lq_batch(tt[None], tc, C0, fix_z=True, return_stats=True)
        rms, t0 = loc.misfit_grid(tt, tc, C0, torch.linspace(30000, 45000, 16, dtype=torch.float64), np.linspace(15000, 25000, 5), -60.0)
        arr = loc.calc_arrival_times(1.5, tc, tt.new_tensor([38000.0, 21000.0, -60.0]), C0)
    s.synchronize()
    for t in (n, nb, st["history"], st["covariance"], rms, t0, arr):
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64
    assert n.shape == (4,) and rms.shape == (5, 16) and arr.shape == (3000,)
    check_n(n.cpu().numpy(), G[case + "/hist"][-1], case)
    assert torch.equal(nb[0], n)
    assert np.array_equal(n.cpu().numpy(), loc.solve_lq(Ti, cable, C0, fix_z=True, verbose=False))


# ------------------------------------------------------------------------------------------
# batches, missing picks, reruns, bad arguments
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,fix_z", [("line_400", False), ("bent_3000", True), ("line_11020", False)])
def test_batch_rows_equal_single_calls(loc, geom, fix_z):
    cases, cable, Ti = _group(geom, fix_z)
    nb, sb = loc.solve_lq_batch(Ti, cable, C0, fix_z=fix_z, return_stats=True)
    for k in range(len(cases)):
        n1, s1 = loc.solve_lq_batch(Ti[k:k + 1], cable, C0, fix_z=fix_z, return_stats=True)
        assert np.array_equal(nb[k], n1[0])                # bit for bit
        assert np.array_equal(nb[k], loc.solve_lq(Ti[k], cable, C0, fix_z=fix_z, verbose=False))
        for key in sb:
            assert np.array_equal(sb[key][k], s1[key][0], equal_nan=True), key


@pytest.mark.parametrize("geom", ["line_3000", "bent_11020", "line_400"])
def test_half_the_channels_missing(loc, geom):
    for fix_z in (False, True):
        cases = [c for c in _group(geom, fix_z)[0] if c + "/sub_idx" in G]
        assert len(cases) == 2
        cable = G[geom + "/cable_pos"]
        Ti = np.stack([G[c + "/Ti"] for c in cases])
        keep = np.zeros(Ti.shape[1], dtype=bool)
        keep[G[cases[0] + "/sub_idx"]] = True
        Ti[:, ~keep] = np.nan
        n, st = loc.solve_lq_batch(Ti, cable, C0, fix_z=fix_z, return_stats=True)
        n20 = loc.solve_lq_batch(Ti, cable, C0, Nbiter=20, fix_z=fix_z)
        assert np.all(st["npicks"] == keep.sum())
        for k, c in enumerate(cases):
            check_n(st["history"][k], G[c + "/sub_hist"], c)           # the reference run on the subset
            check_n(n20[k], G[c + "/sub_n20"], c)


def test_rerun_bit_identical(loc):
    cases, cable, Ti = _group("line_11020", False)
    Ti = np.concatenate([Ti] * 8)
    Ti[1, 100:900] = np.nan
    a, sa = loc.solve_lq_batch(Ti, cable, C0, return_stats=True)
    b, sb = loc.solve_lq_batch(Ti, cable, C0, return_stats=True)
    assert np.array_equal(a, b) and all(np.array_equal(sa[k], sb[k], equal_nan=True) for k in sa)
    assert np.array_equal(a[8:16], a[16:24]) and not np.array_equal(a[1], a[9])
    xs, ys = np.linspace(30000, 50000, 130), np.linspace(15000, 30000, 21)
    g1, g2 = loc.misfit_grid(Ti[:3], cable, C0, xs, ys, -60.0), loc.misfit_grid(Ti[:3], cable, C0, xs, ys, -60.0)
    assert all(np.array_equal(x, y) for x, y in zip(g1, g2))


def test_call_without_a_pick_and_too_few_picks(loc):
    cable, Ti, _ = case_data("bent_400_s0_n10_freez")
    Ti = np.stack([Ti, np.full_like(Ti, np.nan), Ti, Ti])
    Ti[3, 4:] = np.nan                                     # four picks: not more than the parameter count
    for fix_z in (False, True):
        n, st = loc.solve_lq_batch(Ti, cable, C0, Nbiter=5, fix_z=fix_z, return_stats=True)
        assert np.all(np.isnan(n[1])) and np.all(np.isnan(st["history"][1])) and st["npicks"][1] == 0
        assert np.isnan(st["variance"][1]) and np.all(np.isnan(st["covariance"][1])) and np.all(np.isnan(st["uncertainty"][1]))
        assert np.all(np.isfinite(n[[0, 2]])) and np.array_equal(n[0], n[2]) and np.isfinite(st["variance"][0])
        assert st["npicks"][3] == 4 and np.isnan(st["variance"][3]) == (not fix_z)
    rms, t0 = loc.misfit_grid(Ti, cable, C0, np.linspace(30000, 40000, 5), np.linspace(20000, 25000, 3), -60.0)
    assert np.all(np.isnan(rms[1])) and np.all(np.isnan(t0[1])) and np.all(np.isfinite(rms[[0, 2]]))
    fg = loc.first_guess_grid(Ti, cable, C0, np.linspace(30000, 40000, 5), np.linspace(20000, 25000, 3), -60.0)
    assert fg.shape == (4, 4) and np.all(np.isnan(fg[1])) and np.all(np.isfinite(fg[[0, 2, 3]]))


def test_bad_shapes(loc):
    cable, Ti, _ = case_data("line_400_s0_n0_freez")
    with pytest.raises(ValueError):
        loc.solve_lq(Ti[:-1], cable, C0, verbose=False)
    with pytest.raises(ValueError):
        loc.solve_lq(Ti, cable[:, :2], C0, verbose=False)
    with pytest.raises(ValueError):
        loc.solve_lq(np.stack([Ti, Ti]), cable, C0, verbose=False)
    with pytest.raises(ValueError):
        loc.solve_lq_batch(Ti, cable, C0)
    with pytest.raises(ValueError):
        loc.solve_lq_batch(Ti[None], cable, C0, first_guess=np.zeros((2, 4)))
    with pytest.raises(ValueError):
        loc.solve_lq_batch(Ti[None], cable, 0.0)
    with pytest.raises(ValueError):
        loc.solve_lq_batch(Ti[None], cable, C0, Nbiter=-1)
    with pytest.raises(ValueError):
        loc.misfit_grid(Ti, cable, C0, np.zeros(0), np.zeros(3), -60.0)
    with pytest.raises(ValueError):
        loc.calc_arrival_times(0.0, cable, np.zeros(4), C0)


# ------------------------------------------------------------------------------------------
# known answers that need no fixture
# ------------------------------------------------------------------------------------------
def _noise_free(src_xy):
    cable = ka.make_cable("line", 11020)
    src = np.array([src_xy[0], src_xy[1], -60.0, 12.5])
    return cable, src, ka.arrival_times(src[3], cable, src[:3], C0)


def test_known_sources_come_back_exactly(loc):
    cable = ka.make_cable("line", 11020)
    srcs = np.array([[x, y, -60.0, 12.5] for x, y in ka.KNOWN_SOUTH])
    Ti = np.stack([ka.arrival_times(s[3], cable, s[:3], C0) for s in srcs])
    n, st = loc.solve_lq_batch(Ti, cable, C0, Nbiter=20, fix_z=True, return_stats=True)
    print("known sources: n - src", n - srcs, "variance", st["variance"])
    assert np.array_equal(n, srcs), n - srcs


def test_north_source_comes_back_only_with_the_grid_start(loc):
    cable, src, Ti = _noise_free(ka.KNOWN_NORTH)
    n = loc.solve_lq(Ti, cable, C0, 20, True, verbose=False)
    assert np.linalg.norm(n[:2] - src[:2]) > 3000.0        # the mirror image
    fg = loc.first_guess_grid(Ti, cable, C0, GRID_XS, GRID_YS, -60.0)      # 32 m pitch: see tests/test_emu_loc.py
    assert fg.shape == (4,) and abs(fg[0] - src[0]) <= 32.0 and abs(fg[1] - src[1]) <= 32.0 and fg[2] == -60.0
    n = loc.solve_lq(Ti, cable, C0, 20, True, first_guess=fg, verbose=False)
    print("north source: start", fg, "n - src", n - src)
    assert np.array_equal(n, src), n - src


def test_grid_minimum_is_the_true_node(loc):
    cable = ka.make_cable("line", 11020)
    xs, ys = np.linspace(30000.0, 50000.0, 161), np.linspace(18000.0, 32000.0, 113)        # 125 m
    srcs = [(xs[64], ys[12], 12.5), (xs[120], ys[100], 3.0), (xs[0], ys[112], 40.0)]
    Ti = np.stack([ka.arrival_times(t, cable, [x, y, -60.0], C0) for x, y, t in srcs])
    rms, t0 = loc.misfit_grid(Ti, cable, C0, xs, ys, -60.0)
    fg = loc.first_guess_grid(Ti, cable, C0, xs, ys, -60.0)
    assert rms.shape == t0.shape == (3, 113, 161) and rms.dtype == np.float64
    for k, (x, y, t) in enumerate(srcs):
        iy, ix = np.unravel_index(np.argmin(rms[k]), rms[k].shape)
        assert (xs[ix], ys[iy]) == (x, y)
        print("grid node", k, "rms", rms[k, iy, ix], "t0 - true", t0[k, iy, ix] - t)
        assert rms[k, iy, ix] <= 4 * EPS * 60.0 and abs(t0[k, iy, ix] - t) <= 4 * EPS * 60.0
        assert np.array_equal(fg[k], [x, y, -60.0, t0[k, iy, ix]])


@pytest.mark.parametrize("case,nx,ny", [("line_400_s0_n10_freez", 70, 9), ("bent_3000_s2_n10_fixz", 64, 4), ("line_5_s1_n0_freez", 1, 1),
                                        ("line_11020_s1_n10_freez", 129, 33)])
def test_grid_against_restatement(loc, case, nx, ny):
    cable, Ti, _ = case_data(case)
    Ti = Ti.copy()
    if len(Ti) > 100:
        Ti[3:len(Ti):7] = np.nan
    xs, ys = np.linspace(28000.0, 52000.0, nx), np.linspace(16000.0, 31000.0, ny)
    rms, t0 = loc.misfit_grid(Ti, cable, C0, xs, ys, -45.0)
    assert rms.shape == (ny, nx)
    r_ref, t_ref, emax, spread = ka.misfit_grid_f64(Ti, cable, C0, xs, ys, -45.0)
    bt, bv = grid_bounds(len(Ti), emax, spread)
    assert np.max(np.abs(t0 - t_ref)) <= bt, (np.max(np.abs(t0 - t_ref)), bt)
    assert np.max(np.abs(rms ** 2 - r_ref ** 2)) <= bv, (np.max(np.abs(rms ** 2 - r_ref ** 2)), bv)
    assert np.max(np.abs(rms - r_ref)) <= 1e-9 * max(1.0, float(r_ref.max()))


# ------------------------------------------------------------------------------------------
# the small helpers and the uncertainty functions
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [g for g in GEOMS if not g.endswith("11020")])
def test_helpers_against_fixture(loc, geom):
    cable, w = G[geom + "/cable_pos"], G[geom + "/helpers_at"]
    arr = loc.calc_arrival_times(w[3], cable, w[:3], C0)
    assert isinstance(arr, np.ndarray) and arr.dtype == np.float64
    # square root and division are correctly rounded or within an ulp on the device; the sum of squares may be contracted nowhere
    assert np.allclose(arr, G[geom + "/arrival"], rtol=4 * EPS, atol=0)
    batch = loc.calc_arrival_times([w[3], 0.0], cable, np.stack([w[:3], w[:3] + 1.0]), C0)
    assert batch.shape == (2, len(cable)) and np.array_equal(batch[0], arr)
    for fn, key, pos in ((loc.calc_distance_matrix, "distance", w[:3]), (loc.calc_radii_matrix, "radii", w),
                         (loc.calc_theta_vector, "theta", w), (loc.calc_phi_vector, "phi", w)):
        y = fn(cable, pos)
        assert isinstance(y, np.ndarray) and y.dtype == np.float64
        assert np.allclose(y, G["%s/%s" % (geom, key)], rtol=8 * EPS, atol=0), key
        yt = fn(torch.from_numpy(cable).cuda(), torch.from_numpy(pos).cuda())
        assert yt.is_cuda and yt.dtype == torch.float64 and np.allclose(yt.cpu().numpy(), y, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", ["bent_3000_s0_n10_freez", "bent_3000_s0_n10_fixz", "line_3000_s2_n10_fixz", "line_400_s1_n10_freez"])
def test_variance_covariance_uncertainty_functions(loc, case):
    cable, Ti, fix_z = case_data(case)
    n = G[case + "/hist"][-1]                              # the reference's own result: the functions are compared like for like
    var = loc.cal_variance_residuals(Ti, loc.calc_arrival_times(n[3], cable, n[:3], C0), fix_z)
    assert np.isclose(var, float(G[case + "/var"]), rtol=1e-12)
    A, _, cnt = ka.stats_at(Ti, cable, C0, n, fix_z)
    tol = np.linalg.cond(A) * 4 * cnt * EPS + 1e-12
    with contextlib.redirect_stdout(io.StringIO()):
        cov = loc.calc_covariance_matrix(cable, n, C0, float(G[case + "/var"]), fix_z)
        unc = loc.calc_uncertainty_position(cable, n, C0, float(G[case + "/var"]), fix_z)
    ref = G[case + "/cov"]
    err = np.linalg.norm(cov - ref, 2) / np.linalg.norm(ref, 2)
    print(case, "cov rel err %.3e bound %.3e" % (err, tol))
    assert cov.shape == ref.shape and err <= tol, (err, tol)
    assert np.array_equal(unc, np.sqrt(np.diag(cov)))
