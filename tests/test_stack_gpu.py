"""GPU tests of the delay-and-sum stack (csrc/stack.hip) through das4whales_amd.loc: delay_table, stack_grid, stack_best,
arrivals_near and locate_stack, with NumPy input and with CUDA tensor input.

Parity is against the float64 restatement of tests/known_answers_stack.py.  Delays: exact under its margin rule (asserted on
the restatement's own numbers first).  Stack: the restatement sums along the package's own table; per element
|got - ref| <= 1.01 n 2^-24 sum |w env| over the n contributing terms, the bound of recursive float32 summation (with
normalize: divided by the weight sum, plus 2^-23 |ref|).  The known answer of the triangle scene needs no restatement:
400 channels of peak exactly 1.0 add up to exactly 400.0.
"""
import functools

import numpy as np
import pytest
import torch
from scipy import signal as scipy_signal

from tests import known_answers_stack as ks
from tests.known_answers_loc import C0, make_cable
from tests.test_emu_assoc import small_grid

pytestmark = pytest.mark.gpu
CONTAINERS = ("numpy", "tensor")


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available()
    import das4whales_amd as dw
    return dw


def put(x, container):
    if x is None or container == "numpy":
        return x
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(x, container):
    """The result on the host, after checking that it came back in the caller's container."""
    if container == "numpy":
        assert isinstance(x, np.ndarray)
        return x
    assert isinstance(x, torch.Tensor) and x.is_cuda
    return x.cpu().numpy()


def sub_grid(kind):
    xs, ys, z = ks.grid17(kind)
    return xs[3:8], ys[5:7], z                               # 5 x 2 nodes: two tiles, both partial


def weight_sets(nch, rng):
    some = rng.uniform(0.25, 2.0, nch).astype(np.float32)
    some[rng.random(nch) < 0.3] = 0.0
    some[0], some[-1] = 0.0, 1.5
    return {"ones": None, "some": some, "zeros": np.zeros(nch, dtype=np.float32)}


# ------------------------------------------------------------------------------------------
# the delay table
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("container", CONTAINERS)
@pytest.mark.parametrize("nch", [5, 67, 400])
@pytest.mark.parametrize("kind", ["line", "bent"])
def test_delay_table(dw, kind, nch, container):
    cable = make_cable(kind, nch)
    for shape in (1, 17, 65):
        xs, ys, z = ks.grid17(kind) if shape == 17 else small_grid(shape)
        for fs in (50.0, 200.0):
            ref, margin = ks.delay_table(cable, C0, fs, xs, ys, z)
            assert margin >= ks.MARGIN, margin
            got = host(dw.loc.delay_table(put(cable, container), C0, fs, put(xs, container), put(ys, container), z), container)
            assert got.dtype == np.int32 and np.array_equal(got, ref)


# ------------------------------------------------------------------------------------------
# the stack against the restatement
# ------------------------------------------------------------------------------------------
def forms(dw, env, table, w, nx, ny, k0, k1, normalize):
    """The window and the direct form on device tensors: (window, direct, info of each)."""
    e, t = torch.from_numpy(env).cuda(), torch.from_numpy(table).cuda()
    wd = torch.from_numpy(w).cuda() if w is not None else None
    a, ia = dw.loc._stack(e, e.shape[1], t, wd, nx, ny, k0, k1, normalize, form=1)
    b, ib = dw.loc._stack(e, e.shape[1], t, wd, nx, ny, k0, k1, normalize, form=2)
    return a.cpu().numpy(), b.cpu().numpy(), ia.cpu().numpy(), ib.cpu().numpy()


@pytest.mark.parametrize("container", CONTAINERS)
@pytest.mark.parametrize("ns", [257, 3000])
@pytest.mark.parametrize("nch", [5, 67, 400])
def test_stack_against_the_restatement(dw, nch, ns, container):
    rng = np.random.default_rng(1000 * nch + ns)
    kind = "bent" if (nch + ns) % 2 else "line"
    cable = make_cable(kind, nch)
    xs, ys, z = sub_grid(kind)
    fs = 50.0
    table = dw.loc.delay_table(cable, C0, fs, xs, ys, z)
    ref_table, margin = ks.delay_table(cable, C0, fs, xs, ys, z)
    assert margin >= ks.MARGIN and np.array_equal(table, ref_table)
    assert ks.tile_spread(ref_table) <= ks.WINDOW_SPREAD
    env = np.abs(rng.standard_normal((nch, ns))).astype(np.float32)
    worst = 0.0
    for k_range in (None, (-300, 120), (ns - 40, ns + 500), (0, 1)):
        k0, k1 = (0, ns) if k_range is None else k_range
        for name, w in weight_sets(nch, rng).items():
            for normalize in ((False, True) if name == "some" else (False,)):
                e = env.copy()
                if w is not None:
                    e[w == 0] = np.nan                       # a row under weight 0 must leave no trace
                wide = np.full((nch, ns + 5), np.nan, dtype=np.float32)      # a row pitch above ns, NaN in the padding
                wide[:, :ns] = e
                arg = put(wide, container)[:, :ns]           # tensor: a column-sliced view, read in place
                got, times = dw.loc.stack_grid(arg, fs, put(cable, container), C0, xs, ys, z, weights=put(w, container), k_range=k_range,
                                               normalize=normalize, delays=put(table, container) if name == "ones" else None)
                got, times = host(got, container), host(times, container)
                ref, bound = ks.stack_grid(env, ref_table, w, k_range, normalize)
                assert got.dtype == np.float32 and got.shape == ref.shape and np.all(np.isfinite(got))
                assert times.dtype == np.float64 and np.array_equal(times, np.arange(k0, k1) / fs)
                err = np.abs(got.astype(np.float64) - ref)
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if bound.max() > 0 else 0.0)
                assert np.all(err <= bound), (float((err - bound).max()), k_range, name, normalize)
                if name == "zeros":
                    assert np.all(got == 0)
                win, direct, iw, idr = forms(dw, e, table, w, len(xs), len(ys), k0, k1, normalize)
                assert iw[0] == 1 and idr[0] == 2
                assert np.array_equal(win.view(np.int32), direct.view(np.int32)) and np.array_equal(win.view(np.int32), got.view(np.int32))
    print("nch %d ns %d %s: largest error / bound %.3f" % (nch, ns, container, worst))


def test_choice_of_the_form(dw):
    rng = np.random.default_rng(65)
    nch, ns, fs = 67, 257, 200.0
    cable = make_cable("bent", nch)
    env = torch.from_numpy(np.abs(rng.standard_normal((nch, ns))).astype(np.float32)).cuda()
    xs, ys, z = small_grid(65)                               # 65 x 5 nodes, 2900 m between the rows: too wide for the window
    g17x, g17y, _ = ks.grid17("bent")
    tight = (g17x[8] + 150.0 * (np.arange(17) - 8), g17y[8] + 150.0 * (np.arange(17) - 8), z)
    for (gx, gy, gz), k_range, want in (((xs, ys, z), (-1500, 200), 2), (tight, (-2500, 200), 1)):
        table = dw.loc.delay_table(torch.from_numpy(cable).cuda(), C0, fs, gx, gy, gz)
        spread = ks.tile_spread(table.cpu().numpy().astype(np.int64))
        assert (spread > ks.WINDOW_SPREAD) == (want == 2) and spread > 0
        chosen, info = dw.loc._stack(env, ns, table, None, len(gx), len(gy), k_range[0], k_range[1], False, form=0)
        forced, info_f = dw.loc._stack(env, ns, table, None, len(gx), len(gy), k_range[0], k_range[1], False, form=want)
        public, _ = dw.loc.stack_grid(env, fs, cable, C0, gx, gy, gz, k_range=k_range, delays=table)
        assert info.tolist() == [want, spread] and info_f[0].item() == want
        assert bool(chosen.any()) and torch.equal(chosen.view(torch.int32), forced.view(torch.int32))
        assert torch.equal(chosen.view(torch.int32), public.view(torch.int32))
        again, _ = dw.loc._stack(env, ns, table, None, len(gx), len(gy), k_range[0], k_range[1], False, form=0)
        assert torch.equal(chosen.view(torch.int32), again.view(torch.int32))            # run to run


# ------------------------------------------------------------------------------------------
# best node and arrivals
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("container", CONTAINERS)
@pytest.mark.parametrize("nt", [1, 63, 64, 65, 3000])
@pytest.mark.parametrize("G", [1, 7, 289])
def test_best(dw, G, nt, container):
    rng = np.random.default_rng(G * 10000 + nt)
    s = rng.integers(-3, 12, (G, nt)).astype(np.float32)     # few distinct values: ties everywhere
    s[rng.random((G, nt)) < 0.1] = np.nan
    s[:, nt // 2] = np.nan                                   # a column of NaNs
    if nt > 2 and G > 2:
        s[:, 1] = 5.0                                        # all equal: node 0
        s[:, 2] = -np.inf
        s[G - 1, 2] = np.nan
    ref_v, ref_g = ks.stack_best(s)
    arg = s.reshape(17, 17, nt) if G == 289 else s
    peak, node = dw.loc.stack_best(put(arg, container))
    peak, node = host(peak, container), host(node, container)
    assert peak.dtype == np.float32 and node.dtype == np.int32
    assert np.array_equal(node, ref_g) and np.array_equal(peak, ref_v.astype(np.float32), equal_nan=True)
    assert node[nt // 2] == -1 and np.isnan(peak[nt // 2])
    if nt > 2 and G > 2:
        assert node[1] == 0 and node[2] == 0 and peak[2] == -np.inf


@pytest.mark.parametrize("container", CONTAINERS)
@pytest.mark.parametrize("kind,nch", [("line", 5), ("bent", 67), ("bent", 400)])
def test_arrivals(dw, kind, nch, container):
    sc = ks.arrivals_scene(kind, nch)
    env, fs, h, cable, pos, t0 = (sc[k] for k in ("env", "fs", "h", "cable", "pos", "t0"))
    for threshold, weights in sc["cases"]:
        ref, idx, margin = ks.arrivals(env, fs, cable, C0, pos, t0, h, threshold, weights)
        assert margin >= ks.MARGIN, margin
        got = dw.loc.arrivals_near(put(env, container), fs, put(cable, container), C0, put(pos, container), put(t0, container), h,
                                   put(threshold, container) if np.ndim(threshold) else threshold, weights=put(weights, container))
        got = host(got, container)
        assert got.dtype == np.float64 and np.array_equal(got, ref, equal_nan=True)
        assert (idx >= 0).any() and np.array_equal(got[idx >= 0], idx[idx >= 0] / fs)
    one = dw.loc.arrivals_near(env, fs, cable, C0, pos[2], t0[2], h, -1.0)
    assert one.shape == (1, nch) and np.array_equal(one[0], ks.arrivals(env, fs, cable, C0, pos[2], t0[2], h, -1.0)[0][0], equal_nan=True)


def test_argument_checks(dw):
    cable, env = make_cable("line", 5), np.ones((5, 64), dtype=np.float32)
    xs, ys = np.array([30000.0, 31000.0]), np.array([20000.0])
    base = dict(env=env, fs=50.0, cable_pos=cable, c0=C0, xs=xs, ys=ys, z=-10.0)
    for kw in (dict(fs=0.0), dict(fs=float("nan")), dict(c0=-1.0), dict(c0=float("inf")), dict(xs=np.zeros(0)), dict(k_range=(5, 5)),
               dict(k_range=(9, 2)), dict(weights=np.ones(4)), dict(env=np.ones((4, 64), dtype=np.float32)), dict(env=np.ones(64)),
               dict(delays=np.zeros((1, 2, 4), dtype=np.int32)), dict(cable_pos=np.zeros((5, 2)))):
        with pytest.raises(ValueError):
            dw.loc.stack_grid(**dict(base, **kw))
    for kw in (dict(halfwidth=-1), dict(fs=0.0), dict(pos=np.zeros((2, 2))), dict(t0=np.zeros(3)), dict(threshold=np.zeros(4))):
        a = dict(env=env, fs=50.0, cable_pos=cable, c0=C0, pos=np.zeros((2, 3)), t0=np.zeros(2), halfwidth=3, threshold=0.5)
        with pytest.raises(ValueError):
            dw.loc.arrivals_near(**dict(a, **kw))
    with pytest.raises(ValueError):
        dw.loc.locate_stack(env, 50.0, cable, C0, xs, ys, -10.0, 1.0, -1, 0.5)
    with pytest.raises(ValueError):
        dw.loc.stack_best(np.zeros((0, 4), dtype=np.float32))
    Ti, info = dw.loc.locate_stack(np.zeros((5, 64), dtype=np.float32), 50.0, cable, C0, xs, ys, -10.0, 1.0, 3, 0.5)       # no call
    assert Ti.shape == (0, 5) and info["first_guess"].shape == (0, 4) and info["node"].shape == (0,) and info["times"].shape == (64,)


# ------------------------------------------------------------------------------------------
# the known answer: three sources on nodes
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene():
    """(cable, grid, the package's delay table on the host); computed once, callers do not modify it."""
    import das4whales_amd as dw
    cable = make_cable("bent", ks.SCENE_NCH)
    xs, ys, z = ks.grid17("bent")
    return cable, (xs, ys, z), dw.loc.delay_table(cable, C0, ks.SCENE_FS, xs, ys, z)


@functools.lru_cache(maxsize=None)
def noisy_reference():
    """The noisy scene and its restatement: (env, stack, bound)."""
    _, _, d = scene()
    env = ks.triangle_scene(d, noise=0.3, seed=3)
    return (env,) + ks.stack_grid(env, d.astype(np.int64))


@pytest.mark.parametrize("container", CONTAINERS)
def test_three_sources_on_nodes(dw, container):
    cable, (xs, ys, z), d = scene()
    fs, nch = ks.SCENE_FS, ks.SCENE_NCH
    env = ks.triangle_scene(d)
    stack, times = dw.loc.stack_grid(put(env, container), fs, cable, C0, xs, ys, z)
    peak, node = dw.loc.stack_best(stack)
    stack, peak, node = host(stack, container), host(peak, container), host(node, container)
    for ix, iy, k in ks.SOURCES:
        assert stack[iy, ix, k] == 400.0 and peak[k] == 400.0 and node[k] == iy * 17 + ix
    Ti, info = dw.loc.locate_stack(put(env, container), fs, cable, C0, xs, ys, z, 200, 5, 0.5, return_stack=True)
    Ti = host(Ti, container)
    info = {k: host(v, container) for k, v in info.items()}
    want_node = np.array([iy * 17 + ix for ix, iy, _ in ks.SOURCES])
    want_col = np.array([k for _, _, k in ks.SOURCES])
    assert Ti.shape == (3, nch) and info["node"].dtype == np.int32 and info["column"].dtype == np.int32
    assert np.array_equal(info["node"], want_node) and np.array_equal(info["column"], want_col)
    assert np.array_equal(info["value"], np.full(3, 400.0, dtype=np.float32)) and info["value"].dtype == np.float32
    assert np.array_equal(info["npicks"], [nch] * 3) and info["npicks"].dtype == np.int32
    for j, (ix, iy, k) in enumerate(ks.SOURCES):
        assert np.array_equal(Ti[j], (k + d[iy, ix].astype(np.int64)) / fs)
        assert np.array_equal(info["first_guess"][j], [xs[ix], ys[iy], z, k / fs])
    assert np.array_equal(info["times"], np.arange(ks.SCENE_NS) / fs) and np.array_equal(info["times"], times if container == "numpy" else times.cpu().numpy())
    assert np.array_equal(info["stack"], stack) and np.array_equal(info["peak"], peak) and np.array_equal(info["best_node"], node)
    # the hand-off: a sanity condition, not a measurement
    n = dw.loc.solve_lq_batch(Ti, cable, C0, first_guess=info["first_guess"])
    assert np.all(np.isfinite(n))
    for j, (ix, iy, _) in enumerate(ks.SOURCES):
        assert np.hypot(n[j, 0] - xs[ix], n[j, 1] - ys[iy]) <= 1500.0
    # max_calls keeps the largest peaks, in time order: with equal values the earlier ones
    Ti2, info2 = dw.loc.locate_stack(env, fs, cable, C0, xs, ys, z, 200, 5, 0.5, max_calls=2)
    assert np.array_equal(info2["column"], want_col[:2]) and np.array_equal(Ti2, Ti[:2])


def test_dead_channels_by_weight(dw):
    cable, (xs, ys, z), d = scene()
    env = ks.triangle_scene(d, noise=0.3, seed=5)
    w = np.ones(ks.SCENE_NCH, dtype=np.float32)
    w[::3] = 0.0
    dead = env.copy()
    dead[::3] = np.nan
    got, _ = dw.loc.stack_grid(dead, ks.SCENE_FS, cable, C0, xs, ys, z, weights=w)
    ref, bound = ks.stack_grid(env, d.astype(np.int64), w)
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - ref) <= bound)
    only, _ = dw.loc.stack_grid(np.ascontiguousarray(env[w != 0]), ks.SCENE_FS, cable[w != 0], C0, xs, ys, z)
    assert np.array_equal(got.view(np.int32), only.view(np.int32))          # the same terms in the same order


def test_sources_under_noise(dw):
    cable, (xs, ys, z), d = scene()
    env, ref, bound = noisy_reference()
    peak_ref, node_ref = ks.stack_best(ref)
    found = scipy_signal.find_peaks(peak_ref, prominence=200)[0]
    Ti, info = dw.loc.locate_stack(env, ks.SCENE_FS, cable, C0, xs, ys, z, 200, 5, 0.5, return_stack=True)
    assert np.all(np.abs(info["stack"] - ref) <= bound)
    print("peaks of the restatement:", found, "nodes", node_ref[found], "; locate_stack: columns", info["column"], "nodes", info["node"],
          "npicks", info["npicks"])
    assert sorted(found) == [k for _, _, k in ks.SOURCES]
    for k in found:
        near = np.flatnonzero(np.abs(info["column"].astype(np.int64) - k) <= 1)
        assert len(near) == 1 and info["node"][near[0]] == node_ref[k]
    assert len(info["column"]) == len(found) and Ti.shape == (len(found), ks.SCENE_NCH)
