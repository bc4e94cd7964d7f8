"""Delay-and-sum stack (csrc/stack.hip) in the CPU emulator build through the C ABI, against the float64 restatement of
tests/known_answers_stack.py.  Kernel logic only, host pointers.

Delays: exact under the margin rule of known_answers_stack (the restatement's own |cable - node| fs / c0 + 0.5 is asserted to
stay 1e-9 away from every integer, then every delay must be equal).  Stack: the kernel is fed the emulator's own table, and so
is the restatement; per element |got - ref| <= 1.01 n 2^-24 sum |w env| over the n contributing terms, the bound of
recursive float32 summation (with normalize: divided by the weight sum, plus 2^-23 |ref|).  Derived, not measured.  The window
and the direct form must agree bit for bit on every case, and so must two runs.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import known_answers_stack as ks
from tests.emu_util import load_emu, vp
from tests.known_answers_loc import C0, make_cable
from tests.test_emu_assoc import small_grid

D = ctypes.c_double
I64 = ctypes.c_int64


@pytest.fixture(scope="module")
def lib():
    return load_emu()


@functools.lru_cache(maxsize=None)
def emu_delays(kind, nch, shape, fs):
    """(the emulator's table [ny x nx x nch] int32, the restatement's, its margin, xs, ys, z); shape: 1, 17, 65, "sub", "tight"."""
    lib = load_emu()
    cable = np.ascontiguousarray(make_cable(kind, nch))
    if shape == "sub":                                       # 5 x 2 nodes of grid17: two tiles, both partial
        xs, ys, z = ks.grid17(kind)
        xs, ys = xs[3:8], ys[5:7]
    elif shape == "tight":                                   # 17 x 17 nodes at 150 m
        xs, ys, z = ks.grid17(kind)
        xs, ys = xs[8] + 150.0 * (np.arange(17) - 8), ys[8] + 150.0 * (np.arange(17) - 8)
    else:
        xs, ys, z = small_grid(shape) if shape != 17 else ks.grid17(kind)
    xs, ys = np.ascontiguousarray(xs, dtype=np.float64), np.ascontiguousarray(ys, dtype=np.float64)
    got = np.full((len(ys), len(xs), nch), -7, dtype=np.int32)
    rc = lib.d4w_stack_delays_i32(vp(cable), nch, D(C0), D(fs), vp(xs), len(xs), vp(ys), len(ys), D(z), vp(got), None)
    assert rc == 0, lib.d4w_last_error()
    ref, margin = ks.delay_table(cable, C0, fs, xs, ys, z)
    got.setflags(write=False)
    return got, ref, margin, xs, ys, z


# ------------------------------------------------------------------------------------------
# the delay table
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", [50.0, 200.0])
@pytest.mark.parametrize("shape", [1, 17, 65])
@pytest.mark.parametrize("nch", [1, 5, 67, 400])
@pytest.mark.parametrize("kind", ["line", "bent"])
def test_delay_table(kind, nch, shape, fs):
    got, ref, margin, _, _, _ = emu_delays(kind, nch, shape, fs)
    assert margin >= ks.MARGIN, margin
    assert np.array_equal(got, ref)


# ------------------------------------------------------------------------------------------
# the stack
# ------------------------------------------------------------------------------------------
def emu_stack(lib, env, pitch, ns, d, weights, k_range, normalize, form, want_rc=0):
    """(stack, info).  env: the padded buffer [nch x pitch]."""
    ny, nx, nch = d.shape
    k0, k1 = (0, ns) if k_range is None else k_range
    out = np.full((ny, nx, max(k1 - k0, 1)), -7.0, dtype=np.float32)
    info = np.full(2, -7, dtype=np.int32)
    rc = lib.d4w_stack_grid_f32(vp(env), I64(pitch), nch, ns, vp(d), vp(weights) if weights is not None else None, nx, ny, k0, k1,
                                int(normalize), form, vp(out), vp(info), None)
    assert rc == want_rc, lib.d4w_last_error()
    return out, info


def padded(env, pad=5):
    """The block inside a wider buffer whose padding is NaN: (buffer, pitch)."""
    buf = np.full((env.shape[0], env.shape[1] + pad), np.nan, dtype=np.float32)
    buf[:, :env.shape[1]] = env
    return buf, env.shape[1] + pad


def weight_sets(nch, rng):
    some = rng.uniform(0.25, 2.0, nch).astype(np.float32)
    some[rng.random(nch) < 0.3] = 0.0
    if nch > 1:
        some[0], some[-1] = 0.0, 1.5
    return {"ones": None, "some": some, "zeros": np.zeros(nch, dtype=np.float32)}


def check_stack(lib, env, d, weights, k_range, normalize):
    """Both forms against the restatement and against each other; returns the window form's result."""
    nch, ns = env.shape
    e = env.copy()
    if weights is not None:
        e[weights == 0] = np.nan                             # a row under weight 0 must leave no trace
    buf, pitch = padded(e)
    ref, bound = ks.stack_grid(env, d.astype(np.int64), weights, k_range, normalize)
    win, info1 = emu_stack(lib, buf, pitch, ns, d, weights, k_range, normalize, 1)
    direct, info2 = emu_stack(lib, buf, pitch, ns, d, weights, k_range, normalize, 2)
    assert info1[0] == 1 and info2[0] == 2
    assert win.shape == ref.shape and np.all(np.isfinite(win))
    assert np.array_equal(win.view(np.int32), direct.view(np.int32))
    err = np.abs(win.astype(np.float64) - ref)
    assert np.all(err <= bound), (float((err - bound).max()), k_range, normalize)
    return win


@pytest.mark.parametrize("ns", [1, 255, 256, 257, 3000])
@pytest.mark.parametrize("nch", [1, 5, 67, 400])
def test_stack_against_the_restatement(lib, nch, ns):
    rng = np.random.default_rng(1000 * nch + ns)
    kind = "bent" if (nch + ns) % 2 else "line"
    d = emu_delays(kind, nch, "sub", 50.0)[0]
    assert ks.tile_spread(d) <= ks.WINDOW_SPREAD
    env = np.abs(rng.standard_normal((nch, ns))).astype(np.float32)
    for k_range in (None, (-300, 120), (ns - 40, ns + 500), (0, 1)):
        for name, w in weight_sets(nch, rng).items():
            got = check_stack(lib, env, d, w, k_range, False)
            if name == "zeros":
                assert np.all(got == 0)
            if name == "some":
                check_stack(lib, env, d, w, k_range, True)
    check_stack(lib, env, d, None, None, True)


def test_stack_on_the_whole_grid_and_twice(lib):
    """17 x 17 nodes (25 tiles, the last row and column partial) and more columns than one workgroup owns, run twice."""
    rng = np.random.default_rng(17)
    nch, ns = 67, 1300
    d = emu_delays("bent", nch, 17, 50.0)[0]
    env = np.abs(rng.standard_normal((nch, ns))).astype(np.float32)
    w = weight_sets(nch, rng)["some"]
    for normalize in (False, True):
        a = check_stack(lib, env, d, w, (-100, 1250), normalize)
        b = check_stack(lib, env, d, w, (-100, 1250), normalize)
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_nan_under_a_weight_propagates(lib):
    nch = 5
    d = emu_delays("line", nch, "sub", 50.0)[0]
    at = int(d[..., 2].min()) + 7                            # some nodes reach the sample from a column >= 0, some do not
    ns = at + 30
    assert d[..., 2].max() > at
    env = np.ones((nch, ns), dtype=np.float32)
    env[2, at] = np.nan
    buf, pitch = padded(env)
    for form in (1, 2):
        got, _ = emu_stack(lib, buf, pitch, ns, d, None, None, False, form)
        hit = np.zeros(got.shape, dtype=bool)
        for iy, ix in np.ndindex(d.shape[:2]):
            k = at - d[iy, ix, 2]
            if 0 <= k < ns:
                hit[iy, ix, k] = True
        assert hit.any() and np.array_equal(np.isnan(got), hit)


# ------------------------------------------------------------------------------------------
# the choice between the forms
# ------------------------------------------------------------------------------------------
def test_wide_table_takes_the_direct_form(lib):
    rng = np.random.default_rng(65)
    nch, ns = 67, 257
    d = emu_delays("bent", nch, 65, 200.0)[0]                # 65 x 5 nodes, 2900 m between the rows
    spread = ks.tile_spread(d.astype(np.int64))
    assert spread > ks.WINDOW_SPREAD
    buf, pitch = padded(np.abs(rng.standard_normal((nch, ns))).astype(np.float32))
    chosen, info = emu_stack(lib, buf, pitch, ns, d, None, (-1500, 200), False, 0)
    assert list(info) == [2, spread]
    direct, info2 = emu_stack(lib, buf, pitch, ns, d, None, (-1500, 200), False, 2)
    assert list(info2) == [2, 0] and chosen.any()
    assert np.array_equal(chosen.view(np.int32), direct.view(np.int32))
    untouched, info1 = emu_stack(lib, buf, pitch, ns, d, None, (-1500, 200), False, 1)      # the window cannot take it, and says so
    assert list(info1) == [-1, spread] and np.all(untouched == -7.0)


def test_tight_table_takes_the_window_form(lib):
    rng = np.random.default_rng(150)
    nch, ns = 67, 257
    d = emu_delays("bent", nch, "tight", 200.0)[0]           # 17 x 17 nodes at 150 m
    spread = ks.tile_spread(d.astype(np.int64))
    assert 0 < spread <= ks.WINDOW_SPREAD
    buf, pitch = padded(np.abs(rng.standard_normal((nch, ns))).astype(np.float32))
    chosen, info = emu_stack(lib, buf, pitch, ns, d, None, (-2500, 200), False, 0)
    assert list(info) == [1, spread]
    win, info1 = emu_stack(lib, buf, pitch, ns, d, None, (-2500, 200), False, 1)
    assert list(info1) == [1, spread] and chosen.any()
    assert np.array_equal(chosen.view(np.int32), win.view(np.int32))


# ------------------------------------------------------------------------------------------
# best node per column
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [1, 63, 64, 65, 3000])
@pytest.mark.parametrize("G", [1, 7, 289])
def test_best(lib, G, nt):
    rng = np.random.default_rng(G * 10000 + nt)
    s = rng.integers(-3, 12, (G, nt)).astype(np.float32)     # few distinct values: ties everywhere
    s[rng.random((G, nt)) < 0.1] = np.nan
    s[:, nt // 2] = np.nan                                   # a column of NaNs
    if nt > 2 and G > 2:
        s[:, 1] = 5.0                                        # all equal: node 0
        s[:, 2] = -np.inf
        s[G - 1, 2] = np.nan
    ref_v, ref_g = ks.stack_best(s)
    peak, node = np.full(nt, -7.0, dtype=np.float32), np.full(nt, -7, dtype=np.int32)
    assert lib.d4w_stack_best_f32(vp(s), G, nt, vp(peak), vp(node), None) == 0, lib.d4w_last_error()
    assert np.array_equal(node, ref_g) and np.array_equal(peak, ref_v.astype(np.float32), equal_nan=True)
    assert node[nt // 2] == -1 and np.isnan(peak[nt // 2])
    if nt > 2 and G > 2:
        assert node[1] == 0 and node[2] == 0 and peak[2] == -np.inf


# ------------------------------------------------------------------------------------------
# arrival times under a candidate
# ------------------------------------------------------------------------------------------
def emu_arrivals(lib, env, fs, cable, pos, t0, h, threshold, weights=None):
    nch, ns = env.shape
    buf, pitch = padded(env)
    pos, t0 = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(t0, dtype=np.float64).reshape(-1)
    cable = np.ascontiguousarray(cable, dtype=np.float64)
    Ti = np.full((len(pos), nch), 7.0)
    thr = np.ascontiguousarray(threshold, dtype=np.float64) if np.ndim(threshold) else None
    rc = lib.d4w_stack_arrivals_f64(vp(buf), I64(pitch), nch, ns, D(fs), vp(cable), D(C0), vp(pos), vp(t0), len(pos), h,
                                    D(0.0 if thr is not None else threshold), vp(thr) if thr is not None else None,
                                    vp(weights) if weights is not None else None, vp(Ti), None)
    assert rc == 0, lib.d4w_last_error()
    return Ti


@pytest.mark.parametrize("kind,nch", [("line", 5), ("bent", 67), ("bent", 400)])
def test_arrivals(lib, kind, nch):
    sc = ks.arrivals_scene(kind, nch)
    env, fs, ns, h, cable, pos, t0 = (sc[k] for k in ("env", "fs", "ns", "h", "cable", "pos", "t0"))
    for threshold, weights in sc["cases"]:
        ref, idx, margin = ks.arrivals(env, fs, cable, C0, pos, t0, h, threshold, weights)
        assert margin >= ks.MARGIN, margin
        got = emu_arrivals(lib, env, fs, cable, pos, t0, h, threshold, weights)
        assert np.array_equal(got, ref, equal_nan=True)
        assert np.array_equal(got[idx >= 0], idx[idx >= 0] / fs)
    ref, idx, _ = ks.arrivals(env, fs, cable, C0, pos, t0, h, -1.0)
    assert np.all(idx[0] < 0) and np.all(idx[5] < 0) and np.all(idx[6] < 0)              # empty windows, a NaN emission time
    assert np.all(idx[:, 0] < 0)
    if nch > 5:
        for c in (1, 4):                                     # windows cut by the record's start and by its end
            assert (idx[c] >= 0).any() and (idx[c] < 0).any()
        assert idx[1][idx[1] >= 0].min() < h and idx[4][idx[4] >= 0].max() >= ns - h


def test_arrivals_earliest_of_equal_maxima_and_halfwidth_zero(lib):
    # the position sits ON channel 1: its delay is exactly 0; fs = 4, t0 = 5 -> kc = 20
    cable = np.array([[0.0, 0.0, -100.0], [1000.0, 0.0, -100.0], [2000.0, 0.0, -100.0]])
    env = np.zeros((3, 200), dtype=np.float32)
    env[1, [17, 19, 23]] = [2.0, 3.0, 3.0]                   # equal maxima at 19 and 23: the earlier
    pos, t0 = np.array([[1000.0, 0.0, -100.0]]), np.array([5.0])
    Ti = emu_arrivals(lib, env, 4.0, cable, pos, t0, 3, 2.5)
    assert Ti[0, 1] == 19 / 4.0
    Ti = emu_arrivals(lib, env, 4.0, cable, pos, t0, 3, 3.0)     # a maximum AT the threshold is kept
    assert Ti[0, 1] == 19 / 4.0
    Ti = emu_arrivals(lib, env, 4.0, cable, pos, t0, 3, 3.5)
    assert np.isnan(Ti[0, 1])
    Ti = emu_arrivals(lib, env, 4.0, cable, pos, t0, 0, 0.0)     # half-width 0: the sample itself
    assert Ti[0, 1] == 20 / 4.0
    Ti = emu_arrivals(lib, env, 4.0, cable, pos, t0, 100, 0.0, weights=np.array([1.0, 0.0, 1.0], dtype=np.float32))
    assert np.isnan(Ti[0, 1]) and Ti[0, 0] == 0.0 and Ti[0, 2] == 0.0         # all-zero rows: the window's first sample


# ------------------------------------------------------------------------------------------
# bad arguments
# ------------------------------------------------------------------------------------------
def test_bad_arguments(lib):
    nch, ns = 5, 64
    cable = np.ascontiguousarray(make_cable("line", nch))
    xs, ys = np.array([30000.0, 31000.0]), np.array([20000.0])
    d = np.zeros((1, 2, nch), dtype=np.int32)
    env = np.ones((nch, ns), dtype=np.float32)
    out, info = np.zeros((1, 2, ns), dtype=np.float32), np.zeros(2, dtype=np.int32)
    nan, inf = float("nan"), float("inf")

    def p(a):
        return vp(a) if a is not None else None

    def delays(nch=nch, nx=2, ny=1, fs=50.0, c0=C0, cab=cable, gx=xs, gy=ys, o=d, z=-60.0):
        return lib.d4w_stack_delays_i32(p(cab), nch, D(c0), D(fs), p(gx), nx, p(gy), ny, D(z), p(o), None)
    assert delays() == 0
    for kw in (dict(nch=0), dict(nx=0), dict(ny=0), dict(fs=0.0), dict(fs=nan), dict(fs=inf), dict(c0=0.0), dict(c0=-C0), dict(c0=nan),
               dict(cab=None), dict(gx=None), dict(gy=None), dict(o=None), dict(z=nan)):
        assert delays(**kw) == -1, kw
        assert len(lib.d4w_last_error()) > 0

    def grid(e=env, pitch=ns, nch=nch, ns=ns, t=d, nx=2, ny=1, k0=0, k1=ns, form=0, o=out, i=info):
        return lib.d4w_stack_grid_f32(p(e), I64(pitch), nch, ns, p(t), None, nx, ny, k0, k1, 0, form, p(o), p(i), None)
    assert grid() == 0 and grid(form=2, i=None) == 0
    for kw in (dict(e=None), dict(t=None), dict(o=None), dict(nch=0), dict(ns=0), dict(pitch=ns - 1), dict(nx=0), dict(ny=0), dict(k0=5, k1=5),
               dict(k0=6, k1=5), dict(form=3), dict(form=-1), dict(form=0, i=None), dict(form=1, i=None), dict(k1=(1 << 30) + 1), dict(k0=-(1 << 30) - 1),
               dict(k0=-(1 << 30), k1=1 << 30)):            # 2^31 columns: one more than an int holds
        assert grid(**kw) == -1, kw
        assert len(lib.d4w_last_error()) > 0

    peak, node = np.zeros(ns, dtype=np.float32), np.zeros(ns, dtype=np.int32)
    assert lib.d4w_stack_best_f32(vp(out), 2, ns, vp(peak), vp(node), None) == 0
    for args in ((None, 2, ns, vp(peak), vp(node)), (vp(out), 0, ns, vp(peak), vp(node)), (vp(out), 2, 0, vp(peak), vp(node)),
                 (vp(out), 2, ns, None, vp(node)), (vp(out), 2, ns, vp(peak), None)):
        assert lib.d4w_stack_best_f32(*args, None) == -1, args

    pos, t0, Ti = np.array([[30000.0, 20000.0, -60.0]]), np.array([0.1]), np.zeros((1, nch))

    def arr(e=env, pitch=ns, nch=nch, ns=ns, fs=50.0, c0=C0, cab=cable, ps=pos, t=t0, n=1, h=3, o=Ti):
        return lib.d4w_stack_arrivals_f64(p(e), I64(pitch), nch, ns, D(fs), p(cab), D(c0), p(ps), p(t), n, h, D(0.5), None, None, p(o), None)
    assert arr() == 0
    for kw in (dict(e=None), dict(cab=None), dict(ps=None), dict(t=None), dict(o=None), dict(nch=0), dict(ns=0), dict(pitch=ns - 1), dict(n=0),
               dict(h=-1), dict(fs=0.0), dict(fs=nan), dict(c0=0.0), dict(c0=inf)):
        assert arr(**kw) == -1, kw
