"""float64 NumPy restatement of csrc/stack.hip (delay-and-sum stack of envelopes on the position grid), and the scene its
tests share.  Cables: tests/known_answers_loc.make_cable; grid: tests/known_answers_assoc.grid17.

Definitions, for nodes g = iy nx + ix at (xs[ix], ys[iy], z):
    d[g][ch] = floor(|cable[ch] - node_g| fs / c0 + 0.5)
    stack[g][k - k0] = sum over ch of w[ch] env[ch][k + d[g][ch]], over the channels with w[ch] != 0 and 0 <= k + d < ns
    normalize: divided by the sum of the contributing w[ch]; an element without contributors is 0
    best: per column the largest value over the nodes and the smallest node that has it; NaNs never win; all NaN: (NaN, -1)
    arrivals: kc = floor(t0 fs + 0.5), m = kc + d(pos, ch); the largest env[ch][i] over i in [m - h, m + h] and [0, ns), the
      earliest of equals, NaNs skipped; Ti = i / fs, NaN for an empty window, w[ch] = 0 or a maximum below the threshold
Margin rule (as in known_answers_assoc): the kernels multiply by 1 / c0 where this file divides, so the argument of the floor
differs by a few ulp; `delay_table` and `arrivals` also return the smallest distance of |cable - node| fs / c0 + 0.5 to an
integer, a comparing test first asserts it to be at least MARGIN = 1e-9 and then demands exactly equal delays.  On both
cables with 5, 67 and 400 channels, grid17 and fs = 50 that distance lies between 2e-6 and 5e-4: nothing is excluded.
"""
import numpy as np

from tests.known_answers_assoc import grid17                # noqa: F401  (the tests take it from here)
from tests.known_answers_loc import C0, make_cable          # noqa: F401

MARGIN = 1e-9
TILE = 4                 # the kernel's tile of nodes is TILE x TILE (kStackTX, kStackTY)
WINDOW_SPREAD = 992      # the largest delay spread within a tile that the window form takes (kStackSpread)


def _q(cable, c0, fs, px, py, pz):
    cable = np.asarray(cable, dtype=np.float64)
    dist = np.sqrt((cable[:, 0] - px) ** 2 + (cable[:, 1] - py) ** 2 + (cable[:, 2] - pz) ** 2)
    return dist * fs / c0 + 0.5


def delay_table(cable, c0, fs, xs, ys, z):
    """(d [ny x nx x nch] int64, margin)."""
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    q = np.stack([np.stack([_q(cable, c0, fs, x, y, z) for x in xs]) for y in ys])
    return np.floor(q).astype(np.int64), float(np.min(np.abs(q - np.round(q))))


def tile_spread(d):
    """The largest max - min of the delays over a TILE x TILE tile of nodes, over all tiles and channels."""
    ny, nx, _ = d.shape
    m = 0
    for iy in range(0, ny, TILE):
        for ix in range(0, nx, TILE):
            t = d[iy:iy + TILE, ix:ix + TILE].reshape(-1, d.shape[2])
            m = max(m, int((t.max(0) - t.min(0)).max()))
    return m


def stack_grid(env, d, weights=None, k_range=None, normalize=False):
    """(stack [ny x nx x nt] float64, bound [ny x nx x nt]): the sum over the channels in float64, and the bound for a
    recursive float32 summation of the same n terms, 1.01 n 2^-24 sum |w env| (with normalize: divided by the weight sum,
    plus 2^-23 |stack| for the division and the rounding of the weight sum)."""
    env = np.asarray(env)
    nch, ns = env.shape
    ny, nx, _ = d.shape
    G = ny * nx
    k0, k1 = (0, ns) if k_range is None else k_range
    nt = k1 - k0
    w = np.ones(nch) if weights is None else np.asarray(weights, dtype=np.float64)
    dd = np.asarray(d, dtype=np.int64).reshape(G, nch)
    A, B = np.maximum(k0, -dd), np.minimum(k1, ns - dd)      # channel ch reaches node g from the columns A <= k < B
    ok = (A < B) & (w != 0)[None, :]
    gi, ci = np.nonzero(ok)
    cnt, wsum = np.zeros((G, nt + 1)), np.zeros((G, nt + 1))
    np.add.at(cnt, (gi, A[ok] - k0), 1.0)
    np.add.at(cnt, (gi, B[ok] - k0), -1.0)
    np.add.at(wsum, (gi, A[ok] - k0), w[ci])
    np.add.at(wsum, (gi, B[ok] - k0), -w[ci])
    cnt = np.cumsum(cnt, axis=1)[:, :nt]
    wsum = np.where(cnt > 0, np.cumsum(wsum, axis=1)[:, :nt], 0.0)
    live = np.flatnonzero(w != 0)
    e64 = env[live].astype(np.float64) * w[live][:, None]    # rows of weight 0 are never looked at
    signed = bool((e64 < 0).any())
    s = np.zeros((G, nt))
    sabs = np.zeros((G, nt)) if signed else s
    for j, ch in enumerate(live):
        row, arow = e64[j], np.abs(e64[j])
        for g in np.flatnonzero(ok[:, ch]):
            a, b, dl = A[g, ch], B[g, ch], dd[g, ch]
            s[g, a - k0:b - k0] += row[a + dl:b + dl]
            if signed:
                sabs[g, a - k0:b - k0] += arow[a + dl:b + dl]
    bound = 1.01 * cnt * 2.0 ** -24 * sabs
    if normalize:
        with np.errstate(all="ignore"):
            bound = np.where(wsum != 0, bound / np.abs(wsum), 0.0)
            s = np.where(wsum != 0, s / wsum, 0.0)
            bound = bound + 2.0 ** -23 * np.abs(s)
    return s.reshape(ny, nx, nt), bound.reshape(ny, nx, nt)


def stack_best(stack):
    """(peak [nt], node [nt] int64) of a stack [.. x nt]."""
    s = np.asarray(stack, dtype=np.float64).reshape(-1, np.shape(stack)[-1])
    allnan = np.all(np.isnan(s), axis=0)
    node = np.argmax(np.where(np.isnan(s), -np.inf, s), axis=0)          # the first occurrence: the smallest node
    peak = s[node, np.arange(s.shape[1])]
    return np.where(allnan, np.nan, peak), np.where(allnan, -1, node)


def arrivals(env, fs, cable, c0, pos, t0, h, threshold, weights=None):
    """(Ti [ncalls x nch], sample index or -1 [ncalls x nch], margin)."""
    env = np.asarray(env)
    nch, ns = env.shape
    pos, t0 = np.asarray(pos, dtype=np.float64).reshape(-1, 3), np.asarray(t0, dtype=np.float64).reshape(-1)
    w = np.ones(nch) if weights is None else np.asarray(weights, dtype=np.float64)
    thr = np.broadcast_to(np.asarray(threshold, dtype=np.float64), (nch,))
    Ti, idx, margin = np.full((len(pos), nch), np.nan), np.full((len(pos), nch), -1, dtype=np.int64), 0.5
    for c in range(len(pos)):
        q = _q(cable, c0, fs, *pos[c])
        margin = min(margin, float(np.min(np.abs(q - np.round(q)))))
        if not np.isfinite(t0[c]):
            continue
        m = int(np.floor(t0[c] * fs + 0.5)) + np.floor(q).astype(np.int64)
        for ch in range(nch):
            a, b = max(m[ch] - h, 0), min(m[ch] + h, ns - 1)
            if w[ch] == 0 or a > b:
                continue
            win = env[ch, a:b + 1].astype(np.float64)
            if np.all(np.isnan(win)):
                continue
            j = int(np.nanargmax(win))                                   # the first occurrence: the earliest
            if win[j] < thr[ch]:
                continue
            idx[c, ch] = a + j
            Ti[c, ch] = (a + j) / fs
    return Ti, idx, margin


def arrivals_scene(kind, nch):
    """A block of few distinct values (equal maxima in every window) with NaN samples and a NaN channel, and seven calls
    whose windows lie before the record, astride its start, inside it, astride its end, behind it, and one emitted at NaN.
    Returns dict(env, fs, ns, h, cable, pos, t0, cases = [(threshold, weights)])."""
    rng = np.random.default_rng(nch)
    fs, ns, h = 50.0, 1500, 40
    cable = make_cable(kind, nch)
    xs, ys, z = grid17(kind)
    env = rng.integers(0, 6, (nch, ns)).astype(np.float32)
    env[rng.random((nch, ns)) < 0.05] = np.nan
    env[0, :] = np.nan
    pos = np.array([[xs[8], ys[8], z], [xs[2], ys[12], z], [xs[15], ys[3], z - 20.0], [xs[8], ys[8], z], [xs[0], ys[0], z],
                    [xs[5], ys[5], z], [xs[5], ys[5], z]])
    t0 = np.array([-40.0, -8.03, 3.21, 10.0, 20.0, 200.0, np.nan])
    w = rng.uniform(0.5, 1.5, nch).astype(np.float32)
    w[rng.random(nch) < 0.3] = 0.0
    thr_ch = rng.integers(3, 7, nch).astype(np.float64)
    return dict(env=env, fs=fs, ns=ns, h=h, cable=cable, pos=pos, t0=t0,
                cases=[(4.0, None), (5.0, w), (thr_ch, None), (thr_ch, w), (-1.0, None)])


# ------------------------------------------------------------------------------------------
# the scene of the known answer: three sources ON nodes of grid17, triangles of unit height along their moveouts
# ------------------------------------------------------------------------------------------
SOURCES = ((11, 4, 500), (3, 9, 1200), (6, 13, 1900))        # (ix, iy, emission sample k)
SCENE_FS, SCENE_NS, SCENE_NCH, SCENE_HALF = 50.0, 3000, 400, 20


def triangle_scene(d, noise=0.0, seed=0):
    """env [400 x 3000] float32 for the delay table d [17 x 17 x 400]: zero except, per source and channel, a triangle of
    half-width 20 samples and peak exactly 1.0 at k + d[iy, ix, ch]; plus |N(0, noise)| when noise > 0."""
    env = np.zeros((SCENE_NCH, SCENE_NS), dtype=np.float32)
    tri = (1.0 - np.abs(np.arange(-SCENE_HALF, SCENE_HALF + 1)) / SCENE_HALF).astype(np.float32)
    for ix, iy, k in SOURCES:
        for ch in range(SCENE_NCH):
            c = k + int(d[iy, ix, ch])
            assert SCENE_HALF <= c < SCENE_NS - SCENE_HALF
            seg = env[ch, c - SCENE_HALF:c + SCENE_HALF + 1]
            np.maximum(seg, tri, out=seg)
    if noise > 0:
        env += np.abs(np.random.default_rng(seed).normal(0.0, noise, env.shape)).astype(np.float32)
    return env
