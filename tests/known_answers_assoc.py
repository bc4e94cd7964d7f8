"""float64 NumPy restatement of csrc/assoc.hip (delay-and-vote association of picks into calls), and the synthetic scenes
its tests share.  The cables are those of tests/known_answers_loc.make_cable.

Definitions, for picks k (channel ch_k, sample i_k, t_k = i_k / fs, ordered by (channel, sample)) and nodes g = iy nx + ix
at (xs[ix], ys[iy], z):
    e_kg = t_k - |cable[ch_k] - node_g| / c0          bin(k, g) = floor((e_kg - lo) / dt)
    votes[g][b] = #{k : bin(k, g) = b}, 0 <= b < nbins
    score s[g][b] = votes[g][b] + votes[g][b + 1], 0 <= b < nbins - 1
`associate` is the greedy loop written out literally.  `margin` is the smallest |q - round(q)| over all (pick, node) pairs
with q = (e - lo) / dt: the kernels multiply by reciprocals where this file divides, so q differs by a few ulp (about 1e-11
at |e| <= 100 s and dt >= 0.01 s), and a comparison is exact -- every count and every choice -- whenever margin >= 1e-9.
The comparing tests assert that margin on this file's numbers first and then demand equality; no pair is excluded.
"""
import itertools

import numpy as np

from tests.known_answers_loc import C0, make_cable

MARGIN = 1e-9
FS = 200.0


def sort_table(table):
    """(table ordered by (channel, sample), order): stable, so equal picks keep the caller's order."""
    table = np.asarray(table, dtype=np.int64)
    order = np.lexsort((table[1], table[0]))
    return table[:, order], order


def emission(table, fs, cable, c0, xs, ys, z):
    """e [K x G], node g = iy nx + ix."""
    t = table[1] / fs
    c = np.asarray(cable, dtype=np.float64)[table[0]]
    X, Y = np.tile(np.asarray(xs, dtype=np.float64), len(ys)), np.repeat(np.asarray(ys, dtype=np.float64), len(xs))
    d = np.sqrt((c[:, 0][:, None] - X[None, :]) ** 2 + (c[:, 1][:, None] - Y[None, :]) ** 2 + (c[:, 2][:, None] - z) ** 2)
    return t[:, None] - d / c0


def default_range(table, fs, cable, c0, xs, ys, z):
    """(lo, hi) = (min t - Dmax / c0, max t); Dmax over the 8 corners of the cable's bounding box x the 4 corners of the grid."""
    c, xs, ys = np.asarray(cable, dtype=np.float64), np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    dmax = 0.0
    for cx, cy, cz, px, py in itertools.product((c[:, 0].min(), c[:, 0].max()), (c[:, 1].min(), c[:, 1].max()),
                                                (c[:, 2].min(), c[:, 2].max()), (xs.min(), xs.max()), (ys.min(), ys.max())):
        dmax = max(dmax, float(np.sqrt((cx - px) ** 2 + (cy - py) ** 2 + (cz - z) ** 2)))
    imin, imax = (int(table[1].min()), int(table[1].max())) if table.shape[1] else (0, 0)
    return imin / fs - dmax / c0, imax / fs


def bin_layout(table, fs, cable, c0, xs, ys, z, dt, t0_range=None, layout=None):
    """(lo, nbins, edges); layout = (lo, nbins) states them directly."""
    if layout is not None:
        return layout[0], int(layout[1]), layout[0] + dt * np.arange(int(layout[1]) + 1)
    lo, hi = default_range(table, fs, cable, c0, xs, ys, z) if t0_range is None else (float(t0_range[0]), float(t0_range[1]))
    nbins = int(np.ceil((hi - lo) / dt)) + 1
    return lo, nbins, lo + dt * np.arange(nbins + 1)


def bins_and_margin(e, lo, dt):
    """(bin [K x G] int64, the smallest |q - round(q)| over all pairs; 0.5 without pairs)."""
    q = (e - lo) / dt
    return np.floor(q).astype(np.int64), (float(np.min(np.abs(q - np.round(q)))) if q.size else 0.5)


def count_votes(b, nbins, keep=None):
    """votes [G x nbins] of the bins b [K x G] over the picks keep (a boolean mask; None = all)."""
    G = b.shape[1]
    votes = np.zeros((G, nbins), dtype=np.int64)
    if keep is not None:
        b = b[keep]
    for g in range(G):
        col = b[:, g]
        col = col[(col >= 0) & (col < nbins)]
        votes[g] = np.bincount(col, minlength=nbins)
    return votes


def vote(table, fs, cable, c0, xs, ys, z, dt, t0_range=None, layout=None):
    """(votes [ny x nx x nbins], edges, margin)."""
    lo, nbins, edges = bin_layout(table, fs, cable, c0, xs, ys, z, dt, t0_range, layout)
    b, m = bins_and_margin(emission(table, fs, cable, c0, xs, ys, z), lo, dt)
    return count_votes(b, nbins).reshape(len(ys), len(xs), nbins), edges, m


def margin(table, fs, cable, c0, xs, ys, z, dt, t0_range=None):
    lo, _, _ = bin_layout(table, fs, cable, c0, xs, ys, z, dt, t0_range)
    return bins_and_margin(emission(table, fs, cable, c0, xs, ys, z), lo, dt)[1]


def associate(table, fs, cable, c0, xs, ys, z, dt, min_picks, max_calls=64, t0_range=None):
    """The greedy loop.  Returns (Ti [ncalls x nch], info) with info = first_guess, node, bin, score, npicks, assigned, edges,
    votes (the accumulator after the last round, [ny x nx x nbins]), margin, emax (largest |e| of a chosen pick)."""
    table = np.asarray(table, dtype=np.int64)
    nch, K, nx = len(cable), table.shape[1], len(xs)
    lo, nbins, edges = bin_layout(table, fs, cable, c0, xs, ys, z, dt, t0_range)
    e = emission(table, fs, cable, c0, xs, ys, z)
    b, m = bins_and_margin(e, lo, dt)
    t = table[1] / fs
    votes = count_votes(b, nbins)
    assigned = np.zeros(K, dtype=np.int64)
    Ti, fg, node, bin_, score, npicks, emax = [], [], [], [], [], [], 0.0
    for c in range(max_calls if K else 0):
        s = votes[:, :-1] + votes[:, 1:]
        flat = int(np.argmax(s))                             # the first occurrence: the smallest flat index
        g, bs = divmod(flat, nbins - 1)
        if s[g, bs] < min_picks:
            break
        ec = lo + (bs + 1) * dt
        row, chosen = np.full(nch, np.nan), []
        cand = np.flatnonzero((assigned == 0) & ((b[:, g] == bs) | (b[:, g] == bs + 1)))
        for ch in np.unique(table[0][cand]):
            ks = cand[table[0][cand] == ch]                  # ascending k
            k = ks[np.argmin(np.abs(e[ks, g] - ec))]         # the first minimum: ties go to the smaller k
            row[ch] = t[k]
            chosen.append(k)
        chosen = np.asarray(chosen, dtype=np.int64)
        assigned[chosen] = c + 1
        for k in chosen:                                     # the vote with weight -1 over the chosen picks, every node
            ok = (b[k] >= 0) & (b[k] < nbins)
            np.subtract.at(votes, (np.flatnonzero(ok), b[k][ok]), 1)
        Ti.append(row)
        node.append(g)
        bin_.append(bs)
        score.append(int(s[g, bs]))
        npicks.append(len(chosen))
        fg.append([xs[g % nx], ys[g // nx], z, float(np.mean(e[chosen, g]))])
        emax = max(emax, float(np.abs(e[chosen, g]).max()))
    info = {"first_guess": np.asarray(fg, dtype=np.float64).reshape(-1, 4), "node": np.asarray(node, dtype=np.int64),
            "bin": np.asarray(bin_, dtype=np.int64), "score": np.asarray(score, dtype=np.int64),
            "npicks": np.asarray(npicks, dtype=np.int64), "assigned": assigned, "edges": edges,
            "votes": votes.reshape(len(ys), len(xs), nbins), "margin": m, "emax": emax}
    return np.asarray(Ti, dtype=np.float64).reshape(-1, nch), info


# ------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------
def grid17(kind):
    """17 x 17 nodes at 1500 m around the cable's middle, depth -60 m."""
    cx, cy = (42000.0, 27000.0) if kind == "line" else (38000.0, 23000.0)
    return cx + 1500.0 * (np.arange(17) - 8), cy + 1500.0 * (np.arange(17) - 8), -60.0


def scene(kind, nch, seed, nclutter=600, nsrc=3, jitter=0.004, keep=0.7, duration=60.0, fs=FS):
    """(cable, table ordered by (channel, sample), sources [nsrc x 4]): nsrc sources off the nodes of grid17 emitting at
    spread-out times, each picked on `keep` of the channels with `jitter` seconds (standard deviation) of pick error, plus
    nclutter picks uniform over channels and the duration."""
    rng = np.random.default_rng(seed)
    cable = make_cable(kind, nch)
    xs, ys, z = grid17(kind)
    rows = []
    srcs = np.empty((nsrc, 4))
    for j in range(nsrc):
        srcs[j] = [rng.uniform(xs[2], xs[-3]), rng.uniform(ys[2], ys[-3]), z, 8.0 + 14.0 * j + rng.uniform(0.0, 3.0)]
        chans = np.flatnonzero(rng.random(nch) < keep)
        arr = srcs[j, 3] + np.sqrt(((cable[chans] - srcs[j, :3]) ** 2).sum(1)) / C0 + jitter * rng.standard_normal(len(chans))
        rows.append(np.stack([chans, np.round(arr * fs).astype(np.int64)]))
    rows.append(np.stack([rng.integers(0, nch, nclutter), rng.integers(0, int(duration * fs), nclutter)]))
    table, _ = sort_table(np.concatenate(rows, axis=1))
    return cable, table, srcs
