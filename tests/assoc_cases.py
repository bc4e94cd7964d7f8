"""The cases tests/test_emu_assoc_shapes.py (CPU emulator build, host pointers) and tests/test_assoc_shapes_gpu.py (gfx950)
both run against tests/known_answers_assoc.py: the grids, bin counts, ties and duplicates at which csrc/assoc.hip takes the
paths that the 17 x 17 grid with 170 to 260 bins never reaches.  NumPy only.

A case is named "<family>" or "<family>-<seed>"; case(name) returns (cable, table, xs, ys, z, params, t0_range) with
params = dt, min_picks, max_calls and t0_range None for the default range.  reference(name) is the restatement's answer,
computed once and left unchanged.  check_structure(name) asserts, on the restatement's own numbers, the margin rule of
known_answers_assoc (no (pick, node) pair within 1e-9 of a bin edge) and the conditions that keep the case on the path it
was written for; a test calls it before it looks at what the kernels gave.  Nothing is skipped when a condition fails:
the seed has to change.  compare(name, Ti, info) then demands equality with the restatement.
"""
import functools

import numpy as np

from tests import known_answers_assoc as ka
from tests.known_answers_loc import C0, make_cable

FS = ka.FS
EPS = np.finfo(np.float64).eps
LDS_BINS = 1024          # bins per node of the vote's LDS histogram tile (kAssocBins)
TILE_NODES = 8           # nodes per workgroup of the vote (kAssocNodes)
ONE_PASS_NODES = 4096    # the arg-max's first stage visits every node row once up to this count (kAssocParts x kAssocWaves)

NAMES = ("rect_17x5_fine-31", "rect_17x5_fine-32", "rect_17x5_fine-33", "rect_3x17_finer-32", "rect_3x17_finer-33",
         "column_1x9-31", "column_1x9-32", "column_1x9-33", "row_9x1-31", "big_70x61-41", "big_70x61-42", "big_on_nodes",
         "straddle_1024", "crowded_windows", "minimal")

BIG_XS, BIG_YS, BIG_Z = 26000.0 + 350.0 * np.arange(70), 14000.0 + 300.0 * np.arange(61), -60.0
BIG_SOURCES = ((11, 4, 50.25), (60, 59, 10.25), (33, 30, 90.25))                  # (ix, iy, t0)
STRADDLE_SOURCES = ((9, 1, 1024 * 0.05 + 0.0003), (2, 3, 2048 * 0.05 - 0.0004), (5, 4, 20.013))


def on_node_rows(cable, xs, ys, z, sources, fs=FS):
    """Per source (ix, iy, t0) a [2 x nch] block of picks round(arrival fs) on every channel."""
    rows = []
    for ix, iy, t0 in sources:
        arr = t0 + np.sqrt(((cable - [xs[ix], ys[iy], z]) ** 2).sum(1)) / C0
        rows.append(np.stack([np.arange(len(cable)), np.round(arr * fs).astype(np.int64)]))
    return rows


def straddle_grid():
    xs, ys, z = ka.grid17("bent")
    return xs[2:15], ys[6:11], z


def crowded_table():
    """The picks of straddle_1024 and, per source on a fifth of the channels, a second pick one sample beside the
    source's; on every second of those channels the source's pick once more (an exact tie in |e - ec|)."""
    cable = make_cable("bent", 400)
    xs, ys, z = straddle_grid()
    rows = on_node_rows(cable, xs, ys, z, STRADDLE_SOURCES)
    rng = np.random.default_rng(77)
    for r in list(rows):
        chans = np.sort(rng.choice(400, 80, replace=False))
        rows.append(np.stack([chans, r[1][chans] + rng.choice([-1, 1], 80)]))
        rows.append(np.stack([chans[::2], r[1][chans[::2]]]))
    return ka.sort_table(np.concatenate(rows, axis=1))[0]


@functools.lru_cache(maxsize=None)
def case(name):
    """(cable, table, xs, ys, z, params, t0_range); the arrays are shared, callers do not modify them."""
    family, _, seed = name.partition("-")
    seed = int(seed) if seed else None
    t0_range = None
    if family == "rect_17x5_fine":
        cable, table, _ = ka.scene("bent", 400, seed, nclutter=600)
        xs, ys, z = ka.grid17("bent")
        ys = ys[5:10]
        params = dict(dt=0.05, min_picks=40, max_calls=8)
    elif family == "rect_3x17_finer":
        cable, table, _ = ka.scene("bent", 400, seed, nclutter=600)
        xs, ys, z = ka.grid17("bent")
        xs = xs[6:9]
        params = dict(dt=0.02, min_picks=30, max_calls=8)
    elif family in ("column_1x9", "row_9x1"):
        cable, table, _ = ka.scene("line", 67, seed, nclutter=100)
        xs, ys, z = ka.grid17("line")
        xs, ys = (xs[4:5], ys[4:13]) if family == "column_1x9" else (xs[4:13], ys[4:5])
        params = dict(dt=0.5, min_picks=20, max_calls=8)
    elif family == "big_70x61":
        cable, table, _ = ka.scene("bent", 400, seed, 600)
        xs, ys, z = BIG_XS, BIG_YS, BIG_Z
        params = dict(dt=0.5, min_picks=60, max_calls=8)
    elif family == "big_on_nodes":
        cable = make_cable("bent", 400)
        xs, ys, z = BIG_XS, BIG_YS, BIG_Z
        table, _ = ka.sort_table(np.concatenate(on_node_rows(cable, xs, ys, z, BIG_SOURCES), axis=1))
        params, t0_range = dict(dt=0.5, min_picks=60, max_calls=8), (0.0, 130.0)
    elif family == "straddle_1024":
        cable = make_cable("bent", 400)
        xs, ys, z = straddle_grid()
        table, _ = ka.sort_table(np.concatenate(on_node_rows(cable, xs, ys, z, STRADDLE_SOURCES), axis=1))
        params, t0_range = dict(dt=0.05, min_picks=60, max_calls=8), (0.0, 130.0)
    elif family == "crowded_windows":
        cable = make_cable("bent", 400)
        xs, ys, z = straddle_grid()
        table = crowded_table()
        params, t0_range = dict(dt=0.05, min_picks=60, max_calls=8), (0.0, 130.0)
    elif family == "minimal":
        cable = np.array([[30000.0, 20000.0, -100.0]])
        xs, ys, z = np.array([33000.0]), np.array([24000.0]), -60.0
        table = np.array([[0], [2000]], dtype=np.int64)
        e = float(ka.emission(table, FS, cable, C0, xs, ys, z)[0, 0])
        params, t0_range = dict(dt=0.5, min_picks=1, max_calls=8), (e - 0.15, e + 0.15)      # ceil(0.6) + 1 = 2 bins, q = 0.3
    else:
        raise KeyError(name)
    xs, ys = np.ascontiguousarray(xs, dtype=np.float64), np.ascontiguousarray(ys, dtype=np.float64)
    return cable, table, xs, ys, float(z), params, t0_range


def layout(name):
    """(lo, nbins) of the case, from the restatement."""
    cable, table, xs, ys, z, params, t0_range = case(name)
    lo, nbins, _ = ka.bin_layout(table, FS, cable, C0, xs, ys, z, params["dt"], t0_range)
    return lo, nbins


def range_of(name):
    """The case's t0_range spelled out: what a second call needs to land on the same bins with fewer picks."""
    cable, table, xs, ys, z, params, t0_range = case(name)
    return ka.default_range(table, FS, cable, C0, xs, ys, z) if t0_range is None else t0_range


@functools.lru_cache(maxsize=None)
def reference(name):
    """{"Ti", "info", "votes", "edges"}: ka.associate and ka.vote of the case, computed once; callers do not modify it."""
    cable, table, xs, ys, z, params, t0_range = case(name)
    Ti, info = ka.associate(table, FS, cable, C0, xs, ys, z, t0_range=t0_range, **params)
    votes, edges, m = ka.vote(table, FS, cable, C0, xs, ys, z, params["dt"], t0_range)
    assert m == info["margin"] and np.array_equal(edges, info["edges"])
    for a in [Ti, votes] + [v for v in info.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return {"Ti": Ti, "info": info, "votes": votes, "edges": edges}


def left_over(name, assigned, max_calls=None):
    """The restatement's vote of the picks with assigned == 0 on the case's layout (with max_calls: assigned > max_calls
    counts as unassigned too), with that vote's margin."""
    cable, table, xs, ys, z, params, _ = case(name)
    keep = (assigned == 0) if max_calls is None else ((assigned == 0) | (assigned > max_calls))
    votes, _, m = ka.vote(table[:, keep], FS, cable, C0, xs, ys, z, params["dt"], layout=layout(name))
    return votes, m


def index_list(name, seed=8):
    """(idx [nch] int32, keep [K] bool) for a subtract pass at the case's layout: per channel one of its picks, -1 on the
    channels without picks and on a random third of the others; keep marks the picks the list leaves in the vote."""
    cable, table, _, _, _, _, _ = case(name)
    nch = len(cable)
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(np.bincount(table[0], minlength=nch))])
    idx = np.full(nch, -1, dtype=np.int32)
    for ch in range(nch):
        if off[ch + 1] > off[ch] and rng.random() >= 1.0 / 3.0:
            idx[ch] = rng.integers(off[ch], off[ch + 1])
    keep = np.ones(table.shape[1], dtype=bool)
    keep[idx[idx >= 0]] = False
    return idx, keep


def picker_scene(nrows=390, nch=400, ns=2400, fs=40.0):
    """Unit spikes along the moveouts of two sources on nodes of grid17("bent"), on the first nrows channels of the nch-channel
    bent cable: (cable, xs, ys, z, fs, ns, samples [2 x nrows] int64, one row per source in the order of emission)."""
    cable = make_cable("bent", nch)
    xs, ys, z = ka.grid17("bent")
    rows = on_node_rows(cable, xs, ys, z, ((5, 6, 5.0), (12, 10, 30.0)), fs=fs)
    samples = np.stack([r[1][:nrows] for r in rows])
    assert samples.min() >= 0 and samples.max() < ns - 1 and np.all(np.abs(samples[0] - samples[1]) > 2)
    return cable, xs, ys, z, fs, ns, samples


def describe(name):
    """One line of figures: what the summary of a run quotes."""
    cable, table, xs, ys, z, params, _ = case(name)
    info = reference(name)["info"]
    return "%s: grid %d x %d (G = %d) nbins %d picks %d calls %d nodes %s bins %s scores %s margin %.3e" % (
        name, len(ys), len(xs), len(xs) * len(ys), len(info["edges"]) - 1, table.shape[1], len(info["node"]), info["node"].tolist(),
        info["bin"].tolist(), info["score"].tolist(), info["margin"])


def check_structure(name):
    """The margin rule and the case's structure conditions, on the restatement alone."""
    cable, table, xs, ys, z, params, t0_range = case(name)
    ref = reference(name)
    info, votes = ref["info"], ref["votes"]
    family = name.partition("-")[0]
    nx, ny, nbins, ncalls = len(xs), len(ys), len(info["edges"]) - 1, len(info["node"])
    G = nx * ny
    print(describe(name))
    assert info["margin"] >= ka.MARGIN, info["margin"]
    assert left_over(name, info["assigned"])[1] >= ka.MARGIN
    v = votes.reshape(G, nbins)
    if family == "rect_17x5_fine":
        assert (nx, ny) == (17, 5) and G % TILE_NODES == 5                  # the last tile of the vote holds 5 nodes
        assert LDS_BINS < nbins < 2 * LDS_BINS and ncalls >= 3
        assert (info["bin"] < LDS_BINS - 1).any() and (info["bin"] > LDS_BINS).any()
    elif family == "rect_3x17_finer":
        assert (nx, ny) == (3, 17) and nbins > 3 * LDS_BINS and ncalls >= 3
    elif family == "column_1x9":
        assert (nx, ny) == (1, 9) and ncalls >= 2
    elif family == "row_9x1":
        assert (nx, ny) == (9, 1) and ncalls >= 2
    elif family == "big_70x61":
        assert (nx, ny) == (70, 61) and G > ONE_PASS_NODES and ncalls >= 3
    elif family == "big_on_nodes":
        assert G > ONE_PASS_NODES and ncalls == 3 and np.all(info["score"] == info["score"][0])
        flat = info["node"] * (nbins - 1) + info["bin"]
        assert np.all(np.diff(flat) > 0)                                    # equal scores come in increasing flat index
        assert (info["node"] >= ONE_PASS_NODES).any() and (info["node"] < ONE_PASS_NODES).any()
    elif family in ("straddle_1024", "crowded_windows"):
        assert 2 * LDS_BINS < nbins < 3 * LDS_BINS
        for edge in (LDS_BINS - 1, 2 * LDS_BINS - 1):                       # a window written by two workgroups of the vote
            c = np.flatnonzero(info["bin"] == edge)
            assert len(c) >= 1, edge
            g = info["node"][c[0]]
            assert v[g, edge] > 0 and v[g, edge + 1] > 0
        if family == "straddle_1024":
            assert ncalls == 3 and np.all(info["score"] == 400)
    if family == "crowded_windows":
        e = ka.emission(table, FS, cable, C0, xs, ys, z)
        b = ka.bins_and_margin(e, layout(name)[0], params["dt"])[0]
        g, bs = info["node"][0], info["bin"][0]                              # the winning window: the first call's
        inside = (b[:, g] == bs) | (b[:, g] == bs + 1)
        per_channel = np.bincount(table[0][inside], minlength=len(cable))
        twin = np.flatnonzero((table[0][1:] == table[0][:-1]) & (table[1][1:] == table[1][:-1]))      # rows k, k + 1 equal
        twin_in = twin[inside[twin]]
        a = info["assigned"]
        print("crowded_windows: %d channels with >= 2 candidates in the first window, %d exact ties there (%d of them at the "
              "minimum), %d in all" % ((per_channel >= 2).sum(), len(twin_in), (a[twin_in] == 1).sum(), len(twin)))
        assert (per_channel >= 2).sum() >= 20 and len(twin_in) >= 5
        assert np.all(a[twin] > 0) and np.all((a[twin + 1] == 0) | (a[twin + 1] > a[twin]))    # the earlier row goes first
        assert (a[twin_in] == 1).sum() >= 5 and (a[twin + 1] == 0).any()                       # ties at the minimum, decided there
        assert (a == 0).any() and info["votes"].sum() > 0                      # the picks left over stay in the accumulator
        assert np.array_equal(info["votes"], left_over(name, a)[0])
    elif family == "minimal":
        assert (nx, ny, nbins, table.shape[1], len(cable)) == (1, 1, 2, 1, 1)
        assert ncalls == 1 and list(info["assigned"]) == [1] and info["score"][0] == 1 and info["npicks"][0] == 1
        assert ref["Ti"][0, 0] == table[1, 0] / FS and not info["votes"].any()


def compare(name, Ti, info):
    """Ti and info (node, bin, score, npicks, assigned, edges, first_guess, votes) of a backend against the restatement:
    equality, but for the first guess's time, a mean of npicks terms of size <= emax."""
    ref = reference(name)
    Ti_ref, r = ref["Ti"], ref["info"]
    assert Ti.shape == Ti_ref.shape and np.array_equal(Ti, Ti_ref, equal_nan=True)
    for key in ("node", "bin", "score", "npicks", "assigned", "edges"):
        assert np.array_equal(info[key], r[key]), key
    assert np.array_equal(info["first_guess"][:, :3], r["first_guess"][:, :3])
    bound = r["npicks"] * EPS * r["emax"]
    err = np.abs(info["first_guess"][:, 3] - r["first_guess"][:, 3])
    print(name, "first-guess time error", err, "bound", bound)
    assert np.all(err <= bound)
    assert np.array_equal(info["votes"], r["votes"])
