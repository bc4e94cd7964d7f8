"""Delay-and-vote association (csrc/assoc.hip) in the CPU emulator build through the C ABI, against the float64 restatement
of tests/known_answers_assoc.py.  Kernel logic only, host pointers.

Margin rule (known_answers_assoc): every comparison first asserts, on the restatement's own numbers, that no (pick, node)
pair has q = (e - lo) / dt within 1e-9 of an integer; then all counts and all choices must be exactly equal.  The seeds
and offsets below were picked so that the restatement satisfies the margin; the assertion keeps it so.
"""
import ctypes

import numpy as np
import pytest

from tests import known_answers_assoc as ka
from tests.emu_util import load_emu, vp
from tests.known_answers_loc import C0, make_cable

FS = ka.FS
LDS_BINS = 1024          # bins per node of the vote's LDS histogram tile (kAssocBins)
D = ctypes.c_double


@pytest.fixture(scope="module")
def lib():
    lib = load_emu()
    lib.d4w_assoc_best_ws_bytes.restype = ctypes.c_size_t
    return lib


def offsets_of(table, nch):
    return np.cumsum(np.bincount(table[0], minlength=nch)).astype(np.int64)


def emu_vote(lib, table, cable, xs, ys, z, lo, dt, nbins, idx=None, sign=1, votes=None, fs=FS, c0=C0, stop=None):
    table = np.ascontiguousarray(table, dtype=np.int64)
    cable, xs, ys = (np.ascontiguousarray(a, dtype=np.float64) for a in (cable, xs, ys))
    acc = votes is not None
    if votes is None:
        votes = np.full((len(ys), len(xs), nbins), -7, dtype=np.int32)
    rc = lib.d4w_assoc_vote_i32(vp(table) if table.size else None, table.shape[1], vp(idx) if idx is not None else None,
                                len(idx) if idx is not None else 0, sign, int(acc), vp(cable), len(cable), D(fs), D(c0), vp(xs), len(xs),
                                vp(ys), len(ys), D(z), D(lo), D(dt), nbins, vp(votes), vp(stop) if stop is not None else None, None)
    assert rc == 0, lib.d4w_last_error()
    return votes


def check_vote(lib, table, cable, xs, ys, z, dt, t0_range=None):
    ref, edges, m = ka.vote(table, FS, cable, C0, xs, ys, z, dt, t0_range)
    assert m >= ka.MARGIN, m
    lo, nbins = edges[0], len(edges) - 1
    got = emu_vote(lib, table, cable, xs, ys, z, lo, dt, nbins)
    assert np.array_equal(got, ref)
    return ref, lo, nbins


def small_grid(n):
    if n == 1:
        return np.array([37250.0]), np.array([22130.0]), -60.0
    if n == 17:
        return ka.grid17("bent")
    return 20000.0 + 610.0 * np.arange(65), 21000.0 + 2900.0 * np.arange(5), -45.0       # 65 x 5: 325 nodes, 41 tiles of 8


# ------------------------------------------------------------------------------------------
# the vote
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("nch", [5, 400])
def test_vote_pick_counts(lib, nch, K):
    rng = np.random.default_rng(100 + K + nch)
    cable = make_cable("bent", nch)
    table, _ = ka.sort_table(np.stack([rng.integers(0, nch, K), rng.integers(0, 12000, K)]))
    xs, ys, z = small_grid(17)
    ref, _, _ = check_vote(lib, table, cable, xs[3:8], ys[5:8], z, 0.5)
    assert ref.sum() == K * 15                               # the default range holds every pick at every node


@pytest.mark.parametrize("shape", [1, 17, 65])
def test_vote_grids_and_scene(lib, shape):
    cable, table, _ = ka.scene("bent", 400, seed=3)          # ~1400 picks, channels without picks among them
    assert 1300 < table.shape[1] < 1500 and len(np.unique(table[0])) < 400
    xs, ys, z = small_grid(shape)
    check_vote(lib, table, cable, xs, ys, z, 0.5)


def test_vote_two_bins(lib):
    cable, table, _ = ka.scene("line", 400, seed=4)
    xs, ys, z = ka.grid17("line")
    lo, hi = ka.default_range(table, FS, cable, C0, xs[:5], ys[:3], z)
    ref, _, nbins = check_vote(lib, table, cable, xs[:5], ys[:3], z, hi - lo + 1.0)       # one bin holds the range: ceil(< 1) + 1 = 2
    assert nbins == 2 and ref[..., 1].sum() == 0 and ref[..., 0].sum() == table.shape[1] * 15


def test_vote_more_bins_than_the_lds_tile(lib):
    cable, table, _ = ka.scene("bent", 400, seed=5, nclutter=100)
    xs, ys, z = small_grid(65)
    ref, _, nbins = check_vote(lib, table, cable, xs[::8], ys[1:3], z, 0.05)
    assert LDS_BINS < nbins < 2 * LDS_BINS + 200
    assert ref[..., :LDS_BINS].sum() > 0 and ref[..., LDS_BINS:].sum() > 0          # both passes carry votes


def test_vote_range_cuts_both_ends(lib):
    cable, table, _ = ka.scene("bent", 400, seed=6)
    xs, ys, z = small_grid(17)
    full, _, _ = ka.vote(table, FS, cable, C0, xs, ys, z, 0.5)
    ref, _, _ = check_vote(lib, table, cable, xs, ys, z, 0.5, t0_range=(12.3, 31.7))
    assert 0 < ref.sum() < full.sum()
    e = ka.emission(table, FS, cable, C0, xs, ys, z)
    assert (e < 12.3).any() and (e > 32.3).any()


def test_vote_duplicated_pick(lib):
    cable, table, _ = ka.scene("bent", 5, seed=7, nclutter=20)
    table = np.concatenate([table, table[:, 3:4], table[:, 3:4]], axis=1)
    table, _ = ka.sort_table(table)
    xs, ys, z = ka.grid17("bent")
    ref, _, _ = check_vote(lib, table, cable, xs[4:9], ys[4:9], z, 0.5)
    assert ref.max() >= 3


def test_vote_subtract_over_an_index_list(lib):
    cable, table, _ = ka.scene("bent", 400, seed=8)
    xs, ys, z = small_grid(17)
    ref, lo, nbins = check_vote(lib, table, cable, xs, ys, z, 0.5)
    rng = np.random.default_rng(8)
    off = offsets_of(table, 400)
    idx = np.full(400, -1, dtype=np.int32)
    for ch in range(400):
        a, b = (off[ch - 1] if ch else 0), off[ch]
        if b > a and rng.random() < 0.6:
            idx[ch] = rng.integers(a, b)
    assert (idx < 0).any() and (idx >= 0).sum() > 100
    keep = np.ones(table.shape[1], dtype=bool)
    keep[idx[idx >= 0]] = False
    votes = emu_vote(lib, table, cable, xs, ys, z, lo, 0.5, nbins)
    emu_vote(lib, table, cable, xs, ys, z, lo, 0.5, nbins, idx=idx, sign=-1, votes=votes)
    rest, _, m = ka.vote(table[:, keep], FS, cable, C0, xs, ys, z, 0.5, layout=(lo, nbins))
    assert m >= ka.MARGIN and rest.shape == votes.shape
    assert np.array_equal(votes, rest)
    emu_vote(lib, table, cable, xs, ys, z, lo, 0.5, nbins, idx=idx, sign=1, votes=votes)       # and back
    assert np.array_equal(votes, ref)
    stop = np.array([1], dtype=np.int32)                     # a set stop flag: the launch leaves the accumulator alone
    emu_vote(lib, table, cable, xs, ys, z, lo, 0.5, nbins, idx=idx, sign=-1, votes=votes, stop=stop)
    assert np.array_equal(votes, ref)


# ------------------------------------------------------------------------------------------
# arg-max and selection
# ------------------------------------------------------------------------------------------
def emu_best(lib, votes, min_picks, call=0, state=None, rec=None, ncalls=4):
    ny, nx, nbins = votes.shape
    votes = np.ascontiguousarray(votes, dtype=np.int32)
    state = np.zeros(2, dtype=np.int32) if state is None else state
    rec = np.full((ncalls, 4), -7, dtype=np.int32) if rec is None else rec
    ws = np.zeros(lib.d4w_assoc_best_ws_bytes(), dtype=np.uint8)
    rc = lib.d4w_assoc_best_i32(vp(votes), nx, ny, nbins, min_picks, call, vp(state), vp(rec), vp(ws), None)
    assert rc == 0, lib.d4w_last_error()
    return state, rec


def test_best_ties_go_to_the_smaller_flat_index(lib):
    rng = np.random.default_rng(11)
    votes = rng.integers(0, 5, (5, 65, 70)).astype(np.int32)
    h = np.zeros(70, dtype=np.int32)
    h[40:43] = [9, 9, 9]                                     # pairs (40, 41) and (41, 42) both score 18
    for g in (300, 123, 124):                                # identical histograms at three nodes
        votes.reshape(-1, 70)[g] = h
    s = votes.reshape(-1, 70)
    flat = int(np.argmax(s[:, :-1] + s[:, 1:]))
    assert flat == 123 * 69 + 40
    state, rec = emu_best(lib, votes, min_picks=18)
    assert list(state) == [0, 1] and list(rec[0]) == [123, 40, 18, 0]
    state, rec = emu_best(lib, votes, min_picks=19)
    assert list(state) == [1, 0] and np.all(rec == -7)
    state, rec = emu_best(lib, votes, min_picks=1, call=2, state=state, rec=rec)       # stopped: nothing happens
    assert list(state) == [1, 0] and np.all(rec == -7)


@pytest.mark.parametrize("ny,nx,nbins", [(1, 1, 2), (1, 3, 2), (17, 17, 131), (65, 80, 3)])
def test_best_against_argmax(lib, ny, nx, nbins):
    rng = np.random.default_rng(ny + nx + nbins)
    votes = rng.integers(0, 4, (ny, nx, nbins)).astype(np.int32)
    s = votes.reshape(-1, nbins)
    s = s[:, :-1] + s[:, 1:]
    flat = int(np.argmax(s))
    state, rec = emu_best(lib, votes, min_picks=1, call=1)
    assert list(state) == [0, 2] and list(rec[1]) == [flat // (nbins - 1), flat % (nbins - 1), s.reshape(-1)[flat], 0]


def emu_select(lib, table, cable, xs, ys, z, lo, dt, nbins, call, state, rec, assigned, Ti, fs=FS, c0=C0, fg=None):
    nch = len(cable)
    table = np.ascontiguousarray(table, dtype=np.int64)
    cable, xs, ys = (np.ascontiguousarray(a, dtype=np.float64) for a in (cable, xs, ys))
    off = offsets_of(table, nch)
    chosen, e_chosen = np.full(nch, -7, dtype=np.int32), np.full(nch, 7.0)
    fg = np.full((len(rec), 4), 7.0) if fg is None else fg
    rc = lib.d4w_assoc_select_f64(vp(table), table.shape[1], vp(off), vp(cable), nch, D(fs), D(c0), vp(xs), len(xs), vp(ys), len(ys), D(z),
                                  D(lo), D(dt), nbins, call, vp(state), vp(rec), vp(assigned), vp(Ti), vp(chosen), vp(e_chosen), vp(fg), None)
    assert rc == 0, lib.d4w_last_error()
    return chosen, e_chosen, fg


def test_select_ties_go_to_the_smaller_k(lib):
    # the node sits ON channel 1: the distance is exactly 0, e = t exactly.  lo = 0, dt = 1, b* = 4: ec = 5; fs = 4.
    cable = np.array([[0.0, 0.0, -100.0], [1000.0, 0.0, -100.0], [2000.0, 0.0, -100.0]])
    xs, ys, z = np.array([1000.0]), np.array([0.0]), -100.0
    # channel 1: samples 17 (4.25), 19 (4.75), 21 (5.25), 23 (5.75): 19 and 21 are equidistant from 5 -> the smaller k, 19
    table = np.array([[1, 1, 1, 1], [17, 19, 21, 23]], dtype=np.int64)
    state, assigned = np.zeros(2, dtype=np.int32), np.zeros(4, dtype=np.int32)
    rec = np.array([[0, 4, 4, 0]], dtype=np.int32)
    Ti = np.full((1, 3), 7.0)
    chosen, e_chosen, fg = emu_select(lib, table, cable, xs, ys, z, 0.0, 1.0, 8, 0, state, rec, assigned, Ti, fs=4.0)
    assert list(chosen) == [-1, 1, -1] and list(assigned) == [0, 1, 0, 0]
    assert np.isnan(Ti[0, 0]) and Ti[0, 1] == 4.75 and np.isnan(Ti[0, 2]) and e_chosen[1] == 4.75
    assert list(rec[0]) == [0, 4, 4, 1] and list(fg[0]) == [1000.0, 0.0, -100.0, 4.75]
    # with 19 taken, the next round on the same window takes 21; then the nearer of 17 and 23 is a tie again -> 17
    for want, t in ((2, 5.25), (0, 4.25), (3, 5.75)):
        chosen, _, _ = emu_select(lib, table, cable, xs, ys, z, 0.0, 1.0, 8, 0, state, rec, assigned, Ti, fs=4.0)
        assert chosen[1] == want and Ti[0, 1] == t
    chosen, _, fg = emu_select(lib, table, cable, xs, ys, z, 0.0, 1.0, 8, 0, state, rec, assigned, Ti, fs=4.0)
    assert list(chosen) == [-1, -1, -1] and rec[0, 3] == 0 and np.isnan(fg[0, 3]) and np.all(assigned == 1)


def emu_rounds(lib, table, cable, xs, ys, z, lo, dt, nbins, min_picks, max_calls, after_round=None):
    """The greedy loop as loc.associate_picks enqueues it: the vote, then best / select / subtract `max_calls` times with
    the stop flag handed on.  After every round the accumulator must be the restatement's vote of the picks not assigned so
    far, and after_round(c, votes, state, rec, assigned, Ti) may look further.  Returns (state, rec, assigned, Ti, fg, votes)."""
    nch = len(cable)
    votes = emu_vote(lib, table, cable, xs, ys, z, lo, dt, nbins)
    state, rec = np.zeros(2, dtype=np.int32), np.zeros((max_calls, 4), dtype=np.int32)
    assigned, Ti = np.zeros(table.shape[1], dtype=np.int32), np.full((max_calls, nch), 7.0)
    fg = np.full((max_calls, 4), 7.0)
    for c in range(max_calls):
        emu_best(lib, votes, min_picks, call=c, state=state, rec=rec)
        chosen, _, _ = emu_select(lib, table, cable, xs, ys, z, lo, dt, nbins, c, state, rec, assigned, Ti, fg=fg)
        emu_vote(lib, table, cable, xs, ys, z, lo, dt, nbins, idx=chosen, sign=-1, votes=votes, stop=state)
        left, _, _ = ka.vote(table[:, assigned == 0], FS, cable, C0, xs, ys, z, dt, layout=(lo, nbins))
        assert np.array_equal(votes, left), c                # the invariant, after every round
        if after_round is not None:
            after_round(c, votes, state, rec, assigned, Ti)
    return state, rec, assigned, Ti, fg, votes


@pytest.mark.parametrize("kind,seed", [("bent", 21), ("line", 22)])
def test_rounds_against_the_restatement(lib, kind, seed):
    cable, table, _ = ka.scene(kind, 400, seed=seed)
    xs, ys, z = ka.grid17(kind)
    Ti_ref, ref = ka.associate(table, FS, cable, C0, xs, ys, z, 0.5, 60, max_calls=8)
    assert ref["margin"] >= ka.MARGIN and 3 <= len(Ti_ref) < 8
    lo, nbins = ref["edges"][0], len(ref["edges"]) - 1
    state, rec, assigned, Ti, fg, votes = emu_rounds(lib, table, cable, xs, ys, z, lo, 0.5, nbins, 60, 8)
    n = len(Ti_ref)
    assert list(state) == [1, n]
    assert np.array_equal(Ti[:n], Ti_ref, equal_nan=True) and np.array_equal(assigned, ref["assigned"])
    for j, name in enumerate(("node", "bin", "score", "npicks")):
        assert np.array_equal(rec[:n, j], ref[name]), name
    assert np.array_equal(votes, ref["votes"])
    assert np.array_equal(fg[:n, :3], ref["first_guess"][:, :3])
    bound = ref["npicks"] * np.finfo(np.float64).eps * ref["emax"]
    assert np.all(np.abs(fg[:n, 3] - ref["first_guess"][:, 3]) <= bound)


# ------------------------------------------------------------------------------------------
# bad arguments
# ------------------------------------------------------------------------------------------
def test_bad_arguments(lib):
    cable = np.ascontiguousarray(make_cable("line", 5))
    table = np.array([[0, 2, 4], [100, 200, 300]], dtype=np.int64)
    xs, ys = np.array([30000.0, 31000.0]), np.array([20000.0])
    votes = np.zeros((1, 2, 4), dtype=np.int32)
    nan, inf = float("nan"), float("inf")

    def vote(nch=5, nx=2, ny=1, nbins=4, dt=0.5, fs=FS, c0=C0, sign=1, cab=cable, v=votes, gx=xs, K=3):
        return lib.d4w_assoc_vote_i32(vp(table), K, None, 0, sign, 0, vp(cab) if cab is not None else None, nch, D(fs), D(c0),
                                      vp(gx) if gx is not None else None, nx, vp(ys), ny, D(-60.0), D(0.0), D(dt), nbins,
                                      vp(v) if v is not None else None, None, None)
    bad = [dict(nch=0), dict(nx=0), dict(ny=0), dict(nbins=1), dict(dt=0.0), dict(dt=-1.0), dict(dt=nan), dict(dt=inf), dict(fs=0.0),
           dict(fs=nan), dict(c0=0.0), dict(c0=-C0), dict(c0=inf), dict(sign=0), dict(sign=2), dict(cab=None), dict(v=None), dict(gx=None),
           dict(K=-1)]
    assert vote() == 0
    for kw in bad:
        assert vote(**kw) == -1, kw
        assert len(lib.d4w_last_error()) > 0
    votes[:] = -7
    assert vote(K=0) == 0 and np.all(votes == 0)             # no picks: zeros

    state, rec = np.zeros(2, dtype=np.int32), np.zeros((1, 4), dtype=np.int32)
    ws = np.zeros(lib.d4w_assoc_best_ws_bytes(), dtype=np.uint8)

    def best(nx=2, ny=1, nbins=4, v=votes, st=state, w=ws, call=0):
        return lib.d4w_assoc_best_i32(vp(v) if v is not None else None, nx, ny, nbins, 1, call, vp(st) if st is not None else None, vp(rec),
                                      vp(w) if w is not None else None, None)
    assert best() == 0
    for kw in (dict(nx=0), dict(ny=0), dict(nbins=1), dict(v=None), dict(st=None), dict(w=None), dict(call=-1)):
        assert best(**kw) == -1, kw

    off = offsets_of(table, 5)
    assigned, Ti, chosen, ech, fg = np.zeros(3, dtype=np.int32), np.zeros((1, 5)), np.zeros(5, dtype=np.int32), np.zeros(5), np.zeros((1, 4))
    state[:] = 0

    def select(nch=5, nx=2, ny=1, nbins=4, dt=0.5, fs=FS, c0=C0, o=off, t=Ti):
        return lib.d4w_assoc_select_f64(vp(table), 3, vp(o) if o is not None else None, vp(cable), nch, D(fs), D(c0), vp(xs), nx, vp(ys), ny,
                                        D(-60.0), D(0.0), D(dt), nbins, 0, vp(state), vp(rec), vp(assigned), vp(t) if t is not None else None,
                                        vp(chosen), vp(ech), vp(fg), None)
    rec[0] = [0, 0, 1, 0]
    assert select() == 0
    for kw in (dict(nch=0), dict(nx=0), dict(ny=0), dict(nbins=1), dict(dt=0.0), dict(dt=nan), dict(fs=-1.0), dict(fs=inf), dict(c0=0.0),
               dict(c0=nan), dict(o=None), dict(t=None)):
        assert select(**kw) == -1, kw
