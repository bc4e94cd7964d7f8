"""GPU tests of das4whales_amd.loc.vote_grid / associate_picks (csrc/assoc.hip) through the Python interface.

Parity is against the float64 restatement of tests/known_answers_assoc.py under its margin rule: each case first asserts,
on the restatement's own numbers, that no (pick, node) pair has q = (e - lo) / dt within 1e-9 of an integer (the device's
reciprocal multiplies move q by about 1e-11 at most); then every count and every choice must be exactly equal.  The seeds
were picked so that the restatement satisfies the margin.  The third case has 3000 channels and about 2e4 picks: three
sources on 70 % of the channels are 6300 picks, the rest is clutter (the two 400-channel cases carry 600 clutter picks).
"""
import functools

import numpy as np
import pytest
import torch

from tests import known_answers_assoc as ka
from tests.known_answers_loc import C0, make_cable

pytestmark = pytest.mark.gpu
FS = ka.FS
EPS = np.finfo(np.float64).eps
CASES = {"bent_400": ("bent", 400, 21, 600), "line_400": ("line", 400, 22, 600), "bent_3000": ("bent", 3000, 23, 13700)}
PARAMS = dict(dt=0.5, min_picks=60, max_calls=8)


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available()
    import das4whales_amd as dw
    return dw


@functools.lru_cache(maxsize=None)
def reference(case):
    """(cable, table, grid, restatement's Ti and info), computed once and shared; callers do not modify it."""
    kind, nch, seed, nclutter = CASES[case]
    cable, table, _ = ka.scene(kind, nch, seed=seed, nclutter=nclutter)
    xs, ys, z = ka.grid17(kind)
    Ti, info = ka.associate(table, FS, cable, C0, xs, ys, z, **PARAMS)
    return cable, table, (xs, ys, z), Ti, info


# ------------------------------------------------------------------------------------------
# parity with the restatement, and the invariant
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_parity_with_the_restatement(dw, case):
    cable, table, (xs, ys, z), Ti_ref, ref = reference(case)
    print(case, "picks", table.shape[1], "margin %.3e" % ref["margin"], "calls", len(Ti_ref), "scores", ref["score"])
    assert ref["margin"] >= ka.MARGIN
    if case == "bent_3000":
        assert 1.9e4 < table.shape[1] < 2.1e4
    assert len(Ti_ref) >= 3
    v_ref, edges_ref, _ = ka.vote(table, FS, cable, C0, xs, ys, z, PARAMS["dt"])
    votes, edges = dw.loc.vote_grid(table, FS, cable, C0, xs, ys, z, PARAMS["dt"])
    assert isinstance(votes, np.ndarray) and votes.dtype == np.int32 and edges.dtype == np.float64
    assert np.array_equal(edges, edges_ref) and np.array_equal(votes, v_ref)
    Ti, info = dw.loc.associate_picks(table, FS, cable, C0, xs, ys, z, return_votes=True, **PARAMS)
    assert Ti.shape == Ti_ref.shape and np.array_equal(Ti, Ti_ref, equal_nan=True)
    for name in ("node", "bin", "score", "npicks", "assigned", "edges"):
        assert np.array_equal(info[name], ref[name]), name
    assert np.array_equal(info["first_guess"][:, :3], ref["first_guess"][:, :3])
    bound = ref["npicks"] * EPS * ref["emax"]                # rounding of a sum of npicks terms of size <= max |e|, over npicks
    err = np.abs(info["first_guess"][:, 3] - ref["first_guess"][:, 3])
    print(case, "first-guess time error", err, "bound", bound)
    assert np.all(err <= bound)
    # the invariant: the accumulator left behind is the vote of the unassigned picks counted from scratch
    assert np.array_equal(info["votes"], ref["votes"])
    t0_range = ka.default_range(table, FS, cable, C0, xs, ys, z)
    left, _ = dw.loc.vote_grid(table[:, info["assigned"] == 0], FS, cable, C0, xs, ys, z, PARAMS["dt"], t0_range=t0_range)
    Ti2, info2 = dw.loc.associate_picks(table, FS, cable, C0, xs, ys, z, return_votes=True, t0_range=t0_range, **PARAMS)
    assert np.array_equal(Ti2, Ti, equal_nan=True) and np.array_equal(info2["votes"], info["votes"])
    assert np.array_equal(info2["votes"], left)


# ------------------------------------------------------------------------------------------
# a known answer that needs no restatement
# ------------------------------------------------------------------------------------------
def test_sources_on_nodes_come_back_exactly(dw):
    nch = 400
    cable = make_cable("bent", nch)
    xs, ys, z = ka.grid17("bent")
    # emission times in the middle of a 0.5-s bin of t0_range = (0, 130); sample rounding spreads a call's e by <= 0.5 / fs
    srcs = [(11, 4, 50.25), (3, 9, 10.25), (6, 13, 90.25)]   # (ix, iy, t0): 40 s apart, more than any moveout across the grid
    rows, Ti_want = [], {}
    for ix, iy, t0 in srcs:
        arr = t0 + np.sqrt(((cable - [xs[ix], ys[iy], z]) ** 2).sum(1)) / C0
        i = np.round(arr * FS).astype(np.int64)
        rows.append(np.stack([np.arange(nch), i]))
        Ti_want[iy * 17 + ix] = i / FS
    table, _ = ka.sort_table(np.concatenate(rows, axis=1))
    Ti, info = dw.loc.associate_picks(table, FS, cable, C0, xs, ys, z, 0.5, min_picks=60, max_calls=8, t0_range=(0.0, 130.0))
    assert Ti.shape == (3, nch)
    assert np.all(info["score"] == nch) and np.all(info["npicks"] == nch)
    assert sorted(info["node"]) == sorted(Ti_want)
    # equal scores: the calls come out in the order of the flat index node (nbins - 1) + bin
    nbins = len(info["edges"]) - 1
    flat = info["node"].astype(np.int64) * (nbins - 1) + info["bin"]
    assert np.all(np.diff(flat) > 0)
    for c, g in enumerate(info["node"]):
        assert np.array_equal(Ti[c], Ti_want[int(g)])
        t0 = [s[2] for s in srcs if s[1] * 17 + s[0] == g][0]
        assert info["bin"][c] in (int(t0 / 0.5) - 1, int(t0 / 0.5))      # all 400 picks sit in one bin: both pairs holding it score 400
        assert abs(info["first_guess"][c, 3] - t0) <= 0.5 / FS
        assert np.array_equal(info["first_guess"][c, :3], [xs[g % 17], ys[g // 17], z])
    assert np.all(info["assigned"] > 0)


# ------------------------------------------------------------------------------------------
# the chain: picker -> association -> localisation
# ------------------------------------------------------------------------------------------
def test_chain_pick_associate_localise(dw):
    nch, ns, fs = 400, 2400, 40.0
    cable = make_cable("bent", nch)
    xs, ys, z = ka.grid17("bent")
    x = torch.zeros((nch, ns), dtype=torch.float32, device="cuda")
    want = []
    for ix, iy, t0 in ((5, 6, 5.0), (12, 10, 30.0)):
        arr = t0 + np.sqrt(((cable - [xs[ix], ys[iy], z]) ** 2).sum(1)) / C0
        i = np.round(arr * fs).astype(np.int64)
        assert i.max() < ns - 1
        x[torch.arange(nch, device="cuda"), torch.from_numpy(i).cuda()] = 1.0
        want.append(i / fs)
    picks = dw.detect.pick_times(x, 0.5)
    assert isinstance(picks, dw.detect.PickRows) and picks.total == 2 * nch
    Ti, info = dw.loc.associate_picks(picks, fs, cable, C0, xs, ys, z, 0.5, min_picks=200, max_calls=8)
    assert torch.is_tensor(Ti) and Ti.is_cuda and Ti.dtype == torch.float64 and Ti.shape == (2, nch)
    assert all(torch.is_tensor(v) and v.is_cuda for v in info.values())
    order = np.argsort(info["first_guess"][:, 3].cpu().numpy())
    hand = np.stack(want)
    assert np.array_equal(Ti.cpu().numpy()[order], hand)
    assert np.all(info["npicks"].cpu().numpy() == nch) and np.all(info["assigned"].cpu().numpy() > 0)
    fg = info["first_guess"]
    n = dw.loc.solve_lq_batch(Ti, cable, C0, fix_z=True, first_guess=fg)
    n_hand = dw.loc.solve_lq_batch(hand[np.argsort(order)], cable, C0, fix_z=True, first_guess=fg.cpu().numpy())
    assert np.array_equal(n.cpu().numpy(), n_hand)
    assert np.all(np.abs(n_hand[order][:, 3] - [5.0, 30.0]) < 0.05)


# ------------------------------------------------------------------------------------------
# containers and edge cases
# ------------------------------------------------------------------------------------------
def test_containers(dw):
    cable, table, (xs, ys, z), Ti_ref, ref = reference("bent_400")
    Ti, info = dw.loc.associate_picks(table, FS, cable, C0, xs, ys, z, **PARAMS)
    assert isinstance(Ti, np.ndarray) and Ti.dtype == np.float64
    assert info["first_guess"].dtype == np.float64 and info["edges"].dtype == np.float64
    assert all(isinstance(info[k], np.ndarray) and info[k].dtype == np.int32 for k in ("node", "bin", "score", "npicks", "assigned"))
    assert "votes" not in info
    # the other host forms of the same picks
    ragged = [table[1][table[0] == ch] for ch in range(len(cable))]
    for form in ((table[0], table[1]), ragged):
        Ti_f, info_f = dw.loc.associate_picks(form, FS, cable, C0, xs, ys, z, **PARAMS)
        assert np.array_equal(Ti_f, Ti, equal_nan=True) and np.array_equal(info_f["assigned"], info["assigned"])
    # a tensor on the device: tensors on that device
    Ti_t, info_t = dw.loc.associate_picks(torch.from_numpy(table).cuda(), FS, cable, C0, xs, ys, z, return_votes=True, **PARAMS)
    assert torch.is_tensor(Ti_t) and Ti_t.is_cuda and Ti_t.dtype == torch.float64
    assert all(torch.is_tensor(v) and v.is_cuda for v in info_t.values()) and info_t["votes"].dtype == torch.int32
    assert np.array_equal(Ti_t.cpu().numpy(), Ti, equal_nan=True)
    votes_t, edges_t = dw.loc.vote_grid(torch.from_numpy(table).cuda(), FS, torch.from_numpy(cable).cuda(), C0, xs, ys, z, 0.5)
    assert votes_t.is_cuda and votes_t.dtype == torch.int32 and edges_t.is_cuda and edges_t.dtype == torch.float64
    assert tuple(votes_t.shape) == (17, 17, len(ref["edges"]) - 1)


def test_edge_cases(dw):
    cable, table, (xs, ys, z), Ti_ref, ref = reference("bent_400")
    nch = len(cable)
    kw = dict(PARAMS)
    Ti, info = dw.loc.associate_picks(table, FS, cable, C0, xs, ys, z, **dict(kw, min_picks=int(ref["score"].max()) + 1))
    assert Ti.shape == (0, nch) and info["first_guess"].shape == (0, 4) and info["node"].shape == (0,)
    assert np.all(info["assigned"] == 0)
    Ti, info = dw.loc.associate_picks(table, FS, cable, C0, xs, ys, z, **dict(kw, max_calls=1))
    assert np.array_equal(Ti, Ti_ref[:1], equal_nan=True) and info["node"][0] == ref["node"][0]
    assert np.array_equal(info["assigned"], np.where(ref["assigned"] == 1, 1, 0))
    Ti, info = dw.loc.associate_picks(table, FS, cable, C0, xs, ys, z, **dict(kw, max_calls=0))
    assert Ti.shape == (0, nch)
    empty = np.zeros((2, 0), dtype=np.int64)
    Ti, info = dw.loc.associate_picks(empty, FS, cable, C0, xs, ys, z, **kw)
    assert Ti.shape == (0, nch) and info["assigned"].shape == (0,)
    votes, edges = dw.loc.vote_grid(empty, FS, cable, C0, xs, ys, z, 0.5, t0_range=(0.0, 10.0))
    assert votes.shape == (17, 17, 21) and not votes.any()
    # an unsorted table: the same calls, `assigned` in the caller's order  (this table holds no pick twice)
    perm = np.random.default_rng(5).permutation(table.shape[1])
    Ti_p, info_p = dw.loc.associate_picks(table[:, perm], FS, cable, C0, xs, ys, z, **kw)
    assert np.array_equal(Ti_p, Ti_ref, equal_nan=True)
    for name in ("node", "bin", "score", "npicks"):
        assert np.array_equal(info_p[name], ref[name])
    assert np.array_equal(info_p["assigned"], ref["assigned"][perm])
    # two runs are bit-identical
    a = dw.loc.associate_picks(table, FS, cable, C0, xs, ys, z, return_votes=True, **kw)
    b = dw.loc.associate_picks(table, FS, cable, C0, xs, ys, z, return_votes=True, **kw)
    assert np.array_equal(a[0], b[0], equal_nan=True) and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])


def test_value_errors(dw):
    cable, table, (xs, ys, z), _, _ = reference("bent_400")
    bad = table.copy()
    bad[0, -1] = len(cable)
    with pytest.raises(ValueError):
        dw.loc.associate_picks(bad, FS, cable, C0, xs, ys, z, **PARAMS)
    bad[0, -1] = table[0, -1]
    bad[0, 0] = -1
    with pytest.raises(ValueError):
        dw.loc.vote_grid(bad, FS, cable, C0, xs, ys, z, 0.5)
    with pytest.raises(ValueError):
        dw.loc.associate_picks(table, FS, cable, C0, xs, ys, z, 0.5, min_picks=0)
    with pytest.raises(ValueError):
        dw.loc.associate_picks(table, FS, cable, C0, xs, ys, z, 0.5, min_picks=60, max_calls=-1)
    with pytest.raises(ValueError):
        dw.loc.associate_picks(table, FS, cable, C0, xs, ys, z, 0.0, min_picks=60)
