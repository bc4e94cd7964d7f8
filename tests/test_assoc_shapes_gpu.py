"""GPU tests of das4whales_amd.loc.vote_grid / associate_picks (csrc/assoc.hip) at the shapes of tests/assoc_cases.py: grids
with nx != ny, nx = 1 and ny = 1, more than 1024 bins (the vote's second grid dimension, also in the subtract pass), more
than 4096 nodes (the arg-max's grid-stride), windows that two workgroups of the vote write, equal scores above and below
node 4096, crowded windows with exact ties.  tests/test_emu_assoc_shapes.py runs the same cases on the CPU emulator build,
which is compiled without the `fp contract(off)` that the invariant rests on in the HIP build.

Each case first asserts the margin rule of tests/known_answers_assoc.py and its structure conditions on the restatement's
own numbers (assoc_cases.check_structure); then every count and every choice must be exactly equal.  The one bound is the
first guess's time, a mean of npicks terms: npicks eps emax.
"""
import numpy as np
import pytest
import torch

from tests import assoc_cases as ac
from tests import known_answers_assoc as ka
from tests.known_answers_loc import C0

pytestmark = pytest.mark.gpu
FS = ac.FS


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available()
    import das4whales_amd as dw
    return dw


def run(dw, name, **over):
    cable, table, xs, ys, z, params, t0_range = ac.case(name)
    return dw.loc.associate_picks(table, FS, cable, C0, xs, ys, z, return_votes=True, t0_range=t0_range, **dict(params, **over))


def same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and a[1].keys() == b[1].keys() and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])


# ------------------------------------------------------------------------------------------
# every case: parity with the restatement, and the invariant
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ac.NAMES)
def test_case_against_the_restatement(dw, name):
    ac.check_structure(name)
    cable, table, xs, ys, z, params, t0_range = ac.case(name)
    ref = ac.reference(name)
    votes, edges = dw.loc.vote_grid(table, FS, cable, C0, xs, ys, z, params["dt"], t0_range=t0_range)
    assert votes.dtype == np.int32 and votes.shape == ref["votes"].shape
    assert np.array_equal(edges, ref["edges"]) and np.array_equal(votes, ref["votes"])
    Ti, info = run(dw, name)
    ac.compare(name, Ti, info)
    # the invariant: the accumulator left behind is the vote of the unassigned picks counted from scratch
    left, edges_left = dw.loc.vote_grid(table[:, info["assigned"] == 0], FS, cable, C0, xs, ys, z, params["dt"], t0_range=ac.range_of(name))
    assert np.array_equal(edges_left, info["edges"])
    assert np.array_equal(info["votes"], left)


@pytest.mark.parametrize("name", ["rect_17x5_fine-31", "rect_17x5_fine-32", "rect_17x5_fine-33"])
def test_round_by_round(dw, name):
    """max_calls = c returns the first c calls, and its accumulator is the vote of the picks those c rounds left."""
    ac.check_structure(name)
    ref = ac.reference(name)
    r = ref["info"]
    for c in range(1, len(r["node"]) + 1):
        Ti, info = run(dw, name, max_calls=c)
        assert np.array_equal(Ti, ref["Ti"][:c], equal_nan=True)
        for key in ("node", "bin", "score", "npicks"):
            assert np.array_equal(info[key], r[key][:c]), (c, key)
        assert np.array_equal(info["assigned"], np.where(r["assigned"] <= c, r["assigned"], 0)), c
        left, m = ac.left_over(name, r["assigned"], max_calls=c)
        assert m >= ka.MARGIN
        assert np.array_equal(info["votes"], left), c


@pytest.mark.parametrize("name", ["rect_17x5_fine-31", "big_70x61-41"])
def test_two_runs_are_bit_identical(dw, name):
    ac.check_structure(name)
    a, b = run(dw, name), run(dw, name)
    assert len(a[0]) >= 3 and same(a, b)
    assert a[0].tobytes() == b[0].tobytes() and all(a[1][k].tobytes() == b[1][k].tobytes() for k in a[1])


# ------------------------------------------------------------------------------------------
# the subtract pass over an index list, on device memory
# ------------------------------------------------------------------------------------------
def test_subtract_and_add_back_over_an_index_list(dw):
    """More than 1024 bins: each workgroup of the subtract pass stores only the bins of its range that it changed."""
    name = "rect_17x5_fine-31"
    ac.check_structure(name)
    cable, table, xs, ys, z, params, _ = ac.case(name)
    lo, nbins = ac.layout(name)
    lo, dt = float(lo), params["dt"]
    first = ac.reference(name)["votes"]
    idx, keep = ac.index_list(name)
    assert (idx < 0).sum() > 100 and (idx >= 0).sum() > 100
    rest, _, m = ka.vote(table[:, keep], FS, cable, C0, xs, ys, z, dt, layout=(lo, nbins))
    assert m >= ka.MARGIN
    changed = first - rest
    assert changed[..., :ac.LDS_BINS].any() and changed[..., ac.LDS_BINS:].any()

    packed, cab = torch.from_numpy(np.ascontiguousarray(table)).cuda(), torch.from_numpy(np.ascontiguousarray(cable)).cuda()
    gx, gy, idx_d = torch.from_numpy(xs).cuda(), torch.from_numpy(ys).cuda(), torch.from_numpy(idx).cuda()
    votes = torch.full((len(ys), len(xs), nbins), -7, dtype=torch.int32, device="cuda")

    def vote(idx, sign, accumulate, stop=None):
        dw.loc._vote(packed, idx, sign, accumulate, cab, FS, C0, gx, gy, z, lo, dt, nbins, votes, stop)
        return votes.cpu().numpy()
    assert np.array_equal(vote(None, 1, 0), first)
    assert np.array_equal(vote(idx_d, -1, 1), rest)
    assert np.array_equal(vote(idx_d, 1, 1), first)                      # and back
    stop = torch.ones(1, dtype=torch.int32, device="cuda")   # a set stop flag: the launch leaves the accumulator alone
    assert np.array_equal(vote(idx_d, -1, 1, stop), first)
    assert np.array_equal(vote(idx_d, -1, 1, torch.zeros(1, dtype=torch.int32, device="cuda")), rest)


# ------------------------------------------------------------------------------------------
# picker -> association with more than 1024 bins, the picks covering fewer channels than the cable
# ------------------------------------------------------------------------------------------
def test_picker_rows_short_of_the_cable(dw):
    cable, xs, ys, z, fs, ns, samples = ac.picker_scene()
    nrows, nch = samples.shape[1], len(cable)
    assert (nrows, nch) == (390, 400)
    hand = np.full((2, nch), np.nan)
    hand[:, :nrows] = samples / fs
    table, _ = ka.sort_table(np.concatenate([np.stack([np.arange(nrows), s]) for s in samples], axis=1))
    Ti_ref, ref = ka.associate(table, fs, cable, C0, xs, ys, z, 0.05, 200, max_calls=8)
    print("picker scene: nbins", len(ref["edges"]) - 1, "nodes", ref["node"], "bins", ref["bin"], "margin %.3e" % ref["margin"])
    assert ref["margin"] >= ka.MARGIN and np.array_equal(Ti_ref, hand, equal_nan=True)

    x = torch.zeros((nrows, ns), dtype=torch.float32, device="cuda")
    for s in samples:
        x[torch.arange(nrows, device="cuda"), torch.from_numpy(s).cuda()] = 1.0
    picks = dw.detect.pick_times(x, 0.5)
    assert isinstance(picks, dw.detect.PickRows) and picks.total == 2 * nrows and picks.counts.numel() == nrows < nch
    Ti, info = dw.loc.associate_picks(picks, fs, cable, C0, xs, ys, z, 0.05, min_picks=200, max_calls=8, return_votes=True)
    assert torch.is_tensor(Ti) and Ti.is_cuda and Ti.shape == (2, nch)
    Ti, info = Ti.cpu().numpy(), {k: v.cpu().numpy() for k, v in info.items()}
    assert len(info["edges"]) - 1 > ac.LDS_BINS
    assert np.isnan(Ti[:, nrows:]).all()
    host = dw.detect.convert_pick_times(picks)
    assert isinstance(host, np.ndarray) and np.array_equal(host, table)
    Ti_h, info_h = dw.loc.associate_picks(host, fs, cable, C0, xs, ys, z, 0.05, min_picks=200, max_calls=8, return_votes=True)
    assert isinstance(Ti_h, np.ndarray) and same((Ti, info), (Ti_h, info_h))
    assert np.array_equal(Ti, hand, equal_nan=True)
    for key in ("node", "bin", "score", "npicks", "assigned", "edges"):
        assert np.array_equal(info[key], ref[key]), key
    assert np.all(info["npicks"] == nrows) and np.all(info["assigned"] > 0) and not info["votes"].any()
