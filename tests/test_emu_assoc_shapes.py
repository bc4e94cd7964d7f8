"""The cases of tests/assoc_cases.py on the CPU emulator build of csrc/assoc.hip, through the C ABI in rounds: grids with
nx != ny, nx = 1 and ny = 1, more than 1024 bins (the vote's second grid dimension), more than 4096 nodes (the arg-max's
grid-stride), windows that two workgroups of the vote write, equal scores, crowded windows with exact ties.  The same cases
run on hardware in tests/test_assoc_shapes_gpu.py.  Every case first asserts the margin rule and its structure conditions on
the restatement; then every count and every choice must be equal.
"""
import ctypes

import numpy as np
import pytest

from tests import assoc_cases as ac
from tests import known_answers_assoc as ka
from tests.emu_util import load_emu
from tests.known_answers_loc import C0
from tests.test_emu_assoc import emu_rounds, emu_vote

FS = ac.FS


@pytest.fixture(scope="module")
def lib():
    lib = load_emu()
    lib.d4w_assoc_best_ws_bytes.restype = ctypes.c_size_t
    return lib


@pytest.mark.parametrize("name", ac.NAMES)
def test_vote(lib, name):
    ac.check_structure(name)
    cable, table, xs, ys, z, params, _ = ac.case(name)
    lo, nbins = ac.layout(name)
    got = emu_vote(lib, table, cable, xs, ys, z, lo, params["dt"], nbins)
    assert np.array_equal(got, ac.reference(name)["votes"])


@pytest.mark.parametrize("name", ac.NAMES)
def test_rounds(lib, name):
    """vote, then best / select / subtract per round, the invariant after every round (emu_rounds asserts it), and at the
    end every record of the restatement."""
    ac.check_structure(name)
    cable, table, xs, ys, z, params, _ = ac.case(name)
    lo, nbins = ac.layout(name)
    ref = ac.reference(name)["info"]
    n = len(ref["node"])
    seen = []

    def after_round(c, votes, state, rec, assigned, Ti):
        seen.append(int(state[1]))
        if c < n:                                            # the calls so far are the restatement's first c + 1
            assert np.array_equal(rec[:c + 1, :3], np.stack([ref["node"], ref["bin"], ref["score"]], axis=1)[:c + 1])
            assert np.array_equal(assigned, np.where(ref["assigned"] <= c + 1, ref["assigned"], 0))

    state, rec, assigned, Ti, fg, votes = emu_rounds(lib, table, cable, xs, ys, z, lo, params["dt"], nbins, params["min_picks"],
                                                     params["max_calls"], after_round)
    assert list(state) == [int(n < params["max_calls"]), n] and seen == [min(c + 1, n) for c in range(params["max_calls"])]
    info = {"node": rec[:n, 0], "bin": rec[:n, 1], "score": rec[:n, 2], "npicks": rec[:n, 3], "assigned": assigned,
            "edges": lo + params["dt"] * np.arange(nbins + 1), "first_guess": fg[:n], "votes": votes}
    ac.compare(name, Ti[:n], info)


def test_subtract_and_add_back_over_an_index_list(lib):
    """The subtract pass over more than 1024 bins stores only the bins it changed, in both bin ranges."""
    name = "rect_17x5_fine-31"
    ac.check_structure(name)
    cable, table, xs, ys, z, params, _ = ac.case(name)
    lo, nbins = ac.layout(name)
    dt = params["dt"]
    first = ac.reference(name)["votes"]
    idx, keep = ac.index_list(name)
    assert (idx < 0).sum() > 100 and (idx >= 0).sum() > 100
    rest, _, m = ka.vote(table[:, keep], FS, cable, C0, xs, ys, z, dt, layout=(lo, nbins))
    assert m >= ka.MARGIN
    changed = first - rest
    assert changed[..., :ac.LDS_BINS].any() and changed[..., ac.LDS_BINS:].any()
    votes = emu_vote(lib, table, cable, xs, ys, z, lo, dt, nbins)
    emu_vote(lib, table, cable, xs, ys, z, lo, dt, nbins, idx=idx, sign=-1, votes=votes)
    assert np.array_equal(votes, rest)
    emu_vote(lib, table, cable, xs, ys, z, lo, dt, nbins, idx=idx, sign=1, votes=votes)
    assert np.array_equal(votes, first)
    stop = np.array([1], dtype=np.int32)
    emu_vote(lib, table, cable, xs, ys, z, lo, dt, nbins, idx=idx, sign=-1, votes=votes, stop=stop)
    assert np.array_equal(votes, first)
