"""Pins oracle/d4w_oracle.py against what the REAL reference returns at the edge cases of tests/design_cases.py
(tests/golden/design_edges.npz, made by tests/golden/make_design_golden.py): odd shapes, one channel, grid points exactly on
a speed edge, band edges that move the column loops.  Bit for bit.  CPU only."""
import numpy as np
import pytest

from oracle import d4w_oracle as orc
from tests import design_cases as dc


@pytest.fixture(scope="module")
def g(golden):
    return golden("design_edges.npz")


def test_fixture_holds_the_cases(g):
    cases = [str(c) for c in g["cases"]]
    assert cases == [c for c in dc.FIXTURE_CASES if c in cases]
    assert set(dc.FIXTURE_CASES) - set(cases) <= {"wide"}         # the one case the generator may leave out for size
    assert set(dc.TIE_CASES + ("low_band", "high_band", "odd_odd", "odd_even", "even_odd", "tiny", "one_channel")) <= set(cases)


@pytest.mark.parametrize("case", dc.FIXTURE_CASES)
def test_oracle_equals_reference(g, case):
    if case not in [str(c) for c in g["cases"]]:
        assert case == "wide"
        return
    shape = dc.CASES[case][0]
    for design in dc.DESIGNS:
        if not dc.has_design(case, design):
            # the reference's |H|^2 row has 2 (ns // 2) columns: an [nx, ns - 1] mask no [nx, ns] record can be multiplied with
            assert tuple(g[case + "/ninf_shape"]) == (shape[0], shape[1] - 1)
            continue
        m = dc.oracle(case, design)
        assert m.shape == shape
        assert np.array_equal(m, g["%s/%s" % (case, design)]), (case, design)


@pytest.mark.parametrize("shape", dc.FKFILT_SHAPES)
def test_fk_filt_equals_reference(g, shape):
    y = orc.fk_filt(dc.fkfilt_block(shape), *dc.FKFILT_ARGS)
    assert np.array_equal(y, g["fkfilt/%dx%d" % shape])


@pytest.mark.parametrize("case", dc.TIE_CASES)
def test_tie_cases_have_ties(case):
    """A tie case stays a tie case: points with |f / k| exactly on each of the four speeds, from the float64 axes."""
    counts = dc.tie_counts(case)
    assert all(c > 0 for c in counts), counts
    assert counts == dc.TIE_COUNTS[case]


def test_band_edges_move_the_loop_range():
    ns = dc.CASES["low_band"][0][1]
    assert dc.loop_range("low_band", 4.0)[0] < ns // 2 and dc.loop_range("low_band", 14.0)[0] < ns // 2
    assert dc.loop_range("high_band", 14.0)[1] == 0             # nothing at or above fmax + 14: np.argmax returns 0
    assert dc.loop_range("high_band", 4.0)[1] > ns // 2         # ... while the 4-Hz designs keep their loop


@pytest.mark.parametrize("case", dc.EDGE_CASES)
def test_oracle_leaves_few_points_out_of_the_side_check(case):
    """The side check of the GPU and emulator tests (design_cases.sides_agree) compares zeros and non-zeros at every grid
    point but the non-zero oracle values below 1e-6.  In the columns where a design reaches 1e-6 at all, those are under
    1 % of the points compared; for the classic fan there are none.  (Of the NON-ZERO points alone they are no such small
    share: hybrid_ninf's Butterworth row never reaches zero, so 96 % of its non-zero values at 64 x 64 are tails below 1e-6,
    and hybrid has 2 nx values of 6.1e-17 where the reference takes cos(pi / 2).)"""
    for design in dc.CLOSED:
        ref = dc.oracle(case, design)
        wrong, left_out, points = dc.sides_agree(ref, ref)
        print("%s %s: %d of %d points of the live columns left out" % (case, design, left_out, points))
        assert wrong == 0 and points > 0 and left_out <= 0.01 * points, (design, left_out, points)
        if design == "classic":
            assert left_out == 0
    # the tie points themselves are compared, not left out: on the classic fan every one of them is an exact 0 or 1 or sine
    if case in dc.TIE_CASES:
        k, f = dc.axes(case)
        p = dc.CASES[case][4]
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.abs(f[None, :] / k[:, None])
        ref = dc.oracle(case, "classic")
        assert np.all(ref[s == p["cs_min"]] == 0.0) and np.all(ref[s == p["cs_max"]] == 0.0)      # sin(0), s >= cs_max
        fan = np.broadcast_to(np.abs(k[:, None]) >= 0.005, s.shape)                              # rows with |k| < 0.005 are zero
        for speed in ("cp_min", "cp_max"):                                                        # sin(pi / 2), 1 - sin(0)
            on = (s == p[speed]) & fan
            assert np.count_nonzero(on) > 0 and np.all(ref[on] == 1.0), speed
