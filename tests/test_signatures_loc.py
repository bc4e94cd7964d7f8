"""loc mirrors every function of the reference's loc namespace: each name recorded in
tests/golden/reference_signatures_loc.json (tests/golden/make_loc_golden.py) exists with the reference's parameter names,
order and defaults; parameters beyond the reference's are optional.  The library exports the three d4w_loc_* entry points."""
import json
import os

from tests.test_signatures import _params

SIGNATURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_signatures_loc.json")
NAMES = {"calc_arrival_times", "calc_distance_matrix", "calc_radii_matrix", "calc_theta_vector", "calc_phi_vector", "solve_lq",
         "cal_variance_residuals", "calc_covariance_matrix", "calc_uncertainty_position"}


def test_loc_signatures_complete():
    with open(SIGNATURES) as f:
        ref = json.load(f)["loc"]
    assert set(ref) == NAMES
    import das4whales_amd as dw
    from das4whales_amd import loc
    assert dw.loc is loc and "loc" in dw.__all__
    for name, params in sorted(ref.items()):
        assert hasattr(loc, name), "loc.%s is missing" % name
        pa, pb = [tuple(p) for p in params], _params(getattr(loc, name))
        assert pb[:len(pa)] == pa, (name, pa, pb)
        assert all(d != "<required>" for _, d in pb[len(pa):]), name
    assert _params(loc.solve_lq)[len(ref["solve_lq"]):] == [("first_guess", None), ("verbose", True)]
    assert _params(loc.solve_lq_batch) == [("Ti", "<required>"), ("cable_pos", "<required>"), ("c0", "<required>"), ("Nbiter", 10),
                                           ("fix_z", False), ("first_guess", None), ("return_stats", False)]
    assert [p for p, _ in _params(loc.misfit_grid)] == ["Ti", "cable_pos", "c0", "xs", "ys", "z"]
    assert [p for p, _ in _params(loc.first_guess_grid)] == ["Ti", "cable_pos", "c0", "xs", "ys", "z"]


def test_loc_entry_points_are_bound():
    from das4whales_amd import _lib
    for name in ("d4w_loc_solve_f64", "d4w_loc_misfit_grid_f64", "d4w_loc_arrival_times_f64"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    with open(os.path.join(os.path.dirname(SIGNATURES), "..", "..", "include", "d4w.h")) as f:
        header = f.read()
    assert all(("int %s(" % n) in header for n in ("d4w_loc_solve_f64", "d4w_loc_misfit_grid_f64", "d4w_loc_arrival_times_f64"))
