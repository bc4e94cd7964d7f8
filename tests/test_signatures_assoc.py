"""The association entry points exist at every layer: the three d4w_assoc_* names in the library, in its ctypes binding and
in include/d4w.h, and loc.vote_grid / loc.associate_picks with the parameter names and defaults they were specified with."""
import os

from tests.test_signatures import _params

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "d4w.h")
ENTRY_POINTS = ("d4w_assoc_vote_i32", "d4w_assoc_best_i32", "d4w_assoc_select_f64")
R = "<required>"


def test_assoc_entry_points_are_bound():
    from das4whales_amd import _lib
    with open(HEADER) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        assert ("int %s(" % name) in header, name
        assert _lib.SIGNATURES[name][1][-1] is _lib.ctypes.c_void_p          # the stream comes last
    assert "d4w_assoc_best_ws_bytes" in _lib.SIGNATURES and "size_t d4w_assoc_best_ws_bytes(void)" in header


def test_assoc_python_signatures():
    from das4whales_amd import loc
    head = [("picks", R), ("fs", R), ("cable_pos", R), ("c0", R), ("xs", R), ("ys", R), ("z", R), ("dt", R)]
    assert _params(loc.vote_grid) == head + [("t0_range", None)]
    assert _params(loc.associate_picks) == head + [("min_picks", R), ("max_calls", 64), ("t0_range", None), ("return_votes", False)]
