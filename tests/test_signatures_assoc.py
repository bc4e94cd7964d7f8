"""The association entry points exist at every layer: the three d4w_assoc_* names in the library, in its ctypes binding and
in include/d4w.h, and loc.vote_grid / loc.associate_picks with the parameter names and defaults they were specified with; their
argument checks run on the host before any device work, so they are tested here without a GPU."""
import os

import numpy as np
import pytest

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


# The bad calls of tests/test_assoc_gpu.py::test_value_errors, and the shared geometry checks, on 5 channels and 2 x 1 nodes, here
# without a GPU: ValueError, never the RuntimeError of a missing GPU -- nothing was uploaded or launched before the check.
TABLE = np.array([[0, 1, 2, 3, 4, 4], [10, 12, 15, 19, 24, 40]])
BASE = dict(picks=TABLE, fs=50.0, cable_pos=np.arange(15.0).reshape(5, 3) * 100.0, c0=1490.0, xs=np.array([30000.0, 31000.0]),
            ys=np.array([20000.0]), z=-10.0, dt=0.5)
BAD_BOTH = [dict(picks=np.array([[0, 1, 5], [10, 12, 15]])), dict(picks=np.array([[-1, 1, 2], [10, 12, 15]])), dict(dt=0.0), dict(dt=float("nan")),
            dict(fs=0.0), dict(c0=float("inf")), dict(c0=-1.0), dict(xs=np.zeros(0)), dict(cable_pos=np.zeros((5, 2))),
            dict(picks=np.zeros((3, 4), dtype=np.int64)), dict(picks=np.array([[0.5, 1.0], [10.0, 12.0]]))]
BAD = ([("vote_grid", kw) for kw in BAD_BOTH] + [("associate_picks", dict(kw, min_picks=2)) for kw in BAD_BOTH]
       + [("associate_picks", dict(min_picks=0)), ("associate_picks", dict(min_picks=2, max_calls=-1))])


@pytest.mark.parametrize("name,kw", BAD, ids=["%s-%s-%d" % (name, "-".join(kw), i) for i, (name, kw) in enumerate(BAD)])
def test_assoc_rejects_bad_arguments_before_any_gpu_work(name, kw):
    from das4whales_amd import loc
    with pytest.raises(ValueError):
        getattr(loc, name)(**dict(BASE, **kw))
