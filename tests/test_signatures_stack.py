"""The public surface of the delay-and-sum stack: the five functions of dw.loc with their parameter names and defaults, their
argument checks (which run on the host before any device work, so they are tested here without a GPU), and the four C symbols in
include/d4w.h.  Needs the built library (the package does not import without it), no GPU."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQ = inspect.Parameter.empty

EXPECTED = {
    "delay_table": [("cable_pos", REQ), ("c0", REQ), ("fs", REQ), ("xs", REQ), ("ys", REQ), ("z", REQ)],
    "stack_grid": [("env", REQ), ("fs", REQ), ("cable_pos", REQ), ("c0", REQ), ("xs", REQ), ("ys", REQ), ("z", REQ), ("weights", None),
                   ("k_range", None), ("normalize", False)],
    "stack_best": [("stack", REQ)],
    "arrivals_near": [("env", REQ), ("fs", REQ), ("cable_pos", REQ), ("c0", REQ), ("pos", REQ), ("t0", REQ), ("halfwidth", REQ),
                      ("threshold", REQ), ("weights", None)],
    "locate_stack": [("env", REQ), ("fs", REQ), ("cable_pos", REQ), ("c0", REQ), ("xs", REQ), ("ys", REQ), ("z", REQ), ("threshold", REQ),
                     ("halfwidth", REQ), ("pick_threshold", REQ), ("max_calls", 64), ("weights", None), ("k_range", None),
                     ("normalize", False), ("return_stack", False)],
}
KEYWORD_ONLY = {"stack_grid": [("delays", None)]}              # the table a caller kept, by keyword only


@pytest.fixture(scope="module")
def loc():
    if not os.path.exists(os.path.join(ROOT, "das4whales_amd", "lib", "libd4w.so")):
        import __graft_entry__ as ge
        ge.build()
    from das4whales_amd import loc
    return loc


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_public_signature(loc, name):
    params = list(inspect.signature(getattr(loc, name)).parameters.values())
    positional = [(p.name, p.default) for p in params if p.kind == p.POSITIONAL_OR_KEYWORD]
    keyword = [(p.name, p.default) for p in params if p.kind == p.KEYWORD_ONLY]
    assert positional == EXPECTED[name]
    assert keyword == KEYWORD_ONLY.get(name, [])
    assert len(positional) + len(keyword) == len(params)
    assert getattr(loc, name).__doc__


def test_symbols_are_declared_and_bound(loc):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d4w.h")).read(), flags=re.S)
    from das4whales_amd import _lib
    for sym in ("d4w_stack_delays_i32", "d4w_stack_grid_f32", "d4w_stack_best_f32", "d4w_stack_arrivals_f64"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, src), sym
        assert sym in _lib.SIGNATURES and hasattr(_lib.lib, sym)


# The bad-argument lists of tests/test_stack_gpu.py::test_argument_checks at its shapes (5 channels x 64 samples, 2 x 1 nodes), here
# without a GPU: ValueError, never the RuntimeError of a missing GPU -- nothing was uploaded or launched before the check.
CABLE = np.arange(15.0).reshape(5, 3) * 100.0
GEOMETRY = dict(fs=50.0, cable_pos=CABLE, c0=1490.0)
GRID = dict(xs=np.array([30000.0, 31000.0]), ys=np.array([20000.0]), z=-10.0)
ENV = np.ones((5, 64), dtype=np.float32)
BAD_GEOMETRY = [dict(fs=0.0), dict(fs=float("nan")), dict(c0=-1.0), dict(c0=float("inf")), dict(cable_pos=np.zeros((5, 2)))]
BAD_GRID = BAD_GEOMETRY + [dict(xs=np.zeros(0))]
BAD_STACK = BAD_GRID + [dict(k_range=(5, 5)), dict(k_range=(9, 2)), dict(weights=np.ones(4)), dict(env=np.ones((4, 64), dtype=np.float32)),
                        dict(env=np.ones(64))]
BAD = ([("stack_grid", kw) for kw in BAD_STACK + [dict(delays=np.zeros((1, 2, 4), dtype=np.int32))]]
       + [("locate_stack", kw) for kw in BAD_STACK + [dict(halfwidth=-1), dict(max_calls=-1)]]
       + [("delay_table", kw) for kw in BAD_GRID]
       + [("arrivals_near", kw) for kw in BAD_GEOMETRY + [dict(halfwidth=-1), dict(pos=np.zeros((2, 2))), dict(t0=np.zeros(3)),
                                                           dict(threshold=np.zeros(4)), dict(weights=np.ones(4)),
                                                           dict(env=np.ones((4, 64), dtype=np.float32)), dict(env=np.ones(64))]]
       # halfwidth and max_calls go through the one whole-number check of the module (appended: the ids above keep their numbers)
       + [("locate_stack", dict(halfwidth=1.5)), ("locate_stack", dict(max_calls=2.5)), ("locate_stack", dict(halfwidth=True)),
          ("arrivals_near", dict(halfwidth=2.5)), ("arrivals_near", dict(halfwidth=True))])
BASE = {
    "stack_grid": dict(GEOMETRY, env=ENV, **GRID),
    "locate_stack": dict(GEOMETRY, env=ENV, threshold=1.0, halfwidth=3, pick_threshold=0.5, **GRID),
    "delay_table": dict(GEOMETRY, **GRID),
    "arrivals_near": dict(GEOMETRY, env=ENV, pos=np.zeros((2, 3)), t0=np.zeros(2), halfwidth=3, threshold=0.5),
}


@pytest.mark.parametrize("name,kw", BAD, ids=["%s-%s-%d" % (name, "-".join(kw), i) for i, (name, kw) in enumerate(BAD)])
def test_stack_rejects_bad_arguments_before_any_gpu_work(loc, name, kw):
    with pytest.raises(ValueError):
        getattr(loc, name)(**dict(BASE[name], **kw))

