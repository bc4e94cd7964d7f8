"""The public surface of the delay-and-sum stack: the five functions of dw.loc with their parameter names and defaults, and
the four C symbols in include/d4w.h.  Needs the built library (the package does not import without it), no GPU."""
import inspect
import os
import re

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

