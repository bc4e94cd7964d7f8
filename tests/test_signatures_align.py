"""The public surface of the alignment against the beam: the two functions of dw.loc with their parameter names and defaults,
their argument checks (which run on the host before any device work, so they are tested here without a GPU), and the two C
symbols in include/d4w.h.  Needs the built library (the package does not import without it); the return shapes and dtypes
need a GPU."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQ = inspect.Parameter.empty
SYMBOLS = ("d4w_align_limits", "d4w_align_f32")

EXPECTED = {
    "align_limits": [],
    "refine_arrivals": [("trace", REQ), ("fs", REQ), ("cable_pos", REQ), ("c0", REQ), ("pos", REQ), ("template", REQ), ("start", REQ),
                        ("max_lag", REQ), ("min_coef", 0.0), ("weights", None), ("next_block", None), ("subsample", True), ("return_all", False)],
}
KEYWORD_ONLY = {"refine_arrivals": [("delays", None)]}         # the table a caller kept, by keyword only


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


def test_docstring_shows_the_loop_and_the_half_period_rule(loc):
    doc = loc.refine_arrivals.__doc__
    at = [doc.index(name + "(") for name in ("locate_stack", "solve_lq_batch", "beamform", "refine_arrivals")]
    assert at == sorted(at) and doc.index("solve_lq_batch(", at[3]) > at[3]          # ... -> refine_arrivals -> solve_lq_batch
    assert "half the dominant period" in doc and "3.9d" in doc


def test_symbols_are_declared_and_bound(loc):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d4w.h")).read(), flags=re.S)
    from das4whales_amd import _lib
    declared = set(re.findall(r"\bint\s+(d4w_align\w*)\s*\(", src))
    assert declared == set(SYMBOLS)                           # every entry point of the header, and no other
    for sym in SYMBOLS:
        assert sym in _lib.SIGNATURES and hasattr(_lib.lib, sym)
    nargs = {sym: len(re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % sym, src, flags=re.S).group(1).split(",")) for sym in SYMBOLS}
    assert {sym: len(_lib.SIGNATURES[sym][1]) for sym in SYMBOLS} == nargs


def test_limits(loc):
    max_calls, max_length, max_lag, channels = loc.align_limits()
    assert max_calls >= 64 and max_length >= 4096 and max_lag >= 255 and channels >= 2


NCH, NS, L = 5, 64, 8
I32, F32 = np.int32, np.float32
BAD = [dict(template=np.ones((2, L))), dict(template=np.ones((2, L), dtype=np.float16)), dict(template=np.ones((3, L), dtype=F32)),
       dict(template=np.ones(L, dtype=F32)), dict(template=np.ones((2, L, 1), dtype=F32)), dict(template=np.ones((2, 0), dtype=F32)),
       dict(template=np.ones((2, 4097), dtype=F32)), dict(template=np.float32(1.0)),
       dict(max_lag=-1), dict(max_lag=1.5), dict(max_lag=True), dict(max_lag=256), dict(max_lag=float("nan")), dict(max_lag=float("inf")),
       dict(max_lag=np.array([2, 2])), dict(max_lag=None),
       dict(min_coef=float("nan")), dict(min_coef=float("inf")), dict(min_coef=-float("inf")), dict(min_coef=np.zeros(2)),
       dict(start=np.zeros(3, dtype=np.int64)), dict(start=np.zeros((2, 1), dtype=np.int64)), dict(start=1.5), dict(start=np.zeros(2)),
       dict(delays=np.zeros((2, NCH), dtype=F32)), dict(delays=np.zeros((2, NCH), dtype=np.int64)), dict(delays=np.zeros((1, NCH), dtype=I32)),
       dict(delays=np.zeros((2, NCH - 1), dtype=I32)), dict(delays=(np.zeros((2, NCH), dtype=I32), np.zeros((2, NCH), dtype=F32))),
       dict(trace=np.ones((4, NS), dtype=F32)), dict(trace=np.ones(NS)), dict(trace=np.ones((NCH, 0), dtype=F32)),
       dict(next_block=np.ones((4, 9), dtype=F32)), dict(next_block=np.ones(9)), dict(fs=0.0), dict(fs=float("nan")), dict(fs=float("inf")),
       dict(c0=-1.0), dict(c0=0.0), dict(c0=float("nan")), dict(pos=np.zeros((2, 2))), dict(pos=np.zeros(4)), dict(pos=np.zeros((2, 3, 1))),
       dict(pos=np.zeros(3)), dict(weights=np.ones(4)), dict(cable_pos=np.zeros((NCH, 2))), dict(cable_pos=np.zeros((4, 3))),
       dict(pos=np.zeros((65536 * 2, 3)), template=np.ones((65536 * 2, 1), dtype=F32))]


def _id(kw):
    return "-".join("%s=%s" % (k, (str(v.dtype) + str(v.shape)) if isinstance(v, np.ndarray) else v) for k, v in kw.items()).replace(" ", "")[:60]


@pytest.mark.parametrize("kw", BAD, ids=_id)
def test_refine_arrivals_rejects_bad_arguments_before_any_gpu_work(loc, kw):
    """ValueError, never the RuntimeError of a missing GPU: nothing was uploaded or launched before the check."""
    base = dict(trace=np.ones((NCH, NS), dtype=F32), fs=50.0, cable_pos=np.arange(3.0 * NCH).reshape(NCH, 3), c0=1490.0, pos=np.zeros((2, 3)),
                template=np.ones((2, L), dtype=F32), start=np.zeros(2, dtype=np.int64), max_lag=2)
    with pytest.raises(ValueError):
        loc.refine_arrivals(**dict(base, **kw))


@pytest.mark.gpu
def test_return_shapes_and_dtypes(loc):
    import torch
    cable, pos = np.arange(15.0).reshape(5, 3) * 100.0, np.array([[50.0, 0.0, 0.0], [900.0, 40.0, -10.0]])
    x, t = np.ones((5, 64), dtype=F32), np.ones((2, L), dtype=F32)
    Ti, coef = loc.refine_arrivals(x, 50.0, cable, 1490.0, pos, t, [3, 4], 2)
    assert isinstance(Ti, np.ndarray) and (Ti.shape, Ti.dtype, coef.shape, coef.dtype) == ((2, 5), np.float64, (2, 5), F32)
    Ti, coef, lag, rho = loc.refine_arrivals(x, 50.0, cable, 1490.0, pos, t, 3, 2, return_all=True)
    assert (lag.shape, lag.dtype, rho.shape, rho.dtype) == ((2, 5), I32, (2, 5, 5), F32)
    Ti, coef = loc.refine_arrivals(x, 50.0, cable, 1490.0, pos[0], t[0], 3, 0)                    # one call as vectors: still [1 x channel]
    assert (Ti.shape, coef.shape) == ((1, 5), (1, 5))
    out = loc.refine_arrivals(torch.from_numpy(x).cuda(), 50.0, cable, 1490.0, pos, t, 3, 2, return_all=True)
    assert all(o.is_cuda for o in out) and [o.dtype for o in out] == [torch.float64, torch.float32, torch.int32, torch.float32]
    out = loc.refine_arrivals(x, 50.0, cable, 1490.0, np.zeros((0, 3)), np.zeros((0, L), dtype=F32), 0, 2, return_all=True)
    assert [o.shape for o in out] == [(0, 5), (0, 5), (0, 5), (0, 5, 5)] and [o.dtype for o in out] == [np.float64, F32, I32, F32]
