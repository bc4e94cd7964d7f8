"""The public surface of the transpose of the beam: the four functions of dw.loc with their parameter names and defaults, their
argument checks (which run on the host before any device work, so they are tested here without a GPU), and the three C symbols
in include/d4w.h against das4whales_amd/_lib.py.  Needs the built library (the package does not import without it); the return
shapes and dtypes need a GPU."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQ = inspect.Parameter.empty
SYMBOLS = ("d4w_project_limits", "d4w_project_f32", "d4w_project_subtract_f32")

EXPECTED = {
    "project_limits": [],
    "project_calls": [("trace", REQ), ("fs", REQ), ("cable_pos", REQ), ("c0", REQ), ("pos", REQ), ("beam", REQ), ("start", REQ), ("order", 1),
                      ("weights", None), ("next_block", None)],
    "subtract_calls": [("trace", REQ), ("fs", REQ), ("cable_pos", REQ), ("c0", REQ), ("pos", REQ), ("beam", REQ), ("start", REQ), ("amp", REQ),
                       ("order", 1), ("next_block", None), ("inplace", False)],
    "remove_calls": [("trace", REQ), ("fs", REQ), ("cable_pos", REQ), ("c0", REQ), ("pos", REQ), ("start", REQ), ("length", REQ), ("order", 1),
                     ("min_coef", 0.0), ("weights", None), ("next_block", None), ("inplace", False), ("return_parts", False)],
}
KEYWORD_ONLY = {"project_calls": [("delays", None)], "subtract_calls": [("delays", None)]}


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


def test_docstrings_say_what_the_beam_holds(loc):
    assert "1 / channels" in loc.project_calls.__doc__ and "1 / channels" in loc.remove_calls.__doc__
    assert "never read" in loc.project_calls.__doc__ and "jointly" in loc.remove_calls.__doc__
    assert "3.9g" in open(os.path.join(ROOT, "das4whales_amd", "csrc", "project.hip")).read()


def test_symbols_are_declared_and_bound(loc):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d4w.h")).read(), flags=re.S)
    from das4whales_amd import _lib
    declared = set(re.findall(r"\bint\s+(d4w_project\w*)\s*\(", src))
    assert declared == set(SYMBOLS)                           # every entry point of the header, and no other
    for sym in SYMBOLS:
        assert sym in _lib.SIGNATURES and hasattr(_lib.lib, sym)
    nargs = {sym: len(re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % sym, src, flags=re.S).group(1).split(",")) for sym in SYMBOLS}
    assert {sym: len(_lib.SIGNATURES[sym][1]) for sym in SYMBOLS} == nargs


def test_limits(loc):
    max_calls, max_length, channels = loc.project_limits()
    assert max_calls >= 64 and max_length >= 1 << 20 and channels >= 2


NCH, NS, L = 5, 64, 8
I32, F32 = np.int32, np.float32
SHARED = [dict(order=2), dict(order=True), dict(order=None), dict(order=1.5),
          dict(start=np.zeros(3, dtype=np.int64)), dict(start=np.zeros((2, 1), dtype=np.int64)), dict(start=1.5), dict(start=np.zeros(2)),
          dict(trace=np.ones((4, NS), dtype=F32)), dict(trace=np.ones(NS)), dict(trace=np.ones((NCH, 0), dtype=F32)),
          dict(next_block=np.ones((4, 9), dtype=F32)), dict(next_block=np.ones(9)), dict(fs=0.0), dict(fs=float("nan")), dict(fs=float("inf")),
          dict(c0=-1.0), dict(c0=0.0), dict(c0=float("nan")), dict(pos=np.zeros((2, 2))), dict(pos=np.zeros(4)), dict(pos=np.zeros((2, 3, 1))),
          dict(pos=np.zeros(3)), dict(cable_pos=np.zeros((NCH, 2))), dict(cable_pos=np.zeros((4, 3))), dict(pos=np.zeros((65536 * 2, 3)), start=0)]
BEAMS = [dict(beam=np.ones((2, L))), dict(beam=np.ones((3, L), dtype=F32)), dict(beam=np.ones(L, dtype=F32)), dict(beam=np.ones((2, 0), dtype=F32)),
         dict(beam=np.ones((2, L, 1), dtype=F32)),
         dict(delays=np.zeros((2, NCH), dtype=I32)), dict(delays=(np.zeros((2, NCH), dtype=I32),)),
         dict(delays=(np.zeros((2, NCH), dtype=I32), np.zeros((2, NCH)))), dict(delays=(np.zeros((2, NCH), dtype=np.int64), np.zeros((2, NCH), dtype=F32))),
         dict(delays=(np.zeros((2, NCH - 1), dtype=I32), np.zeros((2, NCH - 1), dtype=F32))),
         dict(order=0, delays=(np.zeros((2, NCH), dtype=I32), np.zeros((2, NCH), dtype=F32))), dict(order=0, delays=np.zeros((2, NCH), dtype=F32))]
BAD_PROJECT = SHARED + BEAMS + [dict(weights=np.ones(4))]
BAD_SUBTRACT = SHARED + BEAMS + [dict(amp=np.ones((2, NCH))), dict(amp=np.ones((2, NCH - 1), dtype=F32)), dict(amp=np.ones(NCH, dtype=F32)),
                                 dict(amp=np.ones((1, NCH), dtype=F32)), dict(inplace=True)]
BAD_REMOVE = SHARED + [dict(weights=np.ones(4)), dict(length=0), dict(length=-3), dict(length=1.5), dict(length=True), dict(length=None),
                       dict(length=2 ** 30 + 1), dict(min_coef=float("nan")), dict(min_coef=float("inf")), dict(min_coef=True),
                       dict(min_coef=np.zeros(2)), dict(inplace=True)]


def _id(kw):
    return "-".join("%s=%s" % (k, (str(v.dtype) + str(v.shape)) if isinstance(v, np.ndarray) else v) for k, v in kw.items()).replace(" ", "")[:60]


def _base():
    return dict(trace=np.ones((NCH, NS), dtype=F32), fs=50.0, cable_pos=np.arange(3.0 * NCH).reshape(NCH, 3), c0=1490.0, pos=np.zeros((2, 3)),
                start=np.zeros(2, dtype=np.int64))


@pytest.mark.parametrize("kw", BAD_PROJECT, ids=_id)
def test_project_calls_rejects_bad_arguments_before_any_gpu_work(loc, kw):
    """ValueError, never the RuntimeError of a missing GPU: nothing was uploaded or launched before the check."""
    with pytest.raises(ValueError):
        loc.project_calls(**{**_base(), "beam": np.ones((2, L), dtype=F32), **kw})


@pytest.mark.parametrize("kw", BAD_SUBTRACT, ids=_id)
def test_subtract_calls_rejects_bad_arguments_before_any_gpu_work(loc, kw):
    """inplace=True on a NumPy block is one of them: there is nothing to write into."""
    with pytest.raises(ValueError):
        loc.subtract_calls(**{**_base(), "beam": np.ones((2, L), dtype=F32), "amp": np.ones((2, NCH), dtype=F32), **kw})


@pytest.mark.parametrize("kw", BAD_REMOVE, ids=_id)
def test_remove_calls_rejects_bad_arguments_before_any_gpu_work(loc, kw):
    with pytest.raises(ValueError):
        loc.remove_calls(**{**_base(), "length": L, **kw})


def test_inplace_rejects_host_and_non_float32_tensors(loc):
    import torch
    base = dict(_base(), beam=np.ones((2, L), dtype=F32), amp=np.ones((2, NCH), dtype=F32), inplace=True)
    for t in (torch.ones((NCH, NS)), torch.ones((NCH, NS), dtype=torch.float64), torch.ones((NS, NCH)).t()):
        with pytest.raises(ValueError):
            loc.subtract_calls(**dict(base, trace=t))


@pytest.mark.gpu
def test_return_shapes_and_dtypes(loc):
    import torch
    cable, pos = np.arange(15.0).reshape(5, 3) * 100.0, np.array([[50.0, 0.0, 0.0], [900.0, 40.0, -10.0]])
    x, nb = np.ones((5, 64), dtype=F32), np.ones((5, 9), dtype=F32)
    beam = np.ones((2, L), dtype=F32)
    out = loc.project_calls(x, 50.0, cable, 1490.0, pos, beam, [9, 10])
    assert len(out) == 2 and all(isinstance(o, np.ndarray) and o.shape == (2, 5) and o.dtype == F32 for o in out)
    y = loc.subtract_calls(x, 50.0, cable, 1490.0, pos, beam, [9, 10], out[0])
    assert isinstance(y, np.ndarray) and y.shape == x.shape and y.dtype == F32
    y = loc.subtract_calls(x, 50.0, cable, 1490.0, pos, beam, [9, 10], out[0], next_block=nb)
    assert isinstance(y, tuple) and y[0].shape == x.shape and y[1].shape == nb.shape
    one = loc.project_calls(x, 50.0, cable, 1490.0, pos[0], beam[0], 9, order=0)                    # one call as vectors: still [1 x channel]
    assert all(o.shape == (1, 5) for o in one)
    assert loc.subtract_calls(x, 50.0, cable, 1490.0, pos[0], beam[0], 9, one[0][0], order=0).shape == x.shape
    xt = torch.from_numpy(x).cuda()
    out = loc.project_calls(xt, 50.0, cable, 1490.0, pos, beam, 9)
    assert all(o.is_cuda and o.dtype == torch.float32 for o in out)
    same = loc.subtract_calls(xt, 50.0, cable, 1490.0, pos, beam, 9, out[0], inplace=True)
    assert same is xt
    res = loc.remove_calls(x, 50.0, cable, 1490.0, pos, [9, 10], L, return_parts=True)
    assert len(res) == 4 and res[0].shape == x.shape and res[1].shape == (2, L) and res[2].shape == (2, 5) and res[3].shape == (2, 5)
    res = loc.remove_calls(x, 50.0, cable, 1490.0, pos, [9, 10], L, next_block=nb, return_parts=True)
    assert len(res) == 5 and res[1].shape == nb.shape and res[2].shape == (2, L)
    assert loc.remove_calls(x, 50.0, cable, 1490.0, pos, [9, 10], L, next_block=nb)[1].shape == nb.shape
    none = loc.project_calls(x, 50.0, cable, 1490.0, np.zeros((0, 3)), np.zeros((0, L), dtype=F32), 0)
    assert [o.shape for o in none] == [(0, 5)] * 2 and all(o.dtype == F32 for o in none)
    y = loc.subtract_calls(x, 50.0, cable, 1490.0, np.zeros((0, 3)), np.zeros((0, L), dtype=F32), 0, np.zeros((0, 5), dtype=F32))
    assert np.array_equal(y, x)
