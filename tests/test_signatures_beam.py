"""The public surface of the delay-and-sum beam: the two functions of dw.loc with their parameter names and defaults, their
argument checks (which run on the host before any device work, so they are tested here without a GPU), and the five C symbols
in include/d4w.h.  Needs the built library (the package does not import without it); the return shapes and dtypes need a GPU."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQ = inspect.Parameter.empty
SYMBOLS = ("d4w_beam_limits", "d4w_beam_tile", "d4w_beam_delays", "d4w_beam_ws_bytes", "d4w_beamform_f32")

EXPECTED = {
    "beam_delays": [("cable_pos", REQ), ("c0", REQ), ("fs", REQ), ("pos", REQ), ("rounded", False)],
    "beamform": [("trace", REQ), ("fs", REQ), ("cable_pos", REQ), ("c0", REQ), ("pos", REQ), ("start", 0), ("length", None), ("order", 1),
                 ("weights", None), ("normalize", False), ("next_block", None)],
}
KEYWORD_ONLY = {"beamform": [("delays", None)]}                # the tables a caller kept, by keyword only


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
    declared = set(re.findall(r"\bint\s+(d4w_beam\w*)\s*\(", src))
    assert declared == set(SYMBOLS)                           # every entry point of the header, and no other
    for sym in SYMBOLS:
        assert sym in _lib.SIGNATURES and hasattr(_lib.lib, sym)
    nargs = {sym: len(re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % sym, src, flags=re.S).group(1).split(",")) for sym in SYMBOLS}
    assert {sym: len(_lib.SIGNATURES[sym][1]) for sym in SYMBOLS} == nargs


def test_limits(loc):
    max_calls, max_length, segment, tile = loc.beam_limits()
    assert max_calls >= 64 and max_length >= 120000 and segment >= 2 and tile >= 64


BAD = [dict(order=2), dict(order=-1), dict(order=1.5), dict(order=True), dict(length=0), dict(length=-3), dict(length=2.5),
       dict(trace=np.ones((4, 64), dtype=np.float32)), dict(trace=np.ones(64)), dict(trace=np.ones((5, 0), dtype=np.float32)),
       dict(next_block=np.ones((4, 9), dtype=np.float32)), dict(next_block=np.ones(9)), dict(fs=0.0), dict(fs=float("nan")), dict(fs=float("inf")),
       dict(c0=-1.0), dict(c0=0.0), dict(c0=float("nan")), dict(pos=np.zeros((2, 2))), dict(pos=np.zeros(4)), dict(pos=np.zeros((2, 3, 1))),
       dict(start=np.zeros(3, dtype=np.int64)), dict(start=np.zeros((2, 1), dtype=np.int64)), dict(start=1.5), dict(start=np.zeros(2)),
       dict(weights=np.ones(4)), dict(cable_pos=np.zeros((5, 2))), dict(cable_pos=np.zeros((4, 3))),
       dict(delays=(np.zeros((1, 5), dtype=np.int32), np.zeros((1, 5), dtype=np.float32))),
       dict(delays=(np.zeros((2, 5), dtype=np.int32), np.zeros((2, 5), dtype=np.float64))),
       dict(delays=(np.zeros((2, 5), dtype=np.int64), np.zeros((2, 5), dtype=np.float32))), dict(delays=(np.zeros((2, 5), dtype=np.int32),)),
       dict(order=0, delays=np.zeros((2, 5), dtype=np.float32)), dict(order=0, delays=np.zeros((2, 4), dtype=np.int32)),
       dict(pos=np.zeros((65536 * 2, 3))),
       # length goes through the one whole-number check of the module: no infinity, no array, no bool
       dict(length=float("inf")), dict(length=np.ones(2)), dict(length=True)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "-".join("%s" % k for k in kw))
def test_beamform_rejects_bad_arguments_before_any_gpu_work(loc, kw):
    """ValueError, never the RuntimeError of a missing GPU: nothing was uploaded or launched before the check."""
    base = dict(trace=np.ones((5, 64), dtype=np.float32), fs=50.0, cable_pos=np.arange(15.0).reshape(5, 3), c0=1490.0, pos=np.zeros((2, 3)))
    with pytest.raises(ValueError):
        loc.beamform(**dict(base, **kw))


@pytest.mark.parametrize("kw", [dict(fs=0.0), dict(fs=float("nan")), dict(c0=float("inf")), dict(c0=-3.0), dict(pos=np.zeros((2, 2))),
                                dict(pos=np.zeros(2)), dict(cable_pos=np.zeros((5, 2))), dict(cable_pos=np.zeros(3))],
                         ids=lambda kw: "-".join("%s" % k for k in kw))
def test_beam_delays_rejects_bad_arguments_before_any_gpu_work(loc, kw):
    base = dict(cable_pos=np.arange(15.0).reshape(5, 3), c0=1490.0, fs=50.0, pos=np.zeros((2, 3)))
    with pytest.raises(ValueError):
        loc.beam_delays(**dict(base, **kw))


@pytest.mark.gpu
def test_return_shapes_and_dtypes(loc):
    import torch
    cable, pos = np.arange(15.0).reshape(5, 3) * 100.0, np.array([[50.0, 0.0, 0.0], [900.0, 40.0, -10.0]])
    x = np.ones((5, 64), dtype=np.float32)
    k, f = loc.beam_delays(cable, 1490.0, 50.0, pos)
    r = loc.beam_delays(cable, 1490.0, 50.0, pos, rounded=True)
    assert (k.shape, k.dtype, f.shape, f.dtype, r.shape, r.dtype) == ((2, 5), np.int32, (2, 5), np.float32, (2, 5), np.int32)
    for order in (0, 1, 3):
        beam, times = loc.beamform(x, 50.0, cable, 1490.0, pos, start=[3, -4], length=40, order=order)
        assert isinstance(beam, np.ndarray) and (beam.shape, beam.dtype, times.shape, times.dtype) == ((2, 40), np.float32, (2, 40), np.float64)
        assert times[1, 0] == -4 / 50.0 and times[0, 39] == 42 / 50.0
    beam, times = loc.beamform(torch.from_numpy(x).cuda(), 50.0, cable, 1490.0, pos)
    assert beam.is_cuda and times.is_cuda and (tuple(beam.shape), beam.dtype, tuple(times.shape), times.dtype) == ((2, 64), torch.float32, (2, 64), torch.float64)
    beam, times = loc.beamform(x, 50.0, cable, 1490.0, np.zeros((0, 3)), length=9)
    assert (beam.shape, beam.dtype, times.shape, times.dtype) == ((0, 9), np.float32, (0, 9), np.float64)
