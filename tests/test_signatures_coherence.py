"""dw.loc.coherence_limits, beam_coherence and beamform_pws: names, argument order and defaults, and every argument error as a
ValueError raised on the host -- no GPU is needed for any of it."""
import inspect

import numpy as np
import pytest

from tests.known_answers_loc import C0, make_cable


@pytest.fixture(scope="module")
def loc():
    import das4whales_amd as dw
    return dw.loc


def spec(fn):
    s = inspect.signature(fn)
    return [(p.name, p.default if p.default is not inspect.Parameter.empty else "<required>", p.kind.name) for p in s.parameters.values()]


def test_signatures(loc):
    P, K = "POSITIONAL_OR_KEYWORD", "KEYWORD_ONLY"
    assert spec(loc.coherence_limits) == []
    assert spec(loc.beam_coherence) == [
        ("trace", "<required>", P), ("fs", "<required>", P), ("cable_pos", "<required>", P), ("c0", "<required>", P), ("pos", "<required>", P),
        ("start", 0, P), ("length", None, P), ("half_window", 0, P), ("order", 1, P), ("weights", None, P), ("next_block", None, P),
        ("imag", None, P), ("next_imag", None, P), ("peak_range", None, P), ("delays", None, K)]
    assert spec(loc.beamform_pws) == [
        ("trace", "<required>", P), ("fs", "<required>", P), ("cable_pos", "<required>", P), ("c0", "<required>", P), ("pos", "<required>", P),
        ("start", 0, P), ("length", None, P), ("power", 2.0, P), ("order", 1, P), ("weights", None, P), ("next_block", None, P),
        ("imag", True, P), ("next_imag", None, P), ("delays", None, K)]
    assert loc.Coherence._fields == ("beam", "semblance", "phase", "wsum", "times", "peak", "peak_index")
    for fn in (loc.coherence_limits, loc.beam_coherence, loc.beamform_pws):
        assert fn.__doc__ and len(fn.__doc__) > 60


def test_limits(loc):
    max_calls, max_length, max_half, segment = loc.coherence_limits()
    assert (max_calls, max_length, segment) == loc.beam_limits()[:3] and max_half >= 256


def test_every_argument_error_is_a_value_error_on_the_host(loc):
    nch, ns = 5, 64
    cable = make_cable("line", nch)
    x = np.ones((nch, ns), dtype=np.float32)
    nb = np.ones((nch, 9), dtype=np.float32)
    pos = np.zeros((2, 3))
    k, f = np.zeros((2, nch), dtype=np.int32), np.zeros((2, nch), dtype=np.float32)
    Hmax = loc.coherence_limits()[2]
    nan, inf = float("nan"), float("inf")
    base = dict(trace=x, fs=50.0, cable_pos=cable, c0=C0, pos=pos)
    shared = (dict(order=2), dict(order=-1), dict(order=1.5), dict(order=True), dict(length=0), dict(length=-3), dict(length=2.5),
              dict(trace=np.ones((4, ns), dtype=np.float32)), dict(trace=np.ones(ns)), dict(next_block=np.ones((4, 9), dtype=np.float32)),
              dict(next_block=np.ones(9)), dict(fs=0.0), dict(fs=nan), dict(fs=inf), dict(c0=-1.0), dict(c0=nan), dict(pos=np.zeros((2, 2))),
              dict(pos=np.zeros(4)), dict(start=np.zeros(3, dtype=np.int64)), dict(start=np.zeros((2, 1), dtype=np.int64)), dict(start=1.5),
              dict(weights=np.ones(4)), dict(weights=-np.ones(nch)), dict(weights=np.array([1, 1, nan, 1, 1.0])),
              dict(weights=np.array([1, 1, 1, inf, 1.0])), dict(weights=np.array([1, 1, 1, 1, -1e-9])),
              dict(cable_pos=np.zeros((5, 2))), dict(delays=(k[:1], f[:1])), dict(delays=(k, f.astype(np.float64))), dict(delays=(k,)),
              dict(order=0, delays=f), dict(order=0, delays=k[:, :4]), dict(pos=np.zeros((loc.coherence_limits()[0] + 1, 3))),
              dict(imag=np.ones((nch, ns - 1), dtype=np.float32)), dict(imag=np.ones((4, ns), dtype=np.float32)), dict(imag=np.ones(ns)),
              dict(imag=x, next_imag=nb),                                                  # a next imaginary block without a next block
              dict(imag=x, next_block=nb),                                                 # a next block without its imaginary block
              dict(imag=x, next_block=nb, next_imag=nb[:, :8]), dict(imag=x, next_block=nb, next_imag=nb[:4]),
              dict(imag=True, next_block=nb, next_imag=nb))                                # imag=True forms both here
    only_coherence = (dict(half_window=-1), dict(half_window=Hmax + 1), dict(half_window=1.5), dict(half_window=None),
                      dict(next_imag=nb, next_block=nb),                                   # next_imag without imag
                      dict(peak_range=(5, 5)), dict(peak_range=(6, 5)), dict(peak_range=(-1, 3)), dict(peak_range=(0, ns + 1)),
                      dict(peak_range=(0, 10), length=8), dict(peak_range=(0.5, 3)), dict(peak_range=(1, 2, 3)), dict(peak_range=7))
    only_pws = (dict(power=-1.0), dict(power=nan), dict(power=inf), dict(imag=None), dict(imag=False))
    for fn, cases in ((loc.beam_coherence, shared + only_coherence), (loc.beamform_pws, shared + only_pws)):
        for kw in cases:
            with pytest.raises(ValueError):
                fn(**dict(base, **kw))
