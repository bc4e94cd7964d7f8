"""The public surface of the local slant-stack semblance: the two functions of dw.detect with their names and defaults, the C
symbols in include/d4w.h, the limits, and the errors that are raised before any GPU work.  Needs the built library (the package
does not import without it), no GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQ = inspect.Parameter.empty

EXPECTED = {
    "slowness_delays": [("slowness", REQ), ("dx", REQ), ("fs", REQ), ("half_aperture", REQ)],
    "local_semblance": [("data", REQ), ("delays", REQ), ("half_window", REQ), ("weights", None), ("return_all", False)],
}


@pytest.fixture(scope="module")
def dw():
    if not os.path.exists(os.path.join(ROOT, "das4whales_amd", "lib", "libd4w.so")):
        import __graft_entry__ as ge
        ge.build()
    import das4whales_amd as dw
    return dw


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_public_signature(dw, name):
    params = list(inspect.signature(getattr(dw.detect, name)).parameters.values())
    assert [(p.name, p.default) for p in params] == EXPECTED[name]
    assert all(p.kind == p.POSITIONAL_OR_KEYWORD for p in params)
    assert getattr(dw.detect, name).__doc__


def test_docstring_carries_the_definition_and_the_recipe(dw):
    doc = dw.detect.local_semblance.__doc__
    for piece in ("floor(d)", "v0 + f (v1 - v0)", "sum_tau b^2", "s[idx]", "1 / s[idx]", "ValueError"):
        assert piece in doc, piece


def test_symbols_are_declared_and_bound(dw):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d4w.h")).read(), flags=re.S)
    from das4whales_amd import _lib
    for sym in ("d4w_semblance_limits", "d4w_semblance_tile", "d4w_semblance_f32"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, src), sym
        assert sym in _lib.SIGNATURES and hasattr(_lib.lib, sym)


def test_limits_meet_the_minima(dw):
    from das4whales_amd import _lib
    v = [ctypes.c_int() for _ in range(4)]
    assert _lib.lib.d4w_semblance_limits(*[ctypes.byref(c) for c in v]) == 0
    assert v[0].value >= 16 and v[1].value >= 64 and v[2].value >= 64 and v[3].value >= 64
    assert dw.detect.semblance_limits() == {"half_aperture": v[0].value, "slownesses": v[1].value, "half_window": v[2].value,
                                            "abs_delay": v[3].value}
    tc, ts = ctypes.c_int(), ctypes.c_int()
    assert _lib.lib.d4w_semblance_tile(ctypes.byref(tc), ctypes.byref(ts)) == 0 and tc.value >= 1 and ts.value >= 1


def test_slowness_delays(dw):
    s = np.array([-1.0 / 1400.0, 0.0, 1.0 / 1500.0])
    d = dw.detect.slowness_delays(s, 2.0419, 200.0, 3)
    assert d.dtype == np.float64 and d.shape == (3, 7) and not d[:, 3].any()
    m = np.arange(-3, 4)
    assert np.array_equal(d, m[None, :] * s[:, None] * 2.0419 * 200.0)
    assert d[2, 6] > 0 > d[2, 0] and d[0, 6] < 0                        # positive slowness: later at higher channel numbers
    assert dw.detect.slowness_delays(1e-3, 2.0, 100.0, 1).shape == (1, 3)
    for bad in (dict(slowness=[]), dict(slowness=[np.nan]), dict(half_aperture=0), dict(half_aperture=1.5), dict(dx=0.0), dict(fs=-1.0),
                dict(dx=np.inf)):
        kw = dict(slowness=s, dx=2.0, fs=200.0, half_aperture=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            dw.detect.slowness_delays(**kw)


def test_errors_before_any_gpu_work(dw):
    lim = dw.detect.semblance_limits()
    x = np.zeros((4, 100), dtype=np.float32)
    d = dw.detect.slowness_delays([-1e-3, 0.0, 1e-3], 2.0, 200.0, 2)
    good = dict(data=x, delays=d, half_window=3, weights=None)

    def bad(**kw):
        a = dict(good)
        a.update(kw)
        with pytest.raises(ValueError):
            dw.detect.local_semblance(**a)

    def edit(a, at, v):
        b = np.array(a, dtype=np.float64)
        b[at] = v
        return b
    bad(data=x[0])                                                       # wrong dimensionality
    bad(data=x[None])
    bad(data=x[:, :0])
    bad(delays=d[0])
    bad(delays=d[:, :4])                                                 # an even number of columns has no centre
    bad(delays=d[:, 2:3])
    bad(delays=edit(d, (1, 2), 0.25))                                    # a non-zero centre column
    bad(delays=edit(d, (0, 0), np.nan))
    bad(delays=edit(d, (0, 0), lim["abs_delay"] + 0.5))                  # beyond the limits
    bad(delays=edit(d, (0, 4), -lim["abs_delay"] - 1e-9))
    bad(delays=np.zeros((lim["slownesses"] + 1, 5)))
    bad(delays=np.zeros((2, 2 * lim["half_aperture"] + 3)))
    bad(half_window=-1)
    bad(half_window=lim["half_window"] + 1)
    bad(half_window=2.5)
    bad(weights=[1, 1, 1, 1, -1])                                        # negative, non-finite, zero centre, wrong length
    bad(weights=[1, np.nan, 1, 1, 1])
    bad(weights=[1, 1, 1, np.inf, 1])
    bad(weights=[1, 1, 0, 1, 1])
    bad(weights=[1, 1, 1])
