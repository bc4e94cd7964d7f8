"""The public surface of the STA/LTA detector: the three functions of dw.detect and FileStream's argument with their names and
defaults, the C symbols in include/d4w.h, and the argument errors that are raised before any device work.  Needs the built
library (the package does not import without it), no GPU."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQ = inspect.Parameter.empty
COMMON = [("gap", 0), ("form", "classic"), ("floor", 1e-6), ("scale", None), ("state", None), ("return_state", False)]

EXPECTED = {
    "sta_lta": [("x", REQ), ("nsta", REQ), ("nlta", REQ)] + COMMON,
    "trigger_onset": [("r", REQ), ("thr_on", REQ), ("thr_off", REQ), ("state", None), ("return_state", False)],
    "sta_lta_events": [("x", REQ), ("nsta", REQ), ("nlta", REQ), ("thr_on", REQ), ("thr_off", REQ)] + COMMON,
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
    params = [p for p in inspect.signature(getattr(dw.detect, name)).parameters.values() if not p.name.startswith("_")]
    assert [(p.name, p.default) for p in params] == EXPECTED[name]
    assert all((p.kind == p.KEYWORD_ONLY) == (p.default is not REQ) for p in params)      # the options are keyword-only
    assert getattr(dw.detect, name).__doc__


def test_classes_and_file_stream_argument(dw):
    assert issubclass(dw.detect.EventRows, dw.detect.collections.abc.Sequence)
    assert {"picks", "table", "peak", "total"} <= set(dir(dw.detect.EventRows)) and dw.detect.StaLtaState.__doc__
    p = inspect.signature(dw.stream.FileStream.__init__).parameters
    assert p["sta_lta"].default is None
    assert list(p)[:10] == ["self", "fs", "fmin", "fmax", "templates", "fk_mask", "halo", "prev_tail", "on_filtered", "nmf"]   # the old ones, in place


def test_symbols_are_declared_and_bound(dw):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d4w.h")).read(), flags=re.S)
    from das4whales_amd import _lib
    for sym in ("d4w_stalta_max_window", "d4w_stalta_tile", "d4w_stalta_f32", "d4w_trigger_onset_f32", "d4w_pack_events_i64"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, src), sym
        assert sym in _lib.SIGNATURES and hasattr(_lib.lib, sym)
    assert _lib.lib.d4w_stalta_max_window() >= 16384 and _lib.lib.d4w_stalta_tile() >= 1


def test_errors_that_need_no_gpu(dw):
    from das4whales_amd import _lib
    x = np.zeros((2, 100))
    wmax = _lib.lib.d4w_stalta_max_window()
    for a, kw in (((x, 0, 10), {}), ((x, 5, 0), {}), ((x, 5, 10), dict(gap=-1)), ((x, 5, wmax), dict(gap=1)), ((x, wmax + 1, 10), {}),
                  ((x, 5, 10), dict(floor=-1.0)), ((x, 5, 10), dict(floor=float("nan"))), ((x, 5, 10), dict(floor=float("inf"))),
                  ((x, 5, 10), dict(form="other")), ((x, 5, 10), dict(form="recursive", gap=1)), ((x[0], 5, 10), {}), ((x, 2.5, 10), {})):
        with pytest.raises(ValueError):
            dw.detect.sta_lta(*a, **kw)
        with pytest.raises(ValueError):
            dw.detect.sta_lta_events(*a, 3.0, 1.5, **kw)
    with pytest.raises(ValueError):
        dw.detect.trigger_onset(x[0], 3.0, 1.5)
    with pytest.raises(ValueError):
        dw.stream.FileStream(200.0, 15, 25, sta_lta={"nsta": 5})
    # the C ABI says why
    assert _lib.lib.d4w_stalta_f32(None, 0, 0, 0, None, 0, 0, 0, 1, 1, 0, 1e-6, None, None, None, 0, None, 0, None, None, None, None, None, None,
                                   None, 0, None) == -1
    assert len(_lib.lib.d4w_last_error()) > 0
