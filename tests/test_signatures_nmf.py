"""The public surface of the window-normalised matched filter: the two functions of dw.detect and FileStream's argument with
their names and defaults, the C symbols in include/d4w.h, and the errors that need no GPU.  Needs the built library (the package
does not import without it), no GPU."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQ = inspect.Parameter.empty

EXPECTED = {
    "compute_nmf_correlograms": [("data", REQ), ("templates", REQ), ("center", True), ("floor", 1e-6), ("next_head", None)],
    "compute_nmf_correlogram": [("data", REQ), ("template", REQ), ("center", True), ("floor", 1e-6), ("next_head", None)],
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


def test_file_stream_argument(dw):
    p = inspect.signature(dw.stream.FileStream.__init__).parameters
    assert "nmf" in p and p["nmf"].default is None
    assert list(p)[:9] == ["self", "fs", "fmin", "fmax", "templates", "fk_mask", "halo", "prev_tail", "on_filtered"]     # the old ones, in place


def test_symbols_are_declared_and_bound(dw):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d4w.h")).read(), flags=re.S)
    from das4whales_amd import _lib
    for sym in ("d4w_nmf_max_support", "d4w_nmf_tile", "d4w_nmf_normalise_f32"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, src), sym
        assert sym in _lib.SIGNATURES and hasattr(_lib.lib, sym)
    assert _lib.lib.d4w_nmf_max_support() >= _lib.lib.d4w_xcorr_mm_max_support()


def test_errors_that_need_no_gpu(dw):
    from das4whales_amd import _lib
    x = np.zeros((2, 100))
    too_long = np.ones(_lib.lib.d4w_nmf_max_support() + 1)
    too_long[::2] = -1.0
    with pytest.raises(ValueError):
        dw.detect.compute_nmf_correlograms(x, [too_long])
    with pytest.raises(ValueError):
        dw.detect.compute_nmf_correlogram(x, too_long)
    with pytest.raises(ValueError):
        dw.detect.compute_nmf_correlograms(x[0], [np.array([1.0, -1.0])])
    with pytest.raises(ValueError):
        dw.detect.compute_nmf_correlogram(x[0], np.array([1.0, -1.0]))
    with pytest.raises(ValueError):
        dw.detect.compute_nmf_correlograms(x, [np.zeros(5)])
    with pytest.raises(ValueError):
        dw.detect.compute_nmf_correlograms(x, [np.array([1.0, -1.0])], floor=-1.0)
