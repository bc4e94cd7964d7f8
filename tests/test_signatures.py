"""The Python mirror keeps the reference's function names, parameter names and defaults (SURVEY 8(b):
"signatures to keep verbatim").  The reference's signatures are recorded in tests/golden/reference_signatures.json
(tests/golden/make_golden.py --signatures), so the test runs wherever the package imports."""
import inspect
import json
import os

import pytest

SIGNATURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_signatures.json")


def _params(fn):
    return [(p.name, "<required>" if p.default is inspect._empty else p.default)
            for p in inspect.signature(fn).parameters.values()]


@pytest.mark.parametrize("mod,complete", [("dsp", True), ("detect", True), ("improcess", False)])
def test_signatures_match_reference(mod, complete):
    with open(SIGNATURES) as f:
        ref = json.load(f)[mod]
    import das4whales_amd as dw
    om = getattr(dw, mod)
    checked = 0
    for name, params in sorted(ref.items()):
        if not hasattr(om, name):
            assert not complete, "%s.%s is missing" % (mod, name)      # improcess: only the Gabor detector's part
            continue
        pa, pb = [tuple(p) for p in params], _params(getattr(om, name))
        assert pb[:len(pa)] == pa, (mod, name, pa, pb)                 # same names, order and defaults ...
        assert all(d != "<required>" for _, d in pb[len(pa):]), (mod, name)   # ... extra parameters are optional
        checked += 1
    assert checked >= (15 if mod == "dsp" else 19 if mod == "detect" else 5)
