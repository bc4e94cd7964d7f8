"""tools mirrors the three functions of the reference's tools namespace that compute something, with the reference's
parameter names, order and defaults (tests/golden/reference_signatures_tools.json, read from the reference's source with
ast: tests/golden/make_tools_signatures.py).  Out of scope, without stubs (das4whales_amd/tools.py names the reasons):
the xarray map_blocks wrappers fk_filt_chunk, fk_filt, filtfilt, filtfilt_chunk -- their arithmetic is dsp.fk_filt and
dsp.sosfiltfilt here, they return xarray objects and are inexact at chunk edges by their own account -- and the private
per-chunk helpers _energy_TimeDomain_chunk and __spec_chunk."""
import json
import os

import numpy as np

from tests.test_signatures import _params

SIGNATURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_signatures_tools.json")
MIRRORED = {"disp_comprate", "spec", "energy_TimeDomain"}
OUT_OF_SCOPE = {"fk_filt_chunk", "fk_filt", "filtfilt", "filtfilt_chunk", "_energy_TimeDomain_chunk", "__spec_chunk"}
KEYWORD_ONLY = {"energy_TimeDomain": [("chunk", None)]}


def test_tools_signatures():
    with open(SIGNATURES) as f:
        ref = json.load(f)["tools"]
    import das4whales_amd as dw
    assert "tools" in dw.__all__
    assert set(ref) == MIRRORED | OUT_OF_SCOPE
    for name in OUT_OF_SCOPE:
        assert not hasattr(dw.tools, name), "%s is out of scope: no stub" % name
        assert name in dw.tools.__doc__, "%s: the module docstring gives the reason" % name
    for name in sorted(MIRRORED):
        assert hasattr(dw.tools, name), "tools.%s is missing" % name
        pa = [tuple(p) for p in ref[name]]
        assert _params(getattr(dw.tools, name)) == pa + KEYWORD_ONLY.get(name, []), name
    import inspect
    kinds = [p.kind for p in inspect.signature(dw.tools.energy_TimeDomain).parameters.values()]
    assert kinds[-1] == inspect.Parameter.KEYWORD_ONLY and all(k == inspect.Parameter.POSITIONAL_OR_KEYWORD for k in kinds[:-1])


def test_disp_comprate_dense_ndarray(capsys):
    """The reference's three lines (tools.py:255-257) for a dense mask with known zeros: 96 x 2048 float64 values, one in
    eight of them non-zero."""
    import das4whales_amd as dw
    m = np.zeros((96, 2048))
    m[:, ::8] = 0.5
    assert dw.tools.disp_comprate(m) is None
    gib = 1024.0 ** 3
    sparse, dense = 96 * 256 * 8 / gib, 96 * 2048 * 8 / gib
    assert capsys.readouterr().out == (
        f'The size of the sparse filter is {sparse:.4f} Gib\n'
        f'The size of the dense filter is {dense:.2f} Gib\n'
        f'The compression ratio is {dense / sparse:.2f} ({abs(dense - sparse) * 100 / dense:.1f} %)\n')
    assert "The compression ratio is 8.00 (87.5 %)" in (
        f'The compression ratio is {dense / sparse:.2f} ({abs(dense - sparse) * 100 / dense:.1f} %)')


def test_disp_comprate_sparse_like(capsys):
    """Anything with .data and .todense(), as the sparse.COO the reference's designers return."""
    import das4whales_amd as dw

    class Coo:
        def __init__(self, dense):
            self._dense = dense
            self.data = dense[dense != 0]

        def todense(self):
            return self._dense

    m = np.zeros((64, 1024))
    m[:, :256] = 1.0
    dw.tools.disp_comprate(Coo(m))
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 3 and out[2] == "The compression ratio is 4.00 (75.0 %)"


def test_energy_time_dim():
    import pytest
    import das4whales_amd as dw
    with pytest.raises(ValueError):
        dw.tools.energy_TimeDomain(np.zeros((2, 10)), time_dim="distance")
