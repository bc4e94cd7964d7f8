"""The public surface of the robust relocation: the three functions of dw.loc with their parameter names and defaults, their
argument checks (which run on the host before any device work, so they are tested here without a GPU), and the three C symbols
in include/d4w.h.  Needs the built library (the package does not import without it); the return shapes and dtypes need a GPU."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQ = inspect.Parameter.empty
SYMBOLS = ("d4w_loc_robust_limits", "d4w_loc_robust_ws_bytes", "d4w_loc_robust_f64")

EXPECTED = {
    "robust_limits": [],
    "solve_robust_batch": [("Ti", REQ), ("cable_pos", REQ), ("c0", REQ), ("weights", None), ("loss", "huber"), ("tuning", None), ("scale", None),
                           ("Nbiter", 10), ("warmup", 4), ("fix_z", False), ("first_guess", None), ("return_stats", False)],
    "relocate": [("trace", REQ), ("fs", REQ), ("cable_pos", REQ), ("c0", REQ), ("n", REQ), ("length", REQ), ("max_lag", REQ), ("lead", 0),
                 ("rounds", 1), ("order", 3), ("loss", "huber"), ("tuning", None), ("coef_power", 2.0), ("min_coef", 0.0), ("Nbiter", 10),
                 ("fix_z", True), ("weights", None), ("next_block", None), ("return_stats", False)],
}


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
    assert [(p.name, p.default) for p in params] == EXPECTED[name]
    assert all(p.kind == p.POSITIONAL_OR_KEYWORD for p in params)
    assert getattr(loc, name).__doc__


def test_docstrings_point_at_each_other(loc):
    assert "relocate(" in loc.refine_arrivals.__doc__ and "3.9e" in loc.refine_arrivals.__doc__
    doc = loc.relocate.__doc__
    at = [doc.index(name + "(") for name in ("beamform", "refine_arrivals", "solve_robust_batch")]
    assert at == sorted(at)
    doc = " ".join(loc.solve_robust_batch.__doc__.split())
    for word in ("huber", "bisquare", "1.4826", "NaN, zero or negative weight", "bit for bit"):
        assert word in doc, word


def test_symbols_are_declared_and_bound(loc):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d4w.h")).read(), flags=re.S)
    from das4whales_amd import _lib
    declared = set(re.findall(r"\bint\s+(d4w_loc_robust\w*)\s*\(", src))
    assert declared == set(SYMBOLS)
    for sym in SYMBOLS:
        assert sym in _lib.SIGNATURES and hasattr(_lib.lib, sym)
    nargs = {sym: len(re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % sym, src, flags=re.S).group(1).split(",")) for sym in SYMBOLS}
    assert {sym: len(_lib.SIGNATURES[sym][1]) for sym in SYMBOLS} == nargs


def test_limits(loc):
    from tests import robust_cases as rc
    resident, bits = loc.robust_limits()
    assert resident == rc.RESIDENT and resident >= 11020 and 1 <= bits <= 8


NCH, NC = 6, 2
BAD = [dict(loss="l1"), dict(loss=None), dict(loss=1), dict(loss="Huber"),
       dict(tuning=0.0), dict(tuning=-1.0), dict(tuning=float("nan")), dict(tuning=float("inf")), dict(tuning=np.ones(2)), dict(tuning=True),
       dict(scale=0.0), dict(scale=-1e-3), dict(scale=float("nan")), dict(scale=float("inf")), dict(scale=np.ones(NC)), dict(scale=True),
       dict(warmup=-1), dict(warmup=1.5), dict(warmup=None), dict(warmup=True), dict(warmup=float("nan")),
       dict(Nbiter=-1), dict(Nbiter=2.5), dict(Nbiter=None), dict(Nbiter=100001), dict(Nbiter=True),
       dict(weights=np.ones(NCH - 1)), dict(weights=np.ones((NC + 1, NCH))), dict(weights=np.ones((NC, NCH, 1))), dict(weights=np.ones((NCH, NC))),
       dict(weights=1.0),
       dict(Ti=np.ones(NCH)), dict(Ti=np.ones((NC, NCH + 1))), dict(Ti=np.ones((NC, NCH, 1))),
       dict(first_guess=np.zeros(3)), dict(first_guess=np.zeros((NC + 1, 4))), dict(first_guess=np.zeros((NC, 3))),
       dict(c0=0.0), dict(c0=-1.0), dict(c0=float("nan")), dict(c0=float("inf")),
       dict(cable_pos=np.zeros((NCH, 2))), dict(cable_pos=np.zeros(NCH)), dict(cable_pos=np.zeros((0, 3)))]


def _id(kw):
    return "-".join("%s=%s" % (k, (str(v.dtype) + str(v.shape)) if isinstance(v, np.ndarray) else v) for k, v in kw.items()).replace(" ", "")[:60]


@pytest.mark.parametrize("kw", BAD, ids=_id)
def test_solve_robust_batch_rejects_bad_arguments_before_any_gpu_work(loc, kw):
    """ValueError, never the RuntimeError of a missing GPU: nothing was uploaded or launched before the check."""
    base = dict(Ti=np.ones((NC, NCH)), cable_pos=np.arange(3.0 * NCH).reshape(NCH, 3), c0=1490.0)
    with pytest.raises(ValueError):
        loc.solve_robust_batch(**dict(base, **kw))


BAD_RELOCATE = [dict(rounds=0), dict(rounds=1.5), dict(rounds=True), dict(rounds=None), dict(lead=-1), dict(lead=0.5),
                dict(coef_power=-1.0), dict(coef_power=float("nan")), dict(coef_power=float("inf")), dict(coef_power=np.ones(2)),
                dict(n=np.zeros(4)), dict(n=np.zeros((2, 3))), dict(n=np.zeros((2, 4, 1))), dict(loss="l1")]


@pytest.mark.parametrize("kw", BAD_RELOCATE, ids=_id)
def test_relocate_rejects_its_own_arguments_before_any_gpu_work(loc, kw):
    base = dict(trace=np.ones((NCH, 64), dtype=np.float32), fs=50.0, cable_pos=np.arange(3.0 * NCH).reshape(NCH, 3), c0=1490.0,
                n=np.zeros((2, 4)), length=8, max_lag=2)
    with pytest.raises(ValueError):
        loc.relocate(**dict(base, **kw))


@pytest.mark.gpu
def test_return_shapes_and_dtypes(loc):
    import torch
    from tests import robust_cases as rc
    cable, Ti, srcs, _ = rc.scene(40, 3, seed=1)
    fg = srcs + [300.0, -200.0, 0.0, 0.05]
    n = loc.solve_robust_batch(Ti, cable, rc.C0, first_guess=fg)
    assert isinstance(n, np.ndarray) and (n.shape, n.dtype) == ((3, 4), np.float64)
    for fix_z, p in ((False, 4), (True, 3)):
        n, st = loc.solve_robust_batch(Ti, cable, rc.C0, fix_z=fix_z, first_guess=fg, Nbiter=7, return_stats=True)
        shapes = dict(history=(3, 7, 4), scale=(3,), robust_weights=(3, 40), residuals=(3, 40), nused=(3,), weight_sum=(3,), variance=(3,),
                      covariance=(3, p, p), uncertainty=(3, p))
        assert {k: v.shape for k, v in st.items()} == shapes and all(isinstance(v, np.ndarray) for v in st.values())
        assert np.all(st["variance"] > 0) and np.all(st["uncertainty"] > 0) and np.all(st["nused"] == 40)
    n, st = loc.solve_robust_batch(torch.from_numpy(Ti).cuda(), cable, rc.C0, first_guess=fg, return_stats=True)
    assert n.is_cuda and n.dtype == torch.float64 and all(v.is_cuda for v in st.values())
    n, st = loc.solve_robust_batch(torch.from_numpy(Ti), cable, rc.C0, first_guess=fg, return_stats=True)      # a host tensor: _back's rule
    assert not n.is_cuda and all(torch.is_tensor(v) and not v.is_cuda for v in st.values())
    n, st = loc.solve_robust_batch(np.zeros((0, 40)), cable, rc.C0, return_stats=True)
    assert n.shape == (0, 4) and st["residuals"].shape == (0, 40) and st["covariance"].shape == (0, 4, 4)
