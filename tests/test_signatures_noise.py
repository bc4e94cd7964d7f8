"""The public surface of the noise floor and the per-channel pick thresholds: the new names of dw.dsp and dw.detect with their
parameter names and defaults, the argument checks (which run on the host before any device work, so they are tested here
without a GPU), noise_ratio_db on NumPy and host-tensor input, the C symbols in include/d4w.h, and the unchanged signatures of
the pickers.  Needs the built library (the package does not import without it)."""
import inspect
import os
import re
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQ = inspect.Parameter.empty
SYMBOLS = ("d4w_row_quantile_f32", "d4w_row_quantile_limits", "d4w_channel_noise_fits_lds", "d4w_channel_noise_ws_bytes",
           "d4w_channel_noise_f32", "d4w_find_peaks_rowthr_f32")


@pytest.fixture(scope="module")
def dw():
    if not os.path.exists(os.path.join(ROOT, "das4whales_amd", "lib", "libd4w.so")):
        import __graft_entry__ as ge
        ge.build()
    import das4whales_amd
    return das4whales_amd


def params(fn):
    return [(p.name, p.default, p.kind) for p in inspect.signature(fn).parameters.values()]


def test_public_signatures(dw):
    PK, KW = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    assert params(dw.dsp.row_quantile) == [("x", REQ, PK), ("q", REQ, PK)]
    assert params(dw.dsp.channel_noise) == [("trace", REQ, PK), ("quantiles", (0.5,), PK), ("window", None, PK), ("how", "auto", KW)]
    assert params(dw.dsp.noise_ratio_db) == [("std", REQ, PK), ("env_median", REQ, PK)]
    assert params(dw.detect.ChannelThreshold.__init__)[1:] == [("scale", REQ, PK), ("values", REQ, PK)]
    assert dw.dsp.ChannelNoise._fields == ("mean_square", "std", "env_mean", "env_quantiles")
    for fn in (dw.dsp.row_quantile, dw.dsp.channel_noise, dw.dsp.noise_ratio_db, dw.detect.ChannelThreshold):
        assert fn.__doc__
    assert "main_bathynoise.py" in dw.dsp.channel_noise.__doc__


def test_the_pickers_keep_their_signatures(dw):
    PK = inspect.Parameter.POSITIONAL_OR_KEYWORD
    for fn in (dw.detect.pick_times, dw.detect.pick_times_env):
        assert params(fn) == [("corr_m", REQ, PK), ("threshold", REQ, PK), ("lazy", False, PK)]
    assert params(dw.detect.Threshold.__init__)[1:] == [("scale", REQ, PK), ("value", REQ, PK)]
    assert params(dw.detect.process_corr) == [("corr", REQ, PK), ("threshold", REQ, PK)]
    assert params(dw.detect.pick_times_par) == [("corr_m", REQ, PK), ("threshold", REQ, PK)]


def test_symbols_are_declared_and_bound(dw):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d4w.h")).read(), flags=re.S)
    from das4whales_amd import _lib
    declared = set(re.findall(r"\b(?:int|size_t)\s+(d4w_(?:row_quantile|channel_noise|find_peaks_rowthr)\w*)\s*\(", src))
    assert declared == set(SYMBOLS)
    for sym in SYMBOLS:
        assert sym in _lib.SIGNATURES and hasattr(_lib.lib, sym)
    nargs = {sym: len(re.search(r"\b(?:int|size_t)\s+%s\s*\((.*?)\)\s*;" % sym, src, flags=re.S).group(1).split(",")) for sym in SYMBOLS}
    assert {sym: len(_lib.SIGNATURES[sym][1]) for sym in SYMBOLS} == nargs
    # the comments cite the reference lines
    text = open(os.path.join(ROOT, "include", "d4w.h")).read()
    assert all(cite in text for cite in ("main_bathynoise.py:139", "main_bathynoise.py:256-259", "main_bathynoise.py:189"))


def test_host_only_entry_points(dw):
    """Limits and the LDS question are host arithmetic: they answer without a GPU."""
    from das4whales_amd._lib import lib
    assert dw.dsp.row_quantile_limit() >= 8
    assert lib.d4w_channel_noise_fits_lds(12000) == 1 and lib.d4w_channel_noise_fits_lds(120000) == 0
    assert lib.d4w_channel_noise_ws_bytes(10, 120000) >= 2 * 10 * 120000 * 4


X = np.ones((5, 64), dtype=np.float32)
BAD_NOISE = [dict(trace=np.ones(64, dtype=np.float32)), dict(trace=np.ones((2, 3, 4))), dict(trace=np.ones((0, 64))), dict(trace=np.ones((5, 0))),
             dict(trace=3.0), dict(window=(-1, 10)), dict(window=(10, 10)), dict(window=(12, 10)), dict(window=(0, 65)), dict(window=(64, 65)),
             dict(window=(0.5, 10)), dict(window=(3,)), dict(window=5), dict(window=(7, 8)),
             dict(quantiles=(-0.1,)), dict(quantiles=(0.5, 1.01)), dict(quantiles=(float("nan"),)), dict(quantiles=[0.5] * 9),
             dict(quantiles=[[0.5]]), dict(how="fast"), dict(how=1), dict(trace=np.ones((2, 40000), dtype=np.float32), how="one_read")]


def _id(kw):
    return "-".join("%s=%s" % (k, (str(v.dtype) + str(v.shape)) if isinstance(v, np.ndarray) else v) for k, v in kw.items()).replace(" ", "")[:50]


@pytest.mark.parametrize("kw", BAD_NOISE, ids=_id)
def test_channel_noise_rejects_bad_arguments_before_any_gpu_work(dw, kw):
    """ValueError, never the RuntimeError of a missing GPU: nothing was uploaded or launched before the check."""
    with pytest.raises(ValueError):
        dw.dsp.channel_noise(**dict(dict(trace=X), **kw))


@pytest.mark.parametrize("kw", [dict(q=-0.5), dict(q=[0.2, 1.5]), dict(q=float("nan")), dict(q=[0.5] * 9), dict(q=[]), dict(q=[[0.5]]),
                                dict(x=np.ones((2, 3, 4))), dict(x=np.ones((3, 0))), dict(x=2.0)], ids=_id)
def test_row_quantile_rejects_bad_arguments_before_any_gpu_work(dw, kw):
    with pytest.raises(ValueError):
        dw.dsp.row_quantile(**dict(dict(x=X, q=0.5), **kw))


@pytest.mark.parametrize("thr", [[1.0] * 4, np.ones(6), np.ones((5, 1)), np.ones((1, 5)), [1.0, 2.0]], ids=lambda t: str(np.shape(t)))
@pytest.mark.parametrize("picker", ["pick_times", "pick_times_env"])
def test_pickers_reject_a_wrong_count_before_any_gpu_work(dw, picker, thr):
    with pytest.raises(ValueError):
        getattr(dw.detect, picker)(X, thr)


def test_channel_threshold_wants_a_device_tensor(dw):
    import torch
    for values in (np.ones(5, dtype=np.float32), [1.0] * 5, torch.ones(5), 2.0):
        with pytest.raises(ValueError):
            dw.detect.ChannelThreshold(8.0, values)


def test_noise_ratio_db_is_ieee_and_silent(dw):
    import torch
    inf, nan = np.inf, np.nan
    s = np.array([1.0, 10.0, 0.0, 0.0, 4.0, nan, inf, 2.5], dtype=np.float32)
    m = np.array([1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0, nan], dtype=np.float32)
    want = np.array([0.0, 20.0, -inf, nan, inf, nan, inf, nan])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with np.errstate(all="raise"):
            r = dw.dsp.noise_ratio_db(s, m)
            t = dw.dsp.noise_ratio_db(torch.from_numpy(s), torch.from_numpy(m))
    assert isinstance(r, np.ndarray) and r.dtype == np.float64 and np.array_equal(r, want, equal_nan=True)
    assert isinstance(t, torch.Tensor) and not t.is_cuda and t.dtype == torch.float64 and np.array_equal(t.numpy(), want, equal_nan=True)
    from tests import known_answers_noise as kn
    assert np.array_equal(r, kn.noise_ratio_db(s, m), equal_nan=True)
