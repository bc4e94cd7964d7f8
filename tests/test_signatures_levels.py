"""The public surface of the received levels: the four functions of dw.loc with their parameter names and defaults, the argument
checks of received_levels (which run on the host before any device work, so they are tested here without a GPU), the two host
helpers levels_db and fit_spreading on NumPy and host-tensor input, and the two C symbols in include/d4w.h.  Needs the built
library (the package does not import without it); the return shapes and dtypes of received_levels need a GPU."""
import inspect
import os
import re
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQ = inspect.Parameter.empty
SYMBOLS = ("d4w_level_limits", "d4w_level_f32")

EXPECTED = {
    "level_limits": [],
    "received_levels": [("trace", REQ), ("fs", REQ), ("cable_pos", REQ), ("c0", REQ), ("pos", REQ), ("start", REQ), ("length", REQ),
                        ("noise_length", 0), ("gap", 0), ("weights", None), ("next_block", None)],
    "levels_db": [("signal", REQ), ("noise", None)],
    "fit_spreading": [("level_db", REQ), ("cable_pos", REQ), ("pos", REQ), ("snr_db", None), ("min_snr_db", None)],
}
KEYWORD_ONLY = {"received_levels": [("delays", None)]}         # the table a caller kept, by keyword only


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


def test_docstrings_say_what_the_level_is(loc):
    assert "relative level" in loc.fit_spreading.__doc__ and "1 uPa" in loc.fit_spreading.__doc__
    assert "never read" in loc.received_levels.__doc__ and "3.9f" in open(os.path.join(ROOT, "das4whales_amd", "csrc", "levels.hip")).read()


def test_symbols_are_declared_and_bound(loc):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d4w.h")).read(), flags=re.S)
    from das4whales_amd import _lib
    declared = set(re.findall(r"\bint\s+(d4w_level\w*)\s*\(", src))
    assert declared == set(SYMBOLS)                           # every entry point of the header, and no other
    for sym in SYMBOLS:
        assert sym in _lib.SIGNATURES and hasattr(_lib.lib, sym)
    nargs = {sym: len(re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % sym, src, flags=re.S).group(1).split(",")) for sym in SYMBOLS}
    assert {sym: len(_lib.SIGNATURES[sym][1]) for sym in SYMBOLS} == nargs


def test_limits(loc):
    max_calls, max_length, channels = loc.level_limits()
    assert max_calls >= 64 and max_length >= 1 << 20 and channels >= 2


NCH, NS = 5, 64
I32, F32 = np.int32, np.float32
BAD = [dict(length=0), dict(length=-3), dict(length=1.5), dict(length=True), dict(length=None), dict(length=float("nan")), dict(length=float("inf")),
       dict(length=np.array([8, 8])), dict(length=2 ** 30 + 1),
       dict(noise_length=-1), dict(noise_length=0.5), dict(noise_length=True), dict(noise_length=None), dict(noise_length=2 ** 30 + 1),
       dict(gap=-1), dict(gap=2.5), dict(gap=False), dict(gap=float("nan")), dict(gap=2 ** 30, noise_length=1),
       dict(start=np.zeros(3, dtype=np.int64)), dict(start=np.zeros((2, 1), dtype=np.int64)), dict(start=1.5), dict(start=np.zeros(2)),
       dict(delays=np.zeros((2, NCH), dtype=F32)), dict(delays=np.zeros((2, NCH), dtype=np.int64)), dict(delays=np.zeros((1, NCH), dtype=I32)),
       dict(delays=np.zeros((2, NCH - 1), dtype=I32)),
       dict(trace=np.ones((4, NS), dtype=F32)), dict(trace=np.ones(NS)), dict(trace=np.ones((NCH, 0), dtype=F32)),
       dict(next_block=np.ones((4, 9), dtype=F32)), dict(next_block=np.ones(9)), dict(fs=0.0), dict(fs=float("nan")), dict(fs=float("inf")),
       dict(c0=-1.0), dict(c0=0.0), dict(c0=float("nan")), dict(pos=np.zeros((2, 2))), dict(pos=np.zeros(4)), dict(pos=np.zeros((2, 3, 1))),
       dict(pos=np.zeros(3)), dict(weights=np.ones(4)), dict(cable_pos=np.zeros((NCH, 2))), dict(cable_pos=np.zeros((4, 3))),
       dict(pos=np.zeros((65536 * 2, 3)), start=0)]


def _id(kw):
    return "-".join("%s=%s" % (k, (str(v.dtype) + str(v.shape)) if isinstance(v, np.ndarray) else v) for k, v in kw.items()).replace(" ", "")[:60]


@pytest.mark.parametrize("kw", BAD, ids=_id)
def test_received_levels_rejects_bad_arguments_before_any_gpu_work(loc, kw):
    """ValueError, never the RuntimeError of a missing GPU: nothing was uploaded or launched before the check."""
    base = dict(trace=np.ones((NCH, NS), dtype=F32), fs=50.0, cable_pos=np.arange(3.0 * NCH).reshape(NCH, 3), c0=1490.0, pos=np.zeros((2, 3)),
                start=np.zeros(2, dtype=np.int64), length=8, noise_length=4, gap=1)
    with pytest.raises(ValueError):
        loc.received_levels(**dict(base, **kw))


# ---- levels_db ---------------------------------------------------------------------------------------------------------------
def test_levels_db_is_ieee_and_silent(loc):
    inf, nan = np.inf, np.nan
    s = np.array([[1.0, 100.0, 0.0, 0.0, 4.0, nan, inf, 2.5]], dtype=F32)
    q = np.array([[1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0, nan]], dtype=F32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with np.errstate(all="raise"):                        # the function sets its own error state: nothing escapes
            lev = loc.levels_db(s)
            lev2, snr = loc.levels_db(s, q)
    assert isinstance(lev, np.ndarray) and lev.dtype == np.float64 and lev.shape == s.shape and snr.dtype == np.float64
    want = np.array([[0.0, 20.0, -inf, -inf, 10.0 * np.log10(4.0), nan, inf, 10.0 * np.log10(2.5)]])
    assert np.array_equal(lev, want, equal_nan=True) and np.array_equal(lev2, lev, equal_nan=True)
    want = np.array([[0.0, 20.0, -inf, nan, inf, nan, inf, nan]])
    assert np.array_equal(snr, want, equal_nan=True)


def test_levels_db_on_a_host_tensor_equals_numpy(loc):
    import torch
    rng = np.random.default_rng(4)
    s, q = (rng.standard_normal((3, 40)) ** 2).astype(F32), (rng.standard_normal((3, 40)) ** 2).astype(F32)
    s[0, 3], q[1, 4], s[2, 5], q[2, 5], s[1, 7] = 0.0, 0.0, 0.0, 0.0, np.nan
    lev, snr = loc.levels_db(s, q)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tl, ts = loc.levels_db(torch.from_numpy(s), torch.from_numpy(q))
        only = loc.levels_db(torch.from_numpy(s))
    assert isinstance(tl, torch.Tensor) and isinstance(ts, torch.Tensor) and tl.dtype == torch.float64 and not tl.is_cuda
    assert np.array_equal(tl.numpy(), lev, equal_nan=True) and np.array_equal(ts.numpy(), snr, equal_nan=True)
    assert isinstance(only, torch.Tensor) and np.array_equal(only.numpy(), lev, equal_nan=True)


# ---- fit_spreading -----------------------------------------------------------------------------------------------------------
def _spreading_scene(nch=40, seed=2):
    rng = np.random.default_rng(seed)
    cable = np.stack([np.linspace(0.0, 30000.0, nch), 500.0 * np.sin(np.linspace(0.0, 3.0, nch)), np.full(nch, -300.0)], axis=1)
    pos = np.array([[9000.0, -1500.0, -30.0], [21000.0, 4000.0, -60.0], [100.0, 200.0, -10.0]])
    rge = np.sqrt(((cable[None, :, :] - pos[:, None, :]) ** 2).sum(-1))
    return rng, cable, pos, rge


def test_fit_spreading_recovers_the_law(loc):
    rng, cable, pos, rge = _spreading_scene()
    SL0, k0 = np.array([180.0, 150.5, 90.25]), np.array([1.0, 1.5, 2.0])
    lev = SL0[:, None] - k0[:, None] * 10.0 * np.log10(rge)
    lev[0, [0, 7, 39]] = np.nan
    lev[1, 5] = np.inf
    lev[2, 11:20] = -np.inf
    SL, k, used = loc.fit_spreading(lev, cable, pos)
    assert all(isinstance(a, np.ndarray) for a in (SL, k, used))
    assert (SL.dtype, k.dtype, used.dtype, SL.shape, k.shape, used.shape) == (np.float64, np.float64, I32, (3,), (3,), (3,))
    assert np.array_equal(used, [37, 39, 31])
    assert np.all(np.abs(SL - SL0) <= 1e-9) and np.all(np.abs(k - k0) <= 1e-9), (SL - SL0, k - k0)
    one = loc.fit_spreading(lev[1], cable, pos[1])            # one call as vectors
    assert one[0].shape == (1,) and abs(one[0][0] - SL0[1]) <= 1e-9 and abs(one[1][0] - k0[1]) <= 1e-9 and one[2][0] == 39


def test_fit_spreading_without_enough_channels_is_nan(loc):
    _, cable, pos, rge = _spreading_scene()
    lev = 100.0 - 20.0 * np.log10(rge)
    lev[0, 1:] = np.nan                                       # one channel left
    lev[1, :] = np.nan                                        # none
    SL, k, used = loc.fit_spreading(lev, cable, pos)
    assert np.array_equal(used, [1, 0, 40]) and np.isnan(SL[:2]).all() and np.isnan(k[:2]).all() and abs(k[2] - 2.0) <= 1e-9
    # equal ranges: four channels on a circle around the source
    ring = np.array([[1000.0, 0.0, -50.0], [-1000.0, 0.0, -50.0], [0.0, 1000.0, -50.0], [0.0, -1000.0, -50.0]])
    SL, k, used = loc.fit_spreading(np.array([[60.0, 61.0, 62.0, 63.0]]), ring, np.array([0.0, 0.0, -50.0]))
    assert used[0] == 4 and np.isnan(SL[0]) and np.isnan(k[0])


def test_fit_spreading_min_snr_excludes_what_it_should(loc):
    rng, cable, pos, rge = _spreading_scene()
    lev = 120.0 - 15.0 * np.log10(rge)
    snr = rng.uniform(0.0, 12.0, lev.shape)
    snr[0, 3], snr[0, 4] = 6.0, np.nan                        # at the threshold: kept; NaN: dropped
    low = snr < 6.0
    spoiled = np.where(low | np.isnan(snr), lev + 25.0, lev)  # what the threshold excludes would bend the line
    SL, k, used = loc.fit_spreading(spoiled, cable, pos, snr, min_snr_db=6)
    assert np.array_equal(used, (snr >= 6.0).sum(1)) and used[0] < 40
    assert np.all(np.abs(SL - 120.0) <= 1e-9) and np.all(np.abs(k - 1.5) <= 1e-9)
    SL2, k2, used2 = loc.fit_spreading(spoiled, cable, pos, snr)                       # no threshold: everything finite is used
    assert np.array_equal(used2, [40, 40, 40]) and np.all(np.abs(k2 - 1.5) > 1e-3)
    SL3, k3, used3 = loc.fit_spreading(spoiled, cable, pos, None, min_snr_db=6)        # no SNR: nothing to compare
    assert np.array_equal(used3, used2) and np.array_equal(k3, k2)


def test_fit_spreading_rejects_bad_shapes(loc):
    _, cable, pos, rge = _spreading_scene()
    lev = np.zeros((3, 40))
    for args, kw in (((lev[:, :39], cable, pos), {}), ((lev[:2], cable, pos), {}), ((lev, cable[:, :2], pos), {}), ((lev, cable, pos[:, :2]), {}),
                     ((lev, cable, pos), dict(snr_db=np.zeros((3, 39)))), ((lev, cable, pos), dict(snr_db=lev, min_snr_db=np.zeros(2)))):
        with pytest.raises(ValueError):
            loc.fit_spreading(*args, **kw)


def test_fit_spreading_on_a_host_tensor(loc):
    import torch
    _, cable, pos, rge = _spreading_scene()
    lev = 100.0 - 20.0 * np.log10(rge)
    SL, k, used = loc.fit_spreading(torch.from_numpy(lev), cable, pos)
    assert all(isinstance(a, torch.Tensor) and not a.is_cuda for a in (SL, k, used)) and used.dtype == torch.int32
    assert np.all(np.abs(k.numpy() - 2.0) <= 1e-9) and np.all(np.abs(SL.numpy() - 100.0) <= 1e-9)


@pytest.mark.gpu
def test_return_shapes_and_dtypes(loc):
    import torch
    cable, pos = np.arange(15.0).reshape(5, 3) * 100.0, np.array([[50.0, 0.0, 0.0], [900.0, 40.0, -10.0]])
    x = np.ones((5, 64), dtype=F32)
    out = loc.received_levels(x, 50.0, cable, 1490.0, pos, [9, 10], 8, 4, 1)
    assert all(isinstance(o, np.ndarray) and o.shape == (2, 5) and o.dtype == F32 for o in out) and len(out) == 3
    out = loc.received_levels(x, 50.0, cable, 1490.0, pos[0], 9, 8)                               # one call as a vector: still [1 x channel]
    assert all(o.shape == (1, 5) for o in out) and np.all(np.isnan(out[1]))
    out = loc.received_levels(torch.from_numpy(x).cuda(), 50.0, cable, 1490.0, pos, 9, 8, 4)
    assert all(o.is_cuda and o.dtype == torch.float32 for o in out)
    out = loc.received_levels(x, 50.0, cable, 1490.0, np.zeros((0, 3)), 0, 8)
    assert [o.shape for o in out] == [(0, 5)] * 3 and all(o.dtype == F32 for o in out)
