"""The per-channel noise floor, row quantiles and per-channel pick thresholds on hardware, through the package: dsp.channel_noise,
dsp.row_quantile, dsp.noise_ratio_db, detect.ChannelThreshold and the pickers, against the float64 restatement of
tests/known_answers_noise.py (scripts/main_bathynoise.py:139,183-194,256-259) and SciPy's find_peaks.  Cases and bars:
tests/noise_cases.py (the CPU emulator runs the same, tests/test_emu_noise.py).  No case is skipped or excluded."""
import warnings

import numpy as np
import pytest
import torch

from tests import known_answers_noise as kn
from tests import noise_cases as nc

pytestmark = pytest.mark.gpu
NX = 5
LDS_LENGTHS = (480, 4200, 4095, 2018, 4001)          # the five LDS row paths of tests/test_analytic_modes_gpu.py
LONG_LENGTHS = (38400, 19683)


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import das4whales_amd as dw_
    return dw_


@pytest.fixture(scope="module")
def fits():
    from das4whales_amd._lib import lib
    return lambda ns: bool(lib.d4w_channel_noise_fits_lds(ns))


@pytest.fixture(scope="module")
def edge(fits):
    """The largest even row length of the one-read form."""
    return max(ns for ns in range(2, 60000, 2) if fits(ns))


def host(noise):
    return [a.cpu().numpy() if torch.is_tensor(a) else a for a in noise]


@pytest.mark.parametrize("ns", LDS_LENGTHS)
def test_channel_noise_one_read_and_long_form(dw, fits, ns):
    assert fits(ns)
    x = nc.noise_block(NX, ns)
    xd = torch.from_numpy(x).cuda()
    for how in ("one_read", "long_row", "auto"):
        got = dw.dsp.channel_noise(xd, nc.NOISE_Q, how=how)
        assert all(a.is_cuda and a.dtype == torch.float32 for a in got) and got.env_quantiles.shape == (NX, len(nc.NOISE_Q))
        print(how, ns, nc.check_noise(host(got), x, nc.NOISE_Q))
        if how == "one_read":
            first = got
    assert all(torch.equal(a, b) for a, b in zip(first, got))                   # auto took the one-read form


def test_channel_noise_at_the_edge_of_the_one_read_form(dw, fits, edge):
    assert fits(edge) and not fits(edge + 2) and edge >= 12000
    for ns, hows in ((edge, ("one_read", "long_row")), (edge + 2, ("auto", "long_row"))):
        x = nc.noise_block(NX, ns)
        xd = torch.from_numpy(x).cuda()
        for how in hows:
            print(how, ns, nc.check_noise(host(dw.dsp.channel_noise(xd, nc.NOISE_Q, how=how)), x, nc.NOISE_Q))
    with pytest.raises(ValueError):
        dw.dsp.channel_noise(xd, nc.NOISE_Q, how="one_read")


@pytest.mark.parametrize("ns", LONG_LENGTHS)
def test_channel_noise_long_rows(dw, fits, ns):
    assert not fits(ns) and NX * ns < 1 << 24
    x = nc.noise_block(NX, ns)
    got = dw.dsp.channel_noise(torch.from_numpy(x).cuda(), nc.NOISE_Q)
    print("auto", ns, nc.check_noise(host(got), x, nc.NOISE_Q))


@pytest.mark.parametrize("how", ("one_read", "long_row"))
def test_channel_noise_of_a_window_is_read_in_place(dw, how):
    ns = 4200
    x = nc.noise_block(NX, ns)
    xd = torch.from_numpy(x).cuda()
    for window in ((1, 481), (3, 4098), (0, ns), (2, 481)):
        got = dw.dsp.channel_noise(xd, nc.NOISE_Q, window, how=how)
        nc.check_noise(host(got), x, nc.NOISE_Q, window)
        alone = dw.dsp.channel_noise(xd[:, window[0]:window[1]].contiguous(), nc.NOISE_Q, how=how)
        assert all(torch.equal(a, b) for a, b in zip(got, alone)), window


@pytest.mark.parametrize("ns,how", ((4200, "one_read"), (4095, "one_read"), (4200, "long_row"), (38400, "auto")))
def test_channel_noise_is_deterministic_and_row_independent(dw, ns, how):
    x = torch.from_numpy(nc.noise_block(NX, ns)).cuda()
    a, b = dw.dsp.channel_noise(x, nc.NOISE_Q, how=how), dw.dsp.channel_noise(x, nc.NOISE_Q, how=how)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    for rows in (slice(1, 2), slice(3, 5)):
        part = dw.dsp.channel_noise(x[rows].contiguous(), nc.NOISE_Q, how=how)
        assert all(torch.equal(p[rows], q) for p, q in zip(a, part)), rows


def test_channel_noise_special_rows_and_containers(dw):
    ns = 480
    x = nc.noise_block(NX, ns)
    x[0] = 0.0
    x[2, 17] = np.inf
    x[3, 5] = np.nan
    for how in ("one_read", "long_row"):
        got = dw.dsp.channel_noise(x, nc.NOISE_Q, how=how)                       # NumPy in -> NumPy out
        assert all(isinstance(a, np.ndarray) and a.dtype == np.float32 for a in got)
        assert got.mean_square[0] == 0 and got.std[0] == 0 and got.env_mean[0] == 0 and np.all(got.env_quantiles[0] == 0)
        for c in (2, 3):
            assert np.isnan(got.env_mean[c]) and np.all(np.isnan(got.env_quantiles[c]))
        nc.check_noise([a[[1, 4]] for a in got], x[[1, 4]], nc.NOISE_Q)
        none = dw.dsp.channel_noise(x, (), how=how)
        assert none.env_quantiles.shape == (NX, 0) and np.array_equal(none.std, got.std, equal_nan=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with np.errstate(all="raise"):
            r = dw.dsp.noise_ratio_db(got.std, got.env_quantiles[:, 0])
            t = dw.dsp.noise_ratio_db(torch.from_numpy(got.std).cuda(), torch.from_numpy(got.env_quantiles[:, 0]).cuda())
    assert r.dtype == np.float64 and np.isnan(r[0]) and np.isnan(r[2]) and np.isfinite(r[1])
    assert t.is_cuda and t.dtype == torch.float64 and np.array_equal(t.cpu().numpy(), r, equal_nan=True)
    assert np.array_equal(r, kn.noise_ratio_db(got.std, got.env_quantiles[:, 0]), equal_nan=True)


def test_row_quantile(dw):
    mq = dw.dsp.row_quantile_limit()
    for n in nc.LENGTHS:
        rows = np.stack([nc.row(kind, n) for kind in nc.ROW_KINDS])
        rd = torch.from_numpy(rows).cuda()
        for q in nc.quantile_sets(mq):
            got = dw.dsp.row_quantile(rd, q)
            assert got.is_cuda and got.shape == (len(rows), len(q))
            nc.check_quantiles(got.cpu().numpy(), rows, q)
    big = nc.row("normal", (1 << 17) + 3)
    q = nc.quantile_sets(mq)[2]
    got = dw.dsp.row_quantile(big, q)                                            # 1-D, NumPy: one row, NumPy out
    assert isinstance(got, np.ndarray) and got.shape == (len(q),)
    nc.check_quantiles(got[None, :].astype(np.float32), big[None, :], q)
    med = dw.dsp.row_quantile(torch.from_numpy(rows).cuda(), 0.5)                # a scalar q: [nx]
    assert med.shape == (len(rows),)
    nc.check_quantiles(med.cpu().numpy()[:, None], rows, [0.5])


# ------------------------------------------------------------------------------------------
# per-channel thresholds in the pickers
# ------------------------------------------------------------------------------------------
def smooth_rows(nx, ns, seed):
    """Smooth envelopes with a few bumps per row (the regime of the detection chain), amplitudes rising along the rows."""
    rng = np.random.default_rng(seed)
    t = np.arange(ns)
    x = np.empty((nx, ns), dtype=np.float32)
    for c in range(nx):
        env = np.convolve(0.05 + 0.02 * np.abs(rng.standard_normal(ns)), np.ones(9) / 9, "same")
        for _ in range(int(rng.integers(2, 30))):
            p, w, a = rng.integers(0, ns), rng.uniform(15, 300), rng.uniform(0.2, 1.0)
            env += a * np.exp(-0.5 * ((t - p) / w) ** 2)
        x[c] = env * (1.0 + c)
    x[1] = np.round(x[1] * 40) / 40
    return x


def bars_for(x):
    """One bar per row: fractions of the row's own range, and the special values."""
    span = (x.max(axis=1) - x.min(axis=1)).astype(np.float64)
    bars = span * np.resize([0.5, 0.2, 0.05, 0.9, 0.01], len(x))
    bars[3], bars[4], bars[5], bars[6], bars[7] = 0.0, -1.0, np.nan, np.inf, 2.0 * span[7]
    return bars.astype(np.float32)


@pytest.mark.parametrize("ns", (12000, 20000))                                   # staged in LDS / swept from global memory
def test_pick_times_with_a_bar_per_channel(dw, ns):
    nx = 12
    x = smooth_rows(nx, ns, 500 + ns)
    bars = bars_for(x)
    xd, bd = torch.from_numpy(x).cuda(), torch.from_numpy(bars).cuda()
    ref = kn.find_peaks_rows(x, bars.astype(np.float64))
    assert len(ref[5]) == len(ref[6]) == len(ref[7]) == 0 and len(ref[3]) > 1024 and len(ref[4]) > 1024      # more than the first cap
    forms = (list(map(float, bars)), bars, bd, dw.detect.ChannelThreshold(1.0, bd))
    for thr in forms:
        got = dw.detect.pick_times(xd, thr)
        assert all(np.array_equal(got[c], ref[c]) for c in range(nx)), type(thr)
    half = kn.find_peaks_rows(x, 0.5 * bars.astype(np.float64))
    late = dw.detect.pick_times(xd, dw.detect.ChannelThreshold(0.5, bd), lazy=True)
    assert late._packed is None
    assert all(np.array_equal(late[c], half[c]) for c in range(nx))


@pytest.mark.parametrize("ns", (12000, 20000))
def test_pick_times_env_with_a_bar_per_channel(dw, ns):
    nx = 10
    rng = np.random.default_rng(ns)
    x = (smooth_rows(nx, ns, 600 + ns) * np.cos(0.9 * np.arange(ns))[None, :] + 0.01 * rng.standard_normal((nx, ns))).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    env = dw.dsp.envelope(xd).cpu().numpy()                                      # the envelope the picker sees
    bars = bars_for(env)
    bd = torch.from_numpy(bars).cuda()
    ref = kn.find_peaks_rows(env, bars.astype(np.float64))
    for thr in (list(map(float, bars)), bars, bd, dw.detect.ChannelThreshold(1.0, bd)):
        got = dw.detect.pick_times_env(xd, thr)
        assert all(np.array_equal(got[c], ref[c]) for c in range(nx)), type(thr)
    late = dw.detect.pick_times_env(xd, dw.detect.ChannelThreshold(1.0, bd), lazy=True)
    assert late._packed is None and all(np.array_equal(late[c], ref[c]) for c in range(nx))
    assert np.array_equal(dw.detect.process_corr(x[2], bars[2:3]), ref[2])
    par = dw.detect.pick_times_par(xd, bd)
    assert all(np.array_equal(par[c], ref[c]) for c in range(nx))


@pytest.mark.parametrize("ns", (12000, 20000))
def test_one_bar_forms_pick_what_the_unchanged_entry_points_pick(dw, ns):
    """A number and a Threshold go through d4w_find_peaks_f32 / d4w_find_peaks_dthr_f32 as before: the same picks as those two
    entry points called directly on the block."""
    from das4whales_amd import _device as dev
    from das4whales_amd._lib import check, lib
    nx, cap = 12, ns // 2 + 1
    xd = torch.from_numpy(smooth_rows(nx, ns, 700 + ns)).cuda()
    top = xd.max().reshape(1)
    thr = 0.2 * float(top.cpu()[0])
    idx = torch.empty((2, nx, cap), dtype=torch.int32, device=xd.device)
    cnt = torch.empty((2, nx), dtype=torch.int32, device=xd.device)
    check(lib.d4w_find_peaks_f32(dev.ptr(xd), nx, ns, thr, dev.ptr(idx[0]), dev.ptr(cnt[0]), cap, dev.stream_ptr(xd)))
    check(lib.d4w_find_peaks_dthr_f32(dev.ptr(xd), nx, ns, dev.ptr(top), 0.2, dev.ptr(idx[1]), dev.ptr(cnt[1]), cap, dev.stream_ptr(xd)))
    idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
    for k, got in enumerate((dw.detect.pick_times(xd, thr), dw.detect.pick_times(xd, dw.detect.Threshold(0.2, top)))):
        assert sum(len(got[c]) for c in range(nx)) > nx
        assert all(np.array_equal(got[c], idx[k, c, :cnt[k, c]]) for c in range(nx))


def test_a_cable_whose_noise_floor_rises_thirtyfold(dw):
    """64 channels x 2400 samples, noise 1 .. 30, the same chirp at 6 noise standard deviations on every channel.  For the
    float64 restatement (checked when the seed was chosen, and again here): with ChannelThreshold(8, median envelope) every
    channel yields the pick at the chirp; with the reference's single 0.45 max the quiet third of the cable yields none.  The
    same two facts hold of the GPU's result."""
    block, at, _ = nc.cable_scene()
    nx = block.shape[0]
    env = kn.envelope(block)
    med = np.median(env, axis=1)
    ref_rows = kn.find_peaks_rows(env, nc.SCENE_K * med)
    ref_one = kn.find_peaks_rows(env, [0.45 * float(block.max())] * nx)
    facts = nc.scene_facts(ref_rows, ref_one, at, nx)
    assert facts[0] and facts[1] and facts[2] > 0, facts
    xd = torch.from_numpy(block).cuda()
    noise = dw.dsp.channel_noise(xd)
    got_rows = dw.detect.pick_times_env(xd, dw.detect.ChannelThreshold(nc.SCENE_K, noise.env_quantiles[:, 0]))
    got_one = dw.detect.pick_times_env(xd, dw.detect.Threshold(0.45, dw.detect.correlogram_max(xd, on_device=True)))
    got = nc.scene_facts(list(got_rows), list(got_one), at, nx)
    assert got[0] and got[1] and got[2] > 0, got
    db = dw.dsp.noise_ratio_db(noise.std, noise.env_quantiles[:, 0])
    assert db.is_cuda and bool(torch.isfinite(db).all())
