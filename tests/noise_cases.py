"""Inputs and checks shared by the noise-floor tests: tests/test_emu_noise.py (CPU emulator, C ABI on host pointers) and
tests/test_noise_gpu.py (hardware, through the package).  References: tests/known_answers_noise.py.

Bars, all derived:
  row quantiles   equal to float32(np.quantile(float64 row, q)): exactly where q (n - 1) is an integer and for the median of an
                  even row (the float64 midpoint of two floats is exact: one rounding); within one float32 ulp elsewhere
                  (two float64 evaluations of the lerp can differ in the last float64 bit); NaN exactly where the row holds one.
  env_quantiles,  |got - ref| <= 1e-5 max|env_ref| of the row: analytic_cases.TOL, the project's bar for the envelope -- order
  env_mean        statistics and the mean are 1-Lipschitz in the sup norm, so the envelope's bar carries over unchanged.
  mean_square     within 1 float32 ulp of the float64 value;  std  within 2 (float64 sums, one rounding, a root, one more).
  all-zero rows   exact zeros.
"""
import numpy as np

from tests import analytic_cases as ac
from tests import known_answers_noise as kn

LENGTHS = (1, 2, 3, 4, 5, 2047, 2048, 2049, 4097)
ROW_KINDS = ("equal", "two values", "signed zeros", "denormals", "inf", "nan", "last digit", "split middle", "duplicates",
             "normal", "magnitudes")


def quantile_sets(max_q):
    """nq = 1, 3 and max: 0, 1, 0.5 and values whose h = q (n - 1) is no integer."""
    full = [0.0, 1.0, 0.5, 0.3, 0.9, 1.0 / 3.0, 0.0137, 0.75][:max_q]
    full += [0.61] * (max_q - len(full))
    return [[0.5], [0.0, 0.37, 1.0], full]


def row(kind, n, seed=0):
    rng = np.random.default_rng(1000 * seed + n)
    if kind == "equal":
        v = np.full(n, 2.5)
    elif kind == "two values":
        v = np.where(rng.random(n) < 0.4, -1.25, 3.0)
    elif kind == "signed zeros":
        v = rng.choice([-2.0, -0.0, 0.0, 1.5, -1e-30, 1e-30], n)
    elif kind == "denormals":
        v = (rng.integers(-40, 40, n) * 1.4e-45).astype(np.float32)
    elif kind == "inf":
        v = rng.standard_normal(n)
        v[rng.integers(0, n)] = np.inf
        if n > 3:
            v[1] = -np.inf
    elif kind == "nan":
        v = rng.standard_normal(n)
        v[rng.integers(0, n)] = np.nan
    elif kind == "last digit":                                # 1 + k 2^-23: the top 22 key bits are shared
        v = (1.0 + rng.integers(0, 1024, n) * 2.0 ** -23)
    elif kind == "split middle":                              # an even row's two middle values in different top-digit bins
        lo, hi = n // 2, n - n // 2
        v = np.concatenate([rng.uniform(-3.0, -1.0, lo), rng.uniform(1e3, 1e4, hi)])
        rng.shuffle(v)
    elif kind == "duplicates":                                # copies cover both middle ranks
        v = rng.standard_normal(n)
        v[:max(2, n // 3)] = np.median(v)
        rng.shuffle(v)
    elif kind == "magnitudes":
        v = np.abs(rng.standard_normal(n)) * 3e-9
    else:
        v = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4)
    return np.ascontiguousarray(v, dtype=np.float32)


def check_quantiles(got, rows, q):
    """got [nx, nq] against np.quantile of every row (rows: [nx, n] float32)."""
    rows = np.asarray(rows, dtype=np.float32)
    n = rows.shape[1]
    ref = kn.quantiles(rows, q)
    assert got.shape == ref.shape and got.dtype == np.float32
    for j, qq in enumerate(q):
        h = qq * (n - 1)
        exact = h == np.floor(h) or (qq == 0.5 and n % 2 == 0)
        for c in range(rows.shape[0]):
            g, r = got[c, j], ref[c, j]
            if np.isnan(rows[c]).any():
                assert np.isnan(g), (c, qq, g)
            elif np.isnan(r):                                 # NumPy's lerp on infinities
                assert np.isnan(g), (c, qq, g, r)
            elif exact:
                assert g == r, (c, qq, g, r)
            else:
                assert g == r or abs(float(g) - float(r)) <= float(np.spacing(np.abs(r))), (c, qq, g, r)


NOISE_Q = (0.5, 0.1, 0.95)


def noise_block(nx, ns, seed=7):
    """analytic_cases.tone_block with rising amplitudes and one offset row, so that a row read from another row's place shows."""
    x = ac.tone_block(nx, ns, seed).astype(np.float64)
    x *= (1.0 + np.arange(nx))[:, None]
    x[0] += 0.25
    return np.ascontiguousarray(x, dtype=np.float32)


def check_noise(got, x32, q, window=None, which=(True, True, True, True)):
    """got = (mean_square, std, env_mean, env_quantiles) as float32 arrays or None where `which` is False."""
    msq, sd, em, eq, env = kn.channel_noise(x32, q, window)
    scale = np.max(env, axis=1)
    figs = {}
    if which[0]:
        u = kn.ulps(got[0], msq)
        figs["mean_square ulp"] = float(np.max(u))
        assert np.all(u <= 1.0), u
    if which[1]:
        u = kn.ulps(got[1], sd)
        figs["std ulp"] = float(np.max(u))
        assert np.all(u <= 2.0), u
    if which[2]:
        e = np.abs(got[2].astype(np.float64) - em) / scale
        figs["env_mean"] = float(np.max(e))
        assert np.all(e <= ac.TOL), e
    if which[3] and len(q):
        assert got[3].shape == eq.shape
        e = np.abs(got[3].astype(np.float64) - eq) / scale[:, None]
        figs["env_quantiles"] = float(np.max(e))
        assert np.all(e <= ac.TOL), e
    return figs


def cable_scene(seed=12, nx=64, ns=2400, fs=200.0):
    """A cable whose noise floor rises 30-fold: Gaussian noise of standard deviation 1 .. 30 along the channels, the same
    1-s 28 -> 16 Hz chirp added at 6 times each channel's noise standard deviation, then every row correlated with the
    unit-norm chirp on the host in float64 (the block a picker sees after the matched filter).  Returns (block float32
    [nx, ns], the sample of the correlation peak, the noise standard deviations)."""
    rng = np.random.default_rng(seed)
    sigma = np.linspace(1.0, 30.0, nx)
    n = int(fs)
    t = np.arange(n) / fs
    chirp = np.sin(2.0 * np.pi * (28.0 * t - 6.0 * t * t)) * np.hanning(n)
    start = 1100
    x = rng.standard_normal((nx, ns)) * sigma[:, None]
    x[:, start:start + n] += 6.0 * sigma[:, None] * chirp[None, :]
    tpl = chirp / np.linalg.norm(chirp)
    block = np.stack([np.correlate(r, tpl, "same") for r in x])
    return np.ascontiguousarray(block, dtype=np.float32), start + n // 2, sigma


def scene_facts(picks_rows, picks_one, at, nx):
    """The two facts of the scene, of any picker's result: with k times the channel's own median envelope EVERY channel has a
    pick within 2 samples of the chirp; with the reference's single 0.45 max(block) the quiet third of the cable has none."""
    hit = [len(p) > 0 and int(np.min(np.abs(np.asarray(p) - at))) <= 2 for p in picks_rows]
    quiet = [len(picks_one[c]) for c in range(nx // 3)]
    return all(hit), sum(quiet) == 0, sum(len(p) > 0 for p in picks_one)


SCENE_K = 8.0


PEAK_BARS = (0.0, -1.0, float("nan"), float("inf"), 1e3, 0.8, 2.5)


def peaks_block(nx, ns, seed=3):
    """Smoothed noise rows with plateaus (values rounded to a coarse grid), range a few units."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nx, ns + 8))
    x = np.stack([np.convolve(r, np.ones(5) / 2.0, "valid") for r in x])[:, :ns]
    x[::2] = np.round(x[::2] * 4.0) / 4.0
    return np.ascontiguousarray(x, dtype=np.float32)
