"""Float64 restatement of the per-channel noise analysis of the reference's scripts/main_bathynoise.py, which forms its
numbers inline in main() and cannot be imported:

  lines 139, 183-194   np.median(abs(sp.hilbert(trf_fk, axis=1)), axis=1), the mean of the same envelope, np.std(trf_fk, axis=1)
                       and 20 log10(std / median);
  lines 256-259        for a quiet time window: np.mean(noise**2, axis=1) and np.mean(abs(sp.hilbert(noise, axis=1)), axis=1),
                       the Hilbert transform taken of the slice.

Everything is computed in float64 on the float32 samples the kernel saw.  No figure in here comes from the code under test."""
import numpy as np
import scipy.signal as sp


def envelope(x32):
    """abs(scipy.signal.hilbert(x, axis=1)) in float64 (main_bathynoise.py:139,183,259)."""
    return np.abs(sp.hilbert(np.asarray(x32, dtype=np.float64), axis=1))


def quantiles(rows32, q):
    """np.quantile of every row in float64, default "linear" method, rounded once to float32: [nx, nq].  NumPy's warnings about
    inf - inf in rows that hold infinities are its own business."""
    r = np.asarray(rows32, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.quantile(r, np.asarray(q, dtype=np.float64), axis=1).T.astype(np.float32)


def channel_noise(x32, q=(0.5,), window=None):
    """(mean_square, std, env_mean, env_quantiles, env) in float64 ([nx], [nx], [nx], [nx, nq], [nx, ns]) of trf_fk[:, a:b]."""
    x = np.asarray(x32, dtype=np.float64)
    if window is not None:
        x = x[:, window[0]:window[1]]
    env = envelope(x)
    with np.errstate(all="ignore"):
        eq = np.quantile(env, np.asarray(q, dtype=np.float64), axis=1).T if len(q) else np.zeros((x.shape[0], 0))
    return np.mean(x ** 2, axis=1), np.std(x, axis=1), np.mean(env, axis=1), eq, env


def noise_ratio_db(std, env_median):
    """20 log10(std / median) (main_bathynoise.py:194)."""
    with np.errstate(all="ignore"):
        return 20.0 * np.log10(np.asarray(std, dtype=np.float64) / np.asarray(env_median, dtype=np.float64))


def ulps(got32, ref64):
    """|got - ref| in units of the float32 spacing at ref (0 where got == float32(ref), infinities and zeros included, and
    where both are NaN; NaN where only one is)."""
    got = np.asarray(got32, dtype=np.float32)
    ref64 = np.asarray(ref64, dtype=np.float64)
    ref = ref64.astype(np.float32)
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    with np.errstate(all="ignore"):
        d = np.abs(got.astype(np.float64) - ref64) / np.spacing(np.abs(ref)).astype(np.float64)
    return np.where(same, 0.0, d)


def find_peaks_rows(block, bars):
    """scipy.signal.find_peaks(row.astype(float64), prominence=bar)[0] row by row."""
    with np.errstate(all="ignore"):
        return [sp.find_peaks(np.asarray(r, dtype=np.float64), prominence=float(b))[0] for r, b in zip(block, bars)]
