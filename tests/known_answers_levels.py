"""Float64 NumPy restatement of the received levels (csrc/levels.hip, dw.loc.received_levels).

For call c and channel ch with w[ch] != 0 and n0 = start[c] + r[c, ch] (start clamped to +-2^62):
    signal window [n0, n0 + L), noise window [n0 - gap - N, n0 - gap); a window is valid iff it lies wholly inside the record
    (the block, and the next block behind it); N = 0: no noise window
    signal = mean of x^2 over the signal window, noise = mean of x^2 over the noise window, peak = max |x| over the signal window
    NaN for an invalid window; a NaN sample makes its window's mean square NaN; peak is NaN wherever signal is.
A channel of weight 0 is all NaN.  The restatement takes the rounded delay table r as input.

Tolerance (derived, not measured): every term is non-negative, every step of a chain and of the pairwise tree is one rounding
(fewer than L of them on the way of any term), the square is fused and the division is one more, so
    |signal - ref| <= (L + 8) 2^-24 ref        |noise - ref| <= (N + 8) 2^-24 ref
(the 8 covers the division, the rounding of (float)L and the second-order terms).  peak is exact.  NaN exactly where the
definition says; an entry whose reference is 0 must be exactly 0.
"""
from types import SimpleNamespace

import numpy as np

from tests.known_answers_align import first_samples

U = 2.0 ** -24


def levels_ref(x, r, start, L, gap, N, weights=None, next_block=None):
    """signal, noise, peak float64 [ncalls x nch] with their tolerances tol_signal, tol_noise, the flags valid_signal and
    valid_noise (the window lies inside the record, on a live channel) and n0."""
    x = np.asarray(x, dtype=np.float64)
    rec = x if next_block is None else np.concatenate([x, np.asarray(next_block, dtype=np.float64)], axis=1)
    nch, ntot = rec.shape
    r = np.asarray(r)
    ncalls = r.shape[0]
    w = np.ones(nch) if weights is None else np.asarray(weights, dtype=np.float64)
    n0 = first_samples(start, r)
    signal, noise, peak = (np.full((ncalls, nch), np.nan) for _ in range(3))
    vs, vq = np.zeros((ncalls, nch), dtype=bool), np.zeros((ncalls, nch), dtype=bool)
    with np.errstate(all="ignore"):
        for c in range(ncalls):
            for ch in np.flatnonzero(w != 0):
                a = n0[c, ch]
                if a >= 0 and a + L <= ntot:
                    seg = rec[ch, a:a + L]
                    vs[c, ch] = True
                    signal[c, ch] = float((seg * seg).sum()) / L
                    peak[c, ch] = np.nan if np.isnan(signal[c, ch]) else float(np.abs(seg).max())
                q = a - gap - N
                if N >= 1 and q >= 0 and q + N <= ntot:
                    seg = rec[ch, q:q + N]
                    vq[c, ch] = True
                    noise[c, ch] = float((seg * seg).sum()) / N
    return SimpleNamespace(signal=signal, noise=noise, peak=peak, tol_signal=(L + 8) * U * signal, tol_noise=(N + 8) * U * noise,
                           valid_signal=vs, valid_noise=vq, n0=n0, L=L, N=N, gap=gap)


def same(a, b):
    """Bit for bit, a NaN equal to a NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    na, nb = np.isnan(a), np.isnan(b)
    bits = "u%d" % a.dtype.itemsize
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(bits), b[~nb].view(bits)))


def _ratio(got, ref, tol):
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, (got.dtype, got.shape)
    gone = np.isnan(ref)
    assert np.array_equal(np.isnan(got), gone)
    zero = ~gone & (ref == 0)
    assert not got[zero].any()
    live = ~gone & ~zero
    if not live.any():
        return 0.0
    return float((np.abs(got.astype(np.float64) - ref)[live] / tol[live]).max())


def worst_ratio(got, ref):
    """Checks (signal, noise, peak) against the restatement: NaN exactly where the restatement is NaN, 0 exactly where it is 0,
    peak exactly, signal and noise within the derived tolerance.  Returns the largest error / tolerance (0 without a live entry)."""
    signal, noise, peak = got
    peak = np.asarray(peak)
    assert peak.dtype == np.float32 and same(peak.astype(np.float64), ref.peak)
    return max(_ratio(signal, ref.signal, ref.tol_signal), _ratio(noise, ref.noise, ref.tol_noise))
