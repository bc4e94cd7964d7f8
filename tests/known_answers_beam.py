"""Float64 NumPy restatement of the delay-and-sum beam (csrc/beam.hip, dw.loc.beam_delays, dw.loc.beamform).

    tau[c, ch] = |cable[ch] - pos[c]| (1 / c0) fs
    beam[c, j] = sum over ch of w[ch] v(ch, start[c] + j + delay[c, ch])
      order 0: v = x[n + r];   order 1: q = n + k, v = (1 - f) x[q] + f x[q + 1];   order 3: Lagrange on x[q - 1 .. q + 2]
over the channels with w[ch] != 0 whose taps all lie inside the record (the block, and the next block behind it).

The restatement takes the delay table as input ((k, f) or r), so it is the sum that is compared, not the table.  Beside the
value it returns, per element, the number n of contributing channels and A = sum over ch |w| sum over taps |l_j| |x[q + j]|.

Tolerance (derived, not measured): |beam - ref| <= (n + 16) 2^-24 A.  n: the channel sum is a chain of n float32 additions
(split in segments, which only shortens the chains); 16 covers the float32 evaluation of the coefficients from f (at most 6
roundings each), their product with the weight and the multiply-adds of a term.  With normalize: that bound divided by the
weight sum, plus 2 x 2^-24 |ref| for the division and the rounding of the weight sum.
"""
import numpy as np

U = 2.0 ** -24
DELAY_MAX = 1 << 30


def tau(cable, c0, fs, pos):
    """float64 [ncalls x nch], the kernel's expression: the square root times the reciprocal of c0 times fs."""
    cable, pos = np.asarray(cable, dtype=np.float64), np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    dx, dy, dz = (cable[None, :, i] - pos[:, None, i] for i in range(3))
    return np.sqrt(dx * dx + dy * dy + dz * dz) * (1.0 / c0) * fs


def split(t):
    """tau -> (k int32, f float32): k = floor(tau), f = float32(tau - k), a fraction that rounds to 1.0f carried into k."""
    t = np.asarray(t, dtype=np.float64)
    k = np.floor(t)
    f = (t - k).astype(np.float32)
    carry = f >= np.float32(1.0)
    k = np.where(carry, k + 1, k)
    f = np.where(carry, np.float32(0.0), f).astype(np.float32)
    return k.astype(np.int32), f


def rounded(t):
    return np.floor(np.asarray(t, dtype=np.float64) + 0.5).astype(np.int32)


def coefficients(order, f):
    """(tap offsets, float64 coefficients) of one fraction."""
    f = float(f)
    if order == 0:
        return (0,), (1.0,)
    if order == 1:
        return (0, 1), (1.0 - f, f)
    if order == 3:
        return (-1, 0, 1, 2), (-f * (f - 1) * (f - 2) / 6, (f + 1) * (f - 1) * (f - 2) / 2, -(f + 1) * f * (f - 2) / 2, (f + 1) * f * (f - 1) / 6)
    raise ValueError(order)


def beam_ref(x, delays, order, start, nt, weights=None, normalize=False, next_block=None):
    """(ref, tol, n, A), each [ncalls x nt].  x float [nch x ns]; delays = r [ncalls x nch] for order 0, (k, f) otherwise;
    start [ncalls] ints."""
    x = np.asarray(x, dtype=np.float64)
    rec = x if next_block is None else np.concatenate([x, np.asarray(next_block, dtype=np.float64)], axis=1)
    nch, ntot = rec.shape
    if order == 0:
        k, f = np.asarray(delays, dtype=np.int64), None
    else:
        k, f = np.asarray(delays[0], dtype=np.int64), np.asarray(delays[1], dtype=np.float32)
    ncalls = k.shape[0]
    w = np.ones(nch) if weights is None else np.asarray(weights, dtype=np.float64)
    start = np.broadcast_to(np.asarray(start, dtype=np.int64), (ncalls,))
    val, A, n, wsum = (np.zeros((ncalls, nt)) for _ in range(4))
    j = np.arange(nt, dtype=np.int64)
    for c in range(ncalls):
        for ch in np.flatnonzero(w != 0):
            offs, coef = coefficients(order, 0.0 if f is None else f[c, ch])
            q = int(start[c]) + j + int(k[c, ch])
            ok = (q + offs[0] >= 0) & (q + offs[-1] < ntot)
            if not ok.any():
                continue
            qq = q[ok]
            v, a = np.zeros(len(qq)), np.zeros(len(qq))
            for o, l in zip(offs, coef):
                s = rec[ch, qq + o]
                v += l * s
                a += abs(l) * np.abs(s)
            val[c, ok] += w[ch] * v
            A[c, ok] += abs(w[ch]) * a
            n[c, ok] += 1
            wsum[c, ok] += w[ch]
    tol = (n + 16) * U * A
    if normalize:
        live = wsum != 0
        ref = np.where(live, val / np.where(live, wsum, 1.0), 0.0)
        tol = np.where(live, tol / np.where(live, np.abs(wsum), 1.0), 0.0) + 2 * U * np.abs(ref)
        return ref, tol, n, A
    return val, tol, n, A


def worst_ratio(got, ref, tol):
    """The largest |got - ref| / tol; an element of tolerance 0 must be exact (ratio 0) or counts as infinite."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    return float(ratio.max()) if ratio.size else 0.0
