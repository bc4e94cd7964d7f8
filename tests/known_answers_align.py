"""Float64 NumPy restatement of the alignment against the beam (csrc/align.hip, dw.loc.refine_arrivals).

For call c and channel ch with w[ch] != 0, n0 = start[c] + r[c, ch] (start clamped to +-2^62) and every lag m in [-M, M]:
    valid iff the samples n0 + m .. n0 + m + L - 1 all lie inside the record (the block, and the next block behind it)
    dot[m] = sum_j t[c, j] x[ch, n0 + m + j],   en[m] = sum_j x[ch, n0 + m + j]^2,   tn[c] = sum_j t[c, j]^2
    rho[m] = dot / sqrt(tn en); 0 where the lag is valid but tn or en is 0; NaN where the lag is not valid (and where a NaN
    sample or a NaN of the template reaches it: the arithmetic's own NaN).
A channel of weight 0 is all NaN.

The restatement takes the rounded delay table r as input, so it is the correlation that is compared, not the table.  Beside
rho it returns, per entry, A = sum_j |t[j]| |x[n0 + m + j]|, tn and en.

Tolerance (derived, not measured): |rho - rho_ref| <= (L + 8) 2^-24 (A / sqrt(tn en) + |rho_ref|).  The first term covers the
L-term float32 chain of dot (any other summation order only shortens it); the second the relative errors of en and tn (L-term
chains of non-negative terms, halved by the root) and the roundings of the product, the root and the quotient.  By
Cauchy-Schwarz the bound is at most 2 (L + 8) 2^-24.  Invalid lags must be NaN exactly, zero-energy entries 0 exactly.

The pick is a function of a float32 table (pick_row, pick_table): tests apply it to the table the library returned and demand
exactly equal lag, coefficient and arrival time (the offset of the parabola enters the arrival time in float64, so an equal
time is an equal offset).  No margin rule and no excluded case are needed.
"""
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
START_MAX = 1 << 62


def first_samples(start, r):
    """n0 [ncalls x nch] as Python ints (object array): start clamped to +-2^62, plus the rounded delay."""
    r = np.asarray(r)
    start = np.broadcast_to(np.asarray(start, dtype=np.int64), (r.shape[0],))
    n0 = np.empty(r.shape, dtype=object)
    for c in range(r.shape[0]):
        s = min(max(int(start[c]), -START_MAX), START_MAX)
        for ch in range(r.shape[1]):
            n0[c, ch] = s + int(r[c, ch])
    return n0


def align_ref(x, template, r, start, M, weights=None, next_block=None):
    """rho, A, en [ncalls x nch x (2M + 1)], tn [ncalls], valid, zero (bool, same shape as rho), n0, L.  x float [nch x ns];
    template [ncalls x L]; r [ncalls x nch] ints; start [ncalls] ints."""
    x = np.asarray(x, dtype=np.float64)
    rec = x if next_block is None else np.concatenate([x, np.asarray(next_block, dtype=np.float64)], axis=1)
    nch, ntot = rec.shape
    t = np.asarray(template, dtype=np.float64)
    t = t.reshape(1, -1) if t.ndim == 1 else t
    ncalls, L = t.shape
    nl = 2 * M + 1
    w = np.ones(nch) if weights is None else np.asarray(weights, dtype=np.float64)
    n0 = first_samples(start, r)
    rho = np.full((ncalls, nch, nl), np.nan)
    A, en = np.zeros(rho.shape), np.zeros(rho.shape)
    valid, zero = np.zeros(rho.shape, dtype=bool), np.zeros(rho.shape, dtype=bool)
    with np.errstate(all="ignore"):
        tn = (t * t).sum(1)
        for c in range(ncalls):
            for ch in np.flatnonzero(w != 0):
                for i in range(nl):
                    q = n0[c, ch] + i - M
                    if q < 0 or q + L > ntot:
                        continue
                    seg = rec[ch, q:q + L]
                    valid[c, ch, i] = True
                    e = float((seg * seg).sum())
                    en[c, ch, i] = e
                    A[c, ch, i] = float((np.abs(t[c]) * np.abs(seg)).sum())
                    if tn[c] == 0 or e == 0:
                        rho[c, ch, i], zero[c, ch, i] = 0.0, True
                    else:
                        rho[c, ch, i] = float((t[c] * seg).sum()) / np.sqrt(tn[c] * e)
    return SimpleNamespace(rho=rho, A=A, en=en, tn=tn, valid=valid, zero=zero, n0=n0, L=L, M=M)


def tolerance(ref):
    """The derived bound per entry (NaN where rho_ref is NaN, 0 on zero-energy entries)."""
    with np.errstate(all="ignore"):
        scale = ref.A / np.sqrt(ref.tn[:, None, None] * ref.en)
        return np.where(ref.zero, 0.0, (ref.L + 8) * U * (scale + np.abs(ref.rho)))


def worst_ratio(rho, ref):
    """Checks the table against the restatement: NaN exactly where the restatement is NaN, 0 exactly on zero-energy entries,
    within the derived tolerance elsewhere.  Returns the largest error / tolerance (0 without a live entry)."""
    rho = np.asarray(rho)
    assert rho.dtype == np.float32 and rho.shape == ref.rho.shape, (rho.dtype, rho.shape)
    gone = np.isnan(ref.rho)
    assert np.array_equal(np.isnan(rho), gone)
    assert not rho[ref.zero].any()
    live = ~gone & ~ref.zero
    if not live.any():
        return 0.0
    err = np.abs(rho.astype(np.float64) - ref.rho)[live]
    return float((err / tolerance(ref)[live]).max())


def pick_row(row, n0, M, fs, min_coef=0.0, subsample=True):
    """The pick from one float32 row of the table: (lag, coef float32, delta, Ti).  Without a non-NaN entry: (0, NaN, 0.0, NaN)."""
    row = np.asarray(row, dtype=np.float32)
    ok = ~np.isnan(row)
    if not ok.any():
        return 0, np.float32(np.nan), 0.0, float("nan")
    best = row[ok].max()
    i = int(np.flatnonzero(ok & (row == best))[0])           # the smallest lag of equal values
    b, delta = float(row[i]), 0.0
    if subsample and 0 < i < 2 * M and ok[i - 1] and ok[i + 1]:
        a, c = float(row[i - 1]), float(row[i + 1])
        den = (a - 2.0 * b) + c
        if den < 0.0:
            delta = 0.5 * (a - c) / den
            delta = -0.5 if delta < -0.5 else delta
            delta = 0.5 if delta > 0.5 else delta
    m = i - M
    Ti = float("nan") if b < min_coef else (float(int(n0) + m) + delta) / fs
    return m, row[i], delta, Ti


def pick_table(rho, n0, M, fs, min_coef=0.0, subsample=True):
    """pick_row over a table [ncalls x nch x (2M + 1)]: (lag int32, coef float32, delta float64, Ti float64), each [ncalls x nch]."""
    ncalls, nch = rho.shape[:2]
    lag, coef = np.zeros((ncalls, nch), dtype=np.int32), np.zeros((ncalls, nch), dtype=np.float32)
    delta, Ti = np.zeros((ncalls, nch)), np.zeros((ncalls, nch))
    for c in range(ncalls):
        for ch in range(nch):
            lag[c, ch], coef[c, ch], delta[c, ch], Ti[c, ch] = pick_row(rho[c, ch], n0[c, ch], M, fs, min_coef, subsample)
    return lag, coef, delta, Ti


def same(a, b):
    """Bit for bit, a NaN equal to a NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
