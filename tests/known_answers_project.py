"""Float64 NumPy restatement of the transpose of the beam (csrc/project.hip; dw.loc.project_calls, subtract_calls).

For call c and channel ch, with the delay table of the beam (r for order 0, (k, f) for orders 1 and 3), kLo .. kHi = 0 .. 0,
0 .. 1, -1 .. 2 and l_m the interpolation coefficients of f (known_answers_beam.coefficients, weight 1):
    q0 = start[c] + k[c, ch]  (start clamped to +-2^62)
    g(n) = sum_m l_m b_c[n - q0 - m],  b_c = 0 outside [0, L)            the image of the beam on the channel
    support [lo, lo + W), lo = q0 + kLo, W = L + order; valid iff it lies wholly inside the record (block + next block)
so that over the support g = convolve(b_c, l) (sample i of the support is sum_t l[t] b[i - t]).
    fit:  num = sum x g, den = sum g g, xx = sum x x over the support
          amp = num / den (0 where den = 0), coef = num / sqrt(den xx) (0 where den or xx is 0)
          NaN for an invalid window, for a channel of weight 0 and where a sample of the window is NaN (xx is NaN)
    subtraction:  y = x, then for every call, where amp[c, ch] is finite and non-zero and the window valid:
          y[ch, lo : lo + W] -= amp[c, ch] g
The restatement takes the delay table, the beam and (for the subtraction) amp as input: it is the sums that are compared.

Tolerances (derived, not measured), u = 2^-24.
  The image.  The device forms l_m in float32 (at most 6 roundings each: the differences f +- 1, f - 2, the products, the
  constant 1/6) and a sample of g as one product and up to three fmaf (at most 4 roundings on the way of a tap's term): each of
  the terms l_m b of a sample carries at most 10 relative roundings, 12 u with the second order, so
      |g_dev - g| <= 12 u G,   G = sum_m |l_m| |b|.
  The three sums run in levels.hip's order: one fmaf per term, then the pairwise tree; a term meets fewer than W inexact
  additions on its way (adding a chain that is still 0 is exact).  With the error of g inside the terms (once in x g, twice
  in g g) and 4 u for the second order, as DESIGN.md 3.9f counts its (L + 8):
      |num_dev - num| <= (W + 16) u A_num,  A_num = sum |x| G
      |den_dev - den| <= (W + 28) u A_den,  A_den = sum G^2
      |xx_dev - xx|   <= (W + 4) u xx
  (for order 0, G = |g| and these are (W + c) u sum |terms|).  The division and the square root are correctly rounded:
      amp:  num^/den^ - num/den = (dnum - amp dden) / den^, den^ >= den - tol_den, plus one rounding:
            tol_amp = (tol_num + |amp| tol_den) / (den - tol_den) + u |amp|
      coef: with rd = tol_den / den, rx = tol_xx / xx (both far below 1/2, where |1 / sqrt(1 + e) - 1| <= |e|):
            tol_coef = (tol_num / sqrt(den xx) + |coef| (rd + rx)) (1 + rd + rx) + 4 u |coef|
            (4 u: the product den xx, the square root, the division, and their second order).
  Entries whose den is 0 must be exactly 0 (a product with 0 is exact); NaN exactly where the definition says.
  Where the beam itself is only known within beam_tol (a device beam against the restatement's), E = convolve(beam_tol, |l|)
  bounds the change of g and adds sum |x| E to tol_num and sum (2 G E + E^2) to tol_den.
  The subtraction: one fmaf, one rounding, per subtracted call, of a value of at most |x| + sum |amp| G, plus the error of
  amp g: per call 12 u |amp| G (and, where amp and the beam are only known within bounds, amp_tol G + |amp| E):
      tol_y = sum over the calls that reach the sample of [12 u |amp_c| G_c + u (|x| + sum_{c' <= c} |amp_c'| G_c') (1 + 12 u)].
  A sample no call reaches is the input, bit for bit.
"""
from types import SimpleNamespace

import numpy as np

from tests.known_answers_beam import coefficients
from tests.known_answers_levels import same  # noqa: F401  (re-exported: the bit-for-bit comparison the cases use)

U = 2.0 ** -24
START_MAX = 1 << 62
CG = 12                                                      # |g_dev - g| <= CG u G


def tables(delays, order):
    """(k int64 [ncalls x nch], f float32 [ncalls x nch] or None)."""
    if order == 0:
        return np.asarray(delays, dtype=np.int64), None
    return np.asarray(delays[0], dtype=np.int64), np.asarray(delays[1], dtype=np.float32)


def support_lo(start, k, order):
    """int64 [ncalls x nch]: the first sample of every support."""
    s = np.clip(np.asarray(start, dtype=np.int64), -START_MAX, START_MAX).reshape(-1)
    return np.broadcast_to(s, (k.shape[0],))[:, None] + k + (-1 if order == 3 else 0)


def image(b, order, f, b_tol=None):
    """(g, G, E) over the support, float64 [L + order]: the image, sum |l| |b|, and the bound of its change under b_tol."""
    _, coef = coefficients(order, 0.0 if f is None else f)
    coef = np.asarray(coef, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    g = np.convolve(b, coef)
    G = np.convolve(np.abs(b), np.abs(coef))
    E = np.convolve(np.asarray(b_tol, dtype=np.float64), np.abs(coef)) if b_tol is not None else np.zeros_like(G)
    return g, G, E


def _record(x, next_block):
    x = np.asarray(x, dtype=np.float64)
    return x if next_block is None else np.concatenate([x, np.asarray(next_block, dtype=np.float64)], axis=1)


def fit_ref(x, delays, order, start, beam, weights=None, next_block=None, beam_tol=None):
    """amp, coef, num, den, xx float64 [ncalls x nch] with tol_amp, tol_coef, tol_num, tol_den, the flag valid (a valid
    window on a live channel) and lo."""
    rec = _record(x, next_block)
    nch, ntot = rec.shape
    k, f = tables(delays, order)
    ncalls = k.shape[0]
    beam = np.asarray(beam, dtype=np.float64).reshape(ncalls, -1)
    W = beam.shape[1] + order
    w = np.ones(nch) if weights is None else np.asarray(weights, dtype=np.float64)
    lo = support_lo(start, k, order)
    names = ("amp", "coef", "num", "den", "xx", "tol_amp", "tol_coef", "tol_num", "tol_den")
    o = SimpleNamespace(**{n: np.full((ncalls, nch), np.nan) for n in names})
    o.valid, o.lo, o.W = np.zeros((ncalls, nch), dtype=bool), lo, W
    with np.errstate(all="ignore"):
        for c in range(ncalls):
            for ch in np.flatnonzero(w != 0):
                a = int(lo[c, ch])
                if a < 0 or a + W > ntot:
                    continue
                o.valid[c, ch] = True
                seg = rec[ch, a:a + W]
                xx = float((seg * seg).sum())
                if np.isnan(xx):
                    continue
                g, G, E = image(beam[c], order, None if f is None else f[c, ch], None if beam_tol is None else beam_tol[c])
                num, den = float((seg * g).sum()), float((g * g).sum())
                tn = (W + 16) * U * float((np.abs(seg) * G).sum()) + float((np.abs(seg) * E).sum())
                td = (W + 28) * U * float((G * G).sum()) + float((2 * G * E + E * E).sum())
                tx = (W + 4) * U * xx
                amp = num / den if den != 0 else 0.0
                coef = num / np.sqrt(den * xx) if den != 0 and xx != 0 else 0.0
                ta = (tn + abs(amp) * td) / (den - td) + U * abs(amp) if den - td > 0 else (0.0 if den == 0 else np.inf)
                if den != 0 and xx != 0 and den - td > 0:
                    rd, rx = td / den, tx / xx
                    tc = (tn / np.sqrt(den * xx) + abs(coef) * (rd + rx)) * (1 + rd + rx) + 4 * U * abs(coef)
                else:
                    tc = 0.0 if (den == 0 or xx == 0) else np.inf
                for n, v in zip(names, (amp, coef, num, den, xx, ta, tc, tn, td)):
                    getattr(o, n)[c, ch] = v
    return o


def usable(amp):
    amp = np.asarray(amp, dtype=np.float64)
    return np.isfinite(amp) & (amp != 0)


def subtract_ref(x, delays, order, start, beam, amp, next_block=None, amp_tol=None, beam_tol=None):
    """(y float64 [nch x ntot], tol [nch x ntot], reached bool [nch x ntot]: the samples some call was subtracted from)."""
    rec = _record(x, next_block)
    nch, ntot = rec.shape
    k, f = tables(delays, order)
    ncalls = k.shape[0]
    beam = np.asarray(beam, dtype=np.float64).reshape(ncalls, -1)
    W = beam.shape[1] + order
    lo = support_lo(start, k, order)
    amp = np.asarray(amp, dtype=np.float64)
    ok = usable(amp)
    y, tol, reached = rec.copy(), np.zeros(rec.shape), np.zeros(rec.shape, dtype=bool)
    with np.errstate(all="ignore"):
        mag = np.abs(rec)
        for c in range(ncalls):
            for ch in np.flatnonzero(ok[c]):
                a = int(lo[c, ch])
                if a < 0 or a + W > ntot:
                    continue
                g, G, E = image(beam[c], order, None if f is None else f[c, ch], None if beam_tol is None else beam_tol[c])
                s = slice(a, a + W)
                y[ch, s] -= amp[c, ch] * g
                mag[ch, s] += abs(amp[c, ch]) * G
                tol[ch, s] += CG * U * abs(amp[c, ch]) * G + U * mag[ch, s] * (1 + CG * U)
                if amp_tol is not None:
                    tol[ch, s] += amp_tol[c, ch] * (G + E)
                tol[ch, s] += abs(amp[c, ch]) * E
                reached[ch, s] = True
    return y, tol, reached


def subtract_steps_f32(x, delays, order, start, beam, amp, next_block=None):
    """The subtraction step by step in float32, in increasing call order: y = float32(y - amp g) with the product and the sum
    formed in float64.  The device's bits wherever that product and that sum are exact in float64 (small integers and powers
    of two at order 0): what the call-order test compares with."""
    rec = _record(x, next_block)
    k, f = tables(delays, order)
    beam = np.asarray(beam, dtype=np.float32).reshape(k.shape[0], -1)
    W = beam.shape[1] + order
    lo = support_lo(start, k, order)
    y = rec.astype(np.float32)
    for c in range(k.shape[0]):
        for ch in np.flatnonzero(usable(amp[c])):
            a = int(lo[c, ch])
            if a < 0 or a + W > rec.shape[1]:
                continue
            g = image(beam[c], order, None if f is None else f[c, ch])[0]
            y[ch, a:a + W] = (y[ch, a:a + W].astype(np.float64) - np.float64(amp[c, ch]) * g).astype(np.float32)
    return y


def _ratio(got, ref, tol):
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, (got.dtype, got.shape)
    gone = np.isnan(ref)
    assert np.array_equal(np.isnan(got), gone)
    exact = ~gone & (tol == 0)
    assert np.array_equal(got[exact].astype(np.float64), ref[exact])
    live = ~gone & ~exact
    assert np.all(np.isfinite(tol[live]))                    # den - tol_den > 0: the bound exists for every entry
    if not live.any():
        return 0.0
    return float((np.abs(got.astype(np.float64) - ref)[live] / tol[live]).max())


def worst_fit(got, ref):
    """(amp, coef) of the device against fit_ref: NaN exactly where the restatement is NaN, exact where its tolerance is 0
    (den = 0: both 0), within the derived tolerance elsewhere.  Returns the largest error / tolerance."""
    return max(_ratio(got[0], ref.amp, ref.tol_amp), _ratio(got[1], ref.coef, ref.tol_coef))


def worst_subtract(got, y, tol, reached, given):
    """y of the device [nch x ntot] against subtract_ref: the samples no call reaches are `given` bit for bit; the others
    within the tolerance (a NaN where the restatement has one)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == y.shape
    assert same(got[~reached], np.asarray(given, dtype=np.float32)[~reached])
    gone = np.isnan(y) & reached
    assert np.array_equal(np.isnan(got) & reached, gone)
    live = reached & ~gone
    if not live.any():
        return 0.0
    err, t = np.abs(got.astype(np.float64) - y)[live], tol[live]
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(t > 0, err / t, np.where(err == 0, 0.0, np.inf)).max())
