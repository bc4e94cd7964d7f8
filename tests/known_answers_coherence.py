"""Float64 NumPy restatement of the coherence of located calls along their moveout (csrc/coherence.hip,
dw.loc.beam_coherence): windowed semblance of the beam and phase coherence of the analytic signal.

    b = sum w v      e = sum w v^2      W = sum w      pr = sum w v / a      pi = sum w h / a      a = sqrt(v^2 + h^2)
    semblance[c, j] = sum_tau b^2 / sum_tau (W e), tau over [j - H, j + H] clipped to [0, nt); 0 where the denominator is 0
    phase[c, j]     = sqrt(pr^2 + pi^2) / W; 0 where W is 0
over the channels with w != 0 whose taps all lie inside the record, v and h interpolated as the beam's terms
(known_answers_beam).  Like beam_ref it takes the delay tables as input, so the sums are compared, not the tables.

Tolerances, derived and not measured.  u = 2^-24, n the contributing channels of an element, and per term
a_v = sum over taps |l_j| |x[q + j]| >= |v| (a_h likewise on the imaginary block).

  beam      db = (n + 16) u A, A = sum w a_v: known_answers_beam's bound; a term t = w v is off by at most 16 u w a_v.
  e         the kernel adds fmaf(t (1 / w), t, e).  |t^2 / w - w v^2| <= 2 |v| 16 u w a_v + (16 u)^2 w a_v^2 <= 33 u w a_v^2, the
            reciprocal, its product and the multiply-add's product are three more roundings of a value <= w a_v^2 (1 + 33 u):
            a term is off by at most 37 u w a_v^2.  The terms are >= 0, so the chain of n additions adds at most n u times the
            sum:  de = (n + C_E) u Ea,  Ea = sum w a_v^2,  C_E = 40 (37 and the slack of the second-order products).
  W         a chain of n additions of values >= 0:  dW = (n + C_W) u W,  C_W = 1.
  q = b b   dq = 2 |b| db + db^2 + u (|b| + db)^2
  d = W e   dd = W de + (e + de) dW + u (W + dW) (e + de)
  windows   sums of m = 2 H + 1 terms >= 0, a chain:  dQ = sum dq + (m - 1) u (Q + sum dq), dD likewise.
  S = Q / D dS = (dQ + S dD) / (D - dD) + u S   (infinite where dD >= D > 0: the cases assert that it stays under 1e-4).
  Where D = 0 in float64 every contributing sample is exactly 0 or nothing contributes: the kernel's D is 0 too, S = 0, dS = 0.

  phase     A term adds w times the unit vector of (t, th) = w (v, h) + (e1, e2), |e1| <= 16 u w a_v, |e2| <= 16 u w a_h.  For any
            vectors |x / |x| - y / |y|| <= 2 |x - y| / |x|, and it never exceeds 2: the direction is off by at most
            min(2, 32 u (a_v + a_h) / a).  Its length: two roundings under the square root (half each), v_rsq_f32 within one
            ulp (2 u), the product with w and the multiply-add's product: under C_P u = 6 u.  The chain of n additions of
            values bounded by w adds at most n u W.  Per component:
              P = sum over terms w (min(2, 32 u (a_v + a_h) / a) + C_P u) + n u W
            phase = sqrt(pr^2 + pi^2) / W:  dphase = sqrt(2) P / (W - dW) + phase (dW / (W - dW) + 4 u), four roundings for the
            square, the multiply-add, the root and the division.  After the division by W this is of order (n + c) u, times
            the conditioning a_v / a of terms whose taps cancel.  (A term counts as a = 0 where the float32 t^2 + th^2 is
            below 2^-126; the bound supposes no contributing term lies between 0 and that, which no scene here has.)
"""
import numpy as np

from tests import known_answers_beam as kb

U = kb.U
C_E, C_W, C_P = 40, 1, 6


def window_sum(a, H):
    """sum over tau in [j - H, j + H] clipped, along the last axis, by explicit addition (no cumulative differences: a window
    of zeros sums to exactly 0)."""
    nt = a.shape[-1]
    pad = np.zeros(a.shape[:-1] + (nt + 2 * H,))
    pad[..., H:H + nt] = a
    out = np.zeros_like(a)
    for t in range(2 * H + 1):
        out += pad[..., t:t + nt]
    return out


def coherence_ref(x, delays, order, start, nt, H, weights=None, next_block=None, imag=None, next_imag=None):
    """dict of float64 [ncalls x nt] arrays: beam, semblance, phase (None without imag), wsum, n, and the derived tolerances
    tol_beam, tol_semblance, tol_phase (None without imag), tol_wsum."""
    def record(a, b):
        a = np.asarray(a, dtype=np.float64)
        return a if b is None else np.concatenate([a, np.asarray(b, dtype=np.float64)], axis=1)
    rec = record(x, next_block)
    rim = record(imag, next_imag) if imag is not None else None
    nch, ntot = rec.shape
    if order == 0:
        k, f = np.asarray(delays, dtype=np.int64), None
    else:
        k, f = np.asarray(delays[0], dtype=np.int64), np.asarray(delays[1], dtype=np.float32)
    ncalls = k.shape[0]
    w = np.ones(nch) if weights is None else np.asarray(weights, dtype=np.float64)
    assert np.all(w >= 0) and np.all(np.isfinite(w))
    start = np.broadcast_to(np.asarray(start, dtype=np.int64), (ncalls,))
    b, A, e, Ea, W, n, pr, pi, P = (np.zeros((ncalls, nt)) for _ in range(9))
    j = np.arange(nt, dtype=np.int64)
    for c in range(ncalls):
        for ch in np.flatnonzero(w != 0):
            offs, coef = kb.coefficients(order, 0.0 if f is None else f[c, ch])
            q = int(start[c]) + j + int(k[c, ch])
            ok = (q + offs[0] >= 0) & (q + offs[-1] < ntot)
            if not ok.any():
                continue
            qq = q[ok]
            v, av, h, ah = (np.zeros(len(qq)) for _ in range(4))
            for o, l in zip(offs, coef):
                s = rec[ch, qq + o]
                v += l * s
                av += abs(l) * np.abs(s)
                if rim is not None:
                    s = rim[ch, qq + o]
                    h += l * s
                    ah += abs(l) * np.abs(s)
            b[c, ok] += w[ch] * v
            A[c, ok] += w[ch] * av
            e[c, ok] += w[ch] * v * v
            Ea[c, ok] += w[ch] * av * av
            W[c, ok] += w[ch]
            n[c, ok] += 1
            if rim is not None:
                a = np.hypot(v, h)
                live = a > 0
                aa = np.where(live, a, 1.0)
                pr[c, ok] += np.where(live, w[ch] * v / aa, 0.0)
                pi[c, ok] += np.where(live, w[ch] * h / aa, 0.0)
                P[c, ok] += np.where(live, w[ch] * (np.minimum(2.0, 32 * U * (av + ah) / aa) + C_P * U), 0.0)
    db = (n + 16) * U * A
    de = (n + C_E) * U * Ea
    dW = (n + C_W) * U * W
    qv, dv = b * b, W * e
    dq = 2 * np.abs(b) * db + db * db + U * (np.abs(b) + db) ** 2
    dd = W * de + (e + de) * dW + U * (W + dW) * (e + de)
    m = 2 * H + 1
    Q, D, sdq, sdd = (window_sum(a, H) for a in (qv, dv, dq, dd))
    dQ = sdq + (m - 1) * U * (Q + sdq)
    dD = sdd + (m - 1) * U * (D + sdd)
    live = D > 0
    S = np.where(live, Q / np.where(live, D, 1.0), 0.0)
    room = D - dD
    with np.errstate(divide="ignore", invalid="ignore"):
        dS = np.where(live, np.where(room > 0, (dQ + S * dD) / np.where(room > 0, room, 1.0), np.inf) + U * S, 0.0)
    out = dict(beam=b, semblance=S, wsum=W, n=n, tol_beam=db, tol_semblance=dS, tol_wsum=dW, phase=None, tol_phase=None)
    if rim is not None:
        P = P + n * U * W
        has = W > 0
        Wm = np.where(has, W - dW, 1.0)
        ph = np.where(has, np.hypot(pr, pi) / np.where(has, W, 1.0), 0.0)
        out["phase"] = ph
        out["tol_phase"] = np.where(has, np.sqrt(2.0) * P / Wm + ph * (dW / Wm + 4 * U), 0.0)
    return out


def first_peak(semblance, lo, hi):
    """(peak, index) per row of a float32 array: the largest value over [lo, hi) and the smallest column that attains it."""
    part = np.asarray(semblance)[:, lo:hi]
    at = np.argmax(part, axis=1)                             # the first of equals
    return part[np.arange(len(part)), at], (at + lo).astype(np.int32)
