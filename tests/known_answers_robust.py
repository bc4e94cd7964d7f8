"""float64 NumPy restatement for csrc/robust.hip: the robust weighted Gauss-Newton of dw.loc.solve_robust_batch, one call at a
time, as the definition reads (include/d4w.h): np.median for the scale, the rows of known_answers_loc.g_rows ("algebraic"),
the travel times of known_answers_loc.arrival_times, the normal equations formed by sequential sums over the used channels
taken in a given order and solved with np.linalg.solve.  Running it with permuted channel orders measures how far the summation
order alone moves a result; the limits of tests/robust_cases.py come from that and from nothing the kernel computes.
"""
import numpy as np

from tests.known_answers_loc import LAMBDA, arrival_times, g_rows

MAD = 1.4826
TUNING = {"l2": 1.0, "huber": 1.345, "bisquare": 4.685}


def used_channels(Ti, weights):
    """Ti is not NaN and the weight is > 0 (a NaN, zero or negative weight: not used)."""
    Ti = np.asarray(Ti, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return ~np.isnan(Ti) & (True if weights is None else np.asarray(weights, dtype=np.float64) > 0)


def robust_q(r, loss, tuning, s):
    """The robust weight of the residuals r at the scale s."""
    r = np.asarray(r, dtype=np.float64)
    if loss == "l2" or not s > 0:
        return np.ones_like(r)
    u = np.abs(r) / (tuning * s)
    with np.errstate(divide="ignore"):
        if loss == "huber":
            return np.where(u <= 1.0, 1.0, 1.0 / u)
    v = 1.0 - u * u
    return np.where(u < 1.0, v * v, 0.0)


def _sums(G, w, r):
    """(sum w g g^T, sum w g r, sum w r^2, sum w) as sequential sums in the rows' order."""
    p = G.shape[1]
    seq = lambda x: float(np.cumsum(x)[-1]) if len(x) else 0.0
    A = np.array([[seq(w * G[:, i] * G[:, k]) for k in range(p)] for i in range(p)])
    b = np.array([seq(w * G[:, i] * r) for i in range(p)])
    return A, b, seq(w * r * r), seq(w)


def solve_robust_sums(Ti, cable, c0, weights=None, loss="huber", tuning=None, scale=None, Nbiter=10, warmup=4, fix_z=False,
                      first_guess=None, order=None):
    """One call.  dict of history [Nbiter x 4], n [4], scale, robust_weights and residuals [channel] (NaN on unused channels),
    nused, gtg [p x p] (no regularisation), ssr = sum w r^2 and wsum = sum w at n.  order: a permutation of the channel
    indices in which the sums are taken (None: as given)."""
    Ti, cable = np.asarray(Ti, dtype=np.float64), np.asarray(cable, dtype=np.float64)
    nch, p = len(Ti), 3 if fix_z else 4
    tuning = TUNING[loss] if tuning is None else float(tuning)
    used = used_channels(Ti, weights)
    order = np.arange(nch) if order is None else np.asarray(order)
    keep = order[used[order]]
    w0 = np.ones(len(keep)) if weights is None else np.asarray(weights, dtype=np.float64)[keep]
    t, c = Ti[keep], cable[keep]
    out = dict(history=np.full((Nbiter, 4), np.nan), n=np.full(4, np.nan), scale=np.nan, robust_weights=np.full(nch, np.nan),
               residuals=np.full(nch, np.nan), nused=len(keep), gtg=np.zeros((p, p)), ssr=0.0, wsum=0.0)
    if not len(keep):
        return out
    n = np.array([40000.0, 23000.0, -60.0, t.min()]) if first_guess is None else np.array(first_guess, dtype=np.float64)
    idx = [0, 1, 3] if fix_z else [0, 1, 2, 3]

    def at(n, robust):
        G = g_rows(c, n, c0, fix_z, "algebraic")
        r = t - arrival_times(n[3], c, n[:3], c0)
        s = np.nan
        if robust:
            s = float(scale) if scale is not None else MAD * float(np.median(np.abs(r)))
        return G, r, s, robust_q(r, loss if robust else "l2", tuning, s)

    for j in range(Nbiter):
        G, r, s, q = at(n, loss != "l2" and j >= warmup)
        A, b, _, _ = _sums(G, w0 * q, r)
        dn = np.linalg.solve(A + LAMBDA * np.eye(p), b)
        n[idx] += (0.7 if j < 4 else 1.0) * dn
        out["history"][j] = n
    G, r, s, q = at(n, loss != "l2")
    out["gtg"], _, out["ssr"], out["wsum"] = _sums(G, w0 * q, r)
    out["n"], out["scale"] = n, s
    out["robust_weights"][keep], out["residuals"][keep] = q, r
    return out
