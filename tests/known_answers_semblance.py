"""Local slant-stack semblance (csrc/semblance.hip): the definition restated in float64 NumPy, vectorised over
channels and time, and the tolerance that goes with it.  No GPU, no library: test_emu_semblance.py and test_semblance_gpu.py
compare against this.

    X(c, u) = x[c, u] inside the record, 0 outside; a neighbour c + m outside [0, nx) or of weight 0 is absent
    xi = v0 + f (v1 - v0),  v0 = X(c + m, tau + k),  v1 = X(c + m, tau + k + 1)           (k, f: split_delays, f float32)
    b = sum_m w xi,  e = sum_m w xi^2,  a = sum_m w (|v0| + |v1|),  W = sum_m w
    N = sum_tau b^2,  E = sum_tau e,  A = sum_tau a^2   over tau in [max(0, t - H), min(ns - 1, t + H)]
    S = N / (W E),  R = A / (W E)   where W E > 0, else 0          (R >= S: the absolute-value twin that scales the tolerance)
"""
import numpy as np


def split_delays(delays):
    """float64 [np, 2M + 1] delays in samples -> (k int32, f float32) with k = floor(d), f = float32(d - k), and a fraction
    that rounds to 1.0f carried into k."""
    d = np.asarray(delays, dtype=np.float64)
    k = np.floor(d)
    f = (d - k).astype(np.float32)
    carry = f >= np.float32(1.0)
    k = np.where(carry, k + 1, k)
    f = np.where(carry, np.float32(0.0), f).astype(np.float32)
    return k.astype(np.int32), f


def _window_sum(v, H):
    """sum over tau in [t - H, t + H] clipped to the record: plain sums of the terms (zeros padded at the ends), no prefixes."""
    if H == 0:
        return v.copy()
    p = np.pad(v, ((0, 0), (H, H)))
    return np.lib.stride_tricks.sliding_window_view(p, 2 * H + 1, axis=1).sum(axis=2)


def semblance_ref(x, k, f, w, H):
    """-> (S, R), float64 [np, nx, ns]."""
    x = np.asarray(x, dtype=np.float64)
    nx, ns = x.shape
    k = np.asarray(k)
    npj, n = k.shape
    M = (n - 1) // 2
    f = np.asarray(f, dtype=np.float32).astype(np.float64)
    w = np.asarray(w, dtype=np.float32).astype(np.float64)
    pad = int(np.max(np.abs(k))) + 2
    xp = np.zeros((nx + 2 * M, ns + 2 * pad))
    xp[M:M + nx, pad:pad + ns] = x
    chan = np.arange(nx)
    S = np.zeros((npj, nx, ns))
    R = np.zeros((npj, nx, ns))
    present = [(w[m + M] != 0) & (chan + m >= 0) & (chan + m < nx) for m in range(-M, M + 1)]
    W = sum(np.where(p, w[i], 0.0) for i, p in enumerate(present))
    for j in range(npj):
        b = np.zeros((nx, ns))
        e = np.zeros((nx, ns))
        a = np.zeros((nx, ns))
        for m in range(-M, M + 1):
            wm = w[m + M]
            if wm == 0:
                continue
            kk = int(k[j, m + M])
            v0 = xp[M + m:M + m + nx, pad + kk:pad + kk + ns]
            v1 = xp[M + m:M + m + nx, pad + kk + 1:pad + kk + 1 + ns]
            xi = v0 + f[j, m + M] * (v1 - v0)
            b += wm * xi                         # (rows of absent neighbours are zero rows of xp: they add nothing)
            e += wm * xi * xi
            a += wm * (np.abs(v0) + np.abs(v1))
        N, E, A = _window_sum(b * b, H), _window_sum(e, H), _window_sum(a * a, H)
        den = W[:, None] * E
        ok = den > 0
        S[j] = np.where(ok, N / np.where(ok, den, 1.0), 0.0)
        R[j] = np.where(ok, A / np.where(ok, den, 1.0), 0.0)
    return S, R


def tolerance(R, M, H):
    """|got - ref| <= K 2^-24 R with K = 2 (n + 3) + (2H + 1) + 8, n = 2M + 1: the beam's error is <= gamma_(n+3) a, the
    numerator's therefore <= 2 gamma sum a^2 plus the window sum's gamma_(2H+1) (any order of adding 2H + 1 non-negative terms),
    the denominator's is relative."""
    n = 2 * M + 1
    K = 2 * (n + 3) + (2 * H + 1) + 8
    return K * 2.0 ** -24 * R


def check_against_ref(got_coh, got_idx, got_cube, S, R, M, H):
    """The cube, coh and idx of one run against the restatement (S, R) = semblance_ref(...); no element is excluded.  Returns the
    worst error / tolerance."""
    tol = tolerance(R, M, H)
    worst = 0.0
    if got_cube is not None:
        err = np.abs(got_cube.astype(np.float64) - S)
        assert np.all(err <= tol), "cube: worst error / tol = %g" % np.max(err / np.maximum(tol, 1e-300))
        worst = float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), 0.0)))
    jref = np.argmax(S, axis=0)
    ref_max = np.take_along_axis(S, jref[None], axis=0)[0]
    gi = got_idx.astype(np.int64)
    assert got_idx.dtype == np.uint8 and gi.max() < S.shape[0]
    tol_ref = np.take_along_axis(tol, jref[None], axis=0)[0]
    tol_got = np.take_along_axis(tol, gi[None], axis=0)[0]
    ref_at_got = np.take_along_axis(S, gi[None], axis=0)[0]
    # got[idx] >= got[jref]:  ref[idx] >= got[idx] - tol[idx] >= ref_max - tol[jref] - tol[idx]   (<= the 2 tol of the issue)
    assert np.all(ref_at_got >= ref_max - (tol_ref + tol_got)), "idx names a slowness that is not the best within 2 tol"
    cerr = np.abs(got_coh.astype(np.float64) - ref_max)
    ctol = np.maximum(tol_ref, tol_got)
    assert np.all(cerr <= ctol), "coh: worst error %g" % np.max(cerr)
    assert np.all(got_coh.astype(np.float64) <= 1.0 + ctol)
    if got_cube is not None:                     # coh and idx restate the cube that was returned
        assert np.array_equal(got_coh, got_cube.max(axis=0)) and np.array_equal(gi, np.argmax(got_cube, axis=0))
    return worst
