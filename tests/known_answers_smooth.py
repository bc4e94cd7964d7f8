"""OpenCV's DOCUMENTED definitions of cv2.GaussianBlur and cv2.bilateralFilter as plain float64 loops, and known answers
that the kernels (csrc/edges.hip) and any vectorised restatement must reproduce.  cv2 is not installed anywhere this
project runs, so nothing here was compared with a real OpenCV ("documented definition, unpinned").

    getGaussianKernel(n, sigma): sigma > 0: exp(-(i - (n - 1) / 2)^2 / (2 sigma^2)) normalised to sum 1; sigma <= 0:
        sigma = 0.3 ((n - 1) 0.5 - 1) + 0.8, except the fixed tables of n = 1, 3, 5, 7.
    GaussianBlur(img, (n, n), sigma): correlation with the taps along rows and along columns, BORDER_REFLECT_101.
    bilateralFilter(img, d, sigma_color, sigma_space): sigma <= 0 -> 1; r = max(round(1.5 sigma_space), 1) for d <= 0, else
        d // 2; out(p) = sum_q w I(q) / sum_q w over offsets (i, j) with i^2 + j^2 <= r^2,
        w = exp(-(i^2 + j^2) / (2 sigma_space^2) - (I(q) - I(p))^2 / (2 sigma_color^2)), BORDER_REFLECT_101.
"""
import math

import numpy as np

from tests.known_answers import filter2d_loops, reflect101

FIXED_TAPS = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [1 / 16, 4 / 16, 6 / 16, 4 / 16, 1 / 16],
              7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}


def gaussian_kernel_loops(n, sigma):
    if sigma <= 0 and n in FIXED_TAPS:
        return list(FIXED_TAPS[n])
    s = sigma if sigma > 0 else 0.3 * ((n - 1) * 0.5 - 1) + 0.8
    t = [math.exp(-((i - (n - 1) / 2) ** 2) / (2 * s * s)) for i in range(n)]
    tot = math.fsum(t)
    return [v / tot for v in t]


def gaussian_blur_loops(img, size, sigma):
    """cv2.GaussianBlur(img, (size, size), sigma) by definition (small images only)."""
    img = np.asarray(img, dtype=np.float64)
    h, w = img.shape
    taps = gaussian_kernel_loops(size, sigma)
    a = size // 2
    rows = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            rows[y, x] = math.fsum(taps[t] * img[y, reflect101(x + t - a, w)] for t in range(size))
    out = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            out[y, x] = math.fsum(taps[t] * rows[reflect101(y + t - a, h), x] for t in range(size))
    return out


def bilateral_radius_loops(diameter, sigma_space):
    ss = sigma_space if sigma_space > 0 else 1.0
    return max(int(round(1.5 * ss)), 1) if diameter <= 0 else diameter // 2


def bilateral_loops(img, diameter, sigma_color, sigma_space):
    """cv2.bilateralFilter(img, diameter, sigma_color, sigma_space) by definition (small images only)."""
    img = np.asarray(img, dtype=np.float64)
    h, w = img.shape
    sc = sigma_color if sigma_color > 0 else 1.0
    ss = sigma_space if sigma_space > 0 else 1.0
    r = bilateral_radius_loops(diameter, ss)
    out = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            num, den = [], []
            for i in range(-r, r + 1):
                for j in range(-r, r + 1):
                    if i * i + j * j > r * r:
                        continue
                    q = img[reflect101(y + i, h), reflect101(x + j, w)]
                    wt = math.exp(-(i * i + j * j) / (2 * ss * ss) - (q - img[y, x]) ** 2 / (2 * sc * sc))
                    num.append(wt * q)
                    den.append(wt)
            out[y, x] = math.fsum(num) / math.fsum(den)
    return out


def round_u8(v):
    """float -> uint8 as cv2's saturate_cast: round half to even, saturate."""
    return np.clip(np.rint(np.asarray(v, dtype=np.float64)), 0, 255).astype(np.uint8)


def check_uint8_rule(got_u8, ref_f64, what=""):
    """The uint8 rule: equal to the rounded float64 value wherever that value lies farther than 1e-3 from a half-integer,
    within one level on the rest, and at most 1 % of the pixels left out this way.  Returns the share left out."""
    ref_f64 = np.asarray(ref_f64, dtype=np.float64)
    assert got_u8.dtype == np.uint8 and got_u8.shape == ref_f64.shape, (what, got_u8.dtype, got_u8.shape)
    frac = ref_f64 - np.floor(ref_f64)
    near_tie = np.abs(frac - 0.5) <= 1e-3
    want = round_u8(ref_f64)
    assert np.array_equal(got_u8[~near_tie], want[~near_tie]), (what, int(np.sum(got_u8[~near_tie] != want[~near_tie])))
    assert np.all(np.abs(got_u8[near_tie].astype(np.int64) - want[near_tie].astype(np.int64)) <= 1), what
    share = float(np.mean(near_tie))
    assert share <= 0.01, (what, share)
    return share


def _rel(y, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(y, dtype=np.float64) - ref)) / max(float(np.max(np.abs(ref))), 1e-300))


def check_gaussian(gaussian_filter, tol, sizes=(1, 3, 5, 7, 9, 21, 31, 33)):
    """Known answers of gaussian_filter(img, size, sigma) -> array."""
    rng = np.random.default_rng(77)
    # a constant image stays constant, whatever the size (also with the image smaller than the kernel) and sigma
    for shape in [(3, 4), (1, 7), (5, 1), (40, 70)]:
        for n in sizes:
            for sigma in (0, 1.7):
                y = gaussian_filter(np.full(shape, 37.25), n, sigma)
                assert y.shape == shape and _rel(y, np.full(shape, 37.25)) <= tol, (shape, n, sigma)
    # size 1 is the identity
    x = np.round(rng.random((19, 70)) * 4096) / 16
    assert _rel(gaussian_filter(x, 1, 0), x) <= tol and _rel(gaussian_filter(x, 1, 2.5), x) <= tol
    # an impulse far from the borders comes back as the outer product of the taps
    for n, sigma in [(3, 0), (5, 0), (7, 0), (9, 2.0), (31, 4.5), (31, 0), (33, 5.0)]:
        img = np.zeros((n + 6, n + 9))
        cy, cx = n // 2 + 2, n // 2 + 5
        img[cy, cx] = 3.0
        t = np.array(gaussian_kernel_loops(n, sigma))
        ref = np.zeros_like(img)
        ref[cy - n // 2:cy + n // 2 + 1, cx - n // 2:cx + n // 2 + 1] = 3.0 * np.outer(t, t)
        assert _rel(gaussian_filter(img, n, sigma), ref) <= tol, (n, sigma)
    # scipy's correlate1d with mode='mirror' (= reflect-101) and the same taps, images smaller than the kernel included
    from scipy.ndimage import correlate1d
    for shape, n, sigma in [((45, 70), 9, 2.0), ((33, 130), 31, 4.5), ((3, 4), 31, 6.0), ((7, 5), 21, 0), ((1, 9), 5, 0),
                            ((9, 1), 7, 1.1), ((20, 66), 33, 5.5), ((2, 2), 5, 0.8)]:
        img = rng.standard_normal(shape) * 20 + 100
        t = np.array(gaussian_kernel_loops(n, sigma))
        ref = correlate1d(correlate1d(img, t, axis=1, mode="mirror"), t, axis=0, mode="mirror")
        assert _rel(gaussian_filter(img, n, sigma), ref) <= tol, (shape, n, sigma)
    # hand-worked corner, taps (1/4, 1/2, 1/4): rows (1, 0, 1) and columns (1, 0, 1) around pixel (0, 0) weigh the 2 x 2
    # corner block equally: (1 + 2 + 3 + 4) / 4
    y = gaussian_filter(np.array([[1.0, 2.0, 9.0], [3.0, 4.0, 9.0], [9.0, 9.0, 9.0]]), 3, 0)
    assert abs(float(y[0, 0]) - 2.5) <= tol * 9.0


def check_bilateral(bilateral_filter, tol, diameters=(3, 5, 9, 31, 33)):
    """Known answers of bilateral_filter(img, diameter, sigma_color, sigma_space) -> array."""
    rng = np.random.default_rng(78)
    # a constant image stays constant (also with the image smaller than the footprint)
    for shape in [(3, 4), (1, 7), (5, 1), (20, 70)]:
        for d in diameters:
            y = bilateral_filter(np.full(shape, 37.25), d, 10.0, 3.0)
            assert y.shape == shape and _rel(y, np.full(shape, 37.25)) <= tol, (shape, d)
    # sigma_color -> 1e9: the range weight is 1 and the filter is the normalised circular spatial kernel
    for shape, d, ss in [((21, 70), 5, 1.5), ((12, 67), 9, 3.0), ((3, 4), 7, 2.0), ((18, 66), 31, 6.0), ((18, 35), 33, 7.0)]:
        img = rng.standard_normal(shape) * 20 + 100
        r = d // 2
        i = np.arange(-r, r + 1)
        rr = i[:, None] ** 2 + i[None, :] ** 2
        k = np.where(rr <= r * r, np.exp(-rr / (2 * ss * ss)), 0.0)
        ref = filter2d_loops(img, k / k.sum())
        assert _rel(bilateral_filter(img, d, 1e9, ss), ref) <= tol, (shape, d, ss)
    # a two-level step with sigma_color far below the step: the weights across the step underflow to 0 and both plateaus
    # come back (exactly up to the rounding of sum w I / sum w itself)
    step = np.full((17, 70), 10.0)
    step[:, 33:] = 200.0
    for d in diameters[:3]:
        assert _rel(bilateral_filter(step, d, 1.0, 3.0), step) <= min(tol, 1e-6), d
    # diameter <= 0: the radius comes from sigma_space; sigma <= 0 counts as 1
    img = np.round(rng.random((16, 40)) * 255)
    assert _rel(bilateral_filter(img, 0, 25.0, 1.4), bilateral_loops(img, 5, 25.0, 1.4)) <= tol
    assert _rel(bilateral_filter(img, -1, 0, -3.0), bilateral_loops(img, 5, 1.0, 1.0)) <= tol
    # hand-worked 3 x 3 corner, d = 3 (centre + 4 neighbours), sigma_color = sigma_space = 1: around pixel (0, 0) reflect-101
    # gives I(1, 0) twice (above, below) and I(0, 1) twice (left, right)
    y = bilateral_filter(np.array([[1.0, 2.0, 7.0], [3.0, 5.0, 7.0], [7.0, 7.0, 7.0]]), 3, 1.0, 1.0)
    w1, w2 = math.exp(-0.5 - 0.5), math.exp(-0.5 - 2.0)
    assert abs(float(y[0, 0]) - (1.0 + 2 * w1 * 2.0 + 2 * w2 * 3.0) / (1.0 + 2 * w1 + 2 * w2)) <= tol * 7.0
