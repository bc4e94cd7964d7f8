"""float64 NumPy restatement of the window-normalised matched filter (csrc/nmf.hip, detect.compute_nmf_correlograms) and the
scene its tests share.  No reference counterpart: the definition is DESIGN.md 3.3a.

For a row x of ns samples, the support h of a template (m taps; a zero-padded full-length template cut to its support as
detect._normalised_support does, no DC tail), h' = h - mean(h), the row's mean mu and A = max|x|:
    x'[i] = (x[i] - mu) / A for i < ns; (head[i - ns] - mu) / A for ns <= i < ns + m - 1 when a continuation is given; 0 beyond
    c[k]  = sum_{n < m} x'[k + n] h'[n]
    S1[k] = sum x'[k + n],  S2[k] = sum x'[k + n]^2,  V[k] = S2 - S1^2 / m (center) or S2
    nmf[k] = c[k] / (|h'| sqrt(V[k])) where V[k] > floor^2 m, 0 elsewhere;  a row with A = 0 is all zeros.
The windowed sums are differences of prefix sums in np.longdouble (64-bit mantissa: the cancellation of a 4500-sample prefix
costs 1e-15, a thousandth of floor^2 at the default floor).

Bound (derived from what the kernel may round, not measured): every normalised sample is carried in float32, an absolute error
of at most 2^-23 in units where |x'| <= 1; sqrt(V) is the 2-norm of the (centred) window, so it moves by at most the 2-norm of
the errors, 2^-23 sqrt(m): a relative e = 2^-23 sqrt(m / V[k]), and 1 / sqrt(V) by e / (1 - e).  Three float32 roundings of the
final scale: 2^-21 |ref|.  Where the restatement gives 0 the kernel must give exactly 0.
Margin rule (as in known_answers_stack): the decision V > floor^2 m is compared only where V / m is a factor 4 away from floor^2
on either side; `nmf` returns that mask, the share of excluded elements must be 0 and a comparing test asserts that first.  On
the scene the closest element lies more than ten octaves away.
"""
import numpy as np

from oracle import d4w_oracle as orc

TILE = 2048              # lags one workgroup of csrc/nmf.hip takes (kNmfTile = d4w_nmf_tile())
RUN = 8                  # ... and one thread (kNmfRun)
FLOOR = 1e-6             # the default floor

FS, NS, NHEAD, SEED = 200.0, 4500, 200, 7
CALLS = {0: ("hf", 1000), 1: ("hf", 2000), 2: ("lf", 3000), 3: ("hf", 3500), 4: ("hf", 700), 7: ("hf", NS - 60)}
SPIKE_AT = 2500          # row 4's sample of 1e4
DROPOUT = (1500, 2200)   # row 3: exact zeros
CONSTANT = (800, 1400)   # row 6: 3.25


def support(template):
    """The template's support (up to its last non-zero sample), as a float64 vector."""
    t = np.asarray(template, dtype=np.float64).ravel()
    nz = np.nonzero(t)[0]
    return t[:int(nz[-1]) + 1 if len(nz) else 1]


def demeaned(template):
    """h' = h - mean(h) over the support, scaled by 1 / max|h| (the scale cancels in the result)."""
    h = support(template)
    return (h - h.mean()) / np.max(np.abs(h))


def templates():
    """The scripts' fin-whale templates at fs = 200 (supports 135 and 155), full length (zero-padded to NS)."""
    t = np.arange(NS) / FS
    return {"hf": orc.gen_template_fincall(t, FS, 17.8, 28.8, 0.68), "lf": orc.gen_template_fincall(t, FS, 14.7, 21.8, 0.78)}


def scene():
    """(x [8 x NS] float32, head [8 x NHEAD] float32): the rows of the issue, each generated NS + NHEAD samples long and cut."""
    rng = np.random.default_rng(SEED)
    n = NS + NHEAD
    x = rng.standard_normal((8, n))
    tp = templates()
    for row, (name, at) in CALLS.items():
        h = support(tp[name])
        x[row, at:at + len(h)] += 4.0 * h
    x[1] *= 300.0
    x[2] += 200.0 + (-50.0 + 100.0 * np.arange(n) / (NS - 1))
    x[3, DROPOUT[0]:DROPOUT[1]] = 0.0
    x[4, SPIKE_AT] = 1e4
    x[5] = 0.0
    x[6, CONSTANT[0]:CONSTANT[1]] = 3.25
    x = x.astype(np.float32)
    return np.ascontiguousarray(x[:, :NS]), np.ascontiguousarray(x[:, NS:])


def normalised_rows(x, m, head=None, mean=None, maxabs=None):
    """x' [nx x (ns + m - 1)] float64; mean / maxabs: the statistics the kernel is given (default: the rows' own)."""
    x = np.asarray(x, dtype=np.float64)
    nx, ns = x.shape
    mu = x.mean(axis=1) if mean is None else np.asarray(mean, dtype=np.float64)
    A = np.abs(x).max(axis=1) if maxabs is None else np.asarray(maxabs, dtype=np.float64)
    g = np.where(A > 0, 1.0 / np.where(A > 0, A, 1.0), 0.0)
    xe = np.zeros((nx, ns + m - 1))
    xe[:, :ns] = (x - mu[:, None]) * g[:, None]
    if head is not None and m > 1:
        hd = np.asarray(head, dtype=np.float64)[:, :m - 1]
        xe[:, ns:ns + hd.shape[1]] = (hd - mu[:, None]) * g[:, None]
    return xe


def window_energy(xe, m, center=True):
    """V [nx x ns] float64 from prefix sums in np.longdouble."""
    xl = xe.astype(np.longdouble)
    z = np.zeros((xe.shape[0], 1), dtype=np.longdouble)
    p1 = np.concatenate((z, np.cumsum(xl, axis=1)), axis=1)
    p2 = np.concatenate((z, np.cumsum(xl * xl, axis=1)), axis=1)
    s1, s2 = p1[:, m:] - p1[:, :-m], p2[:, m:] - p2[:, :-m]
    return (s2 - s1 * s1 / m if center else s2).astype(np.float64)


def correlate(xe, hp):
    """c [nx x ns] float64: sum_n x'[k + n] h'[n]."""
    return np.stack([np.correlate(r, hp, "valid") for r in xe])


def nmf(x, c, m, hnorm, center=True, floor=FLOOR, head=None, mean=None, maxabs=None):
    """(ref, bound, compared) per element for the numerator c [nx x ns] (any array: the kernel alone takes what it is given),
    a support of m taps of 2-norm hnorm.  compared: the margin rule's mask."""
    xe = normalised_rows(x, m, head, mean, maxabs)
    V = window_energy(xe, m, center)
    thr = floor * floor * m
    live = (V > thr) & (hnorm > 0)
    with np.errstate(all="ignore"):
        ref = np.where(live, np.asarray(c, dtype=np.float64) / (hnorm * np.sqrt(np.where(live, V, 1.0))), 0.0)
        e = 2.0 ** -23 * np.sqrt(m / np.where(live, V, 1.0))
    bound = np.where(live, np.abs(ref) * (e / np.maximum(1.0 - e, 2.0 ** -10) + 2.0 ** -21), 0.0)
    compared = (V > 4.0 * thr) | (V < thr / 4.0) | ~(hnorm > 0)
    return ref, bound, compared


def nmf_of_template(x, template, center=True, floor=FLOOR, head=None):
    """The public call's answer: (ref, bound, compared, slack) with slack = max_k |c_ref(row)| / (|h'| sqrt(V[k])) -- what a
    correlator tolerance TOL (relative to the row's largest correlation) becomes after the division."""
    hp = demeaned(template)
    m, hn = len(hp), float(np.sqrt(np.sum(hp * hp)))
    xe = normalised_rows(x, m, head)
    c = correlate(xe, hp)
    ref, bound, compared = nmf(x, c, m, hn, center, floor, head)
    V = window_energy(xe, m, center)
    live = (V > floor * floor * m) & (hn > 0)
    with np.errstate(all="ignore"):
        slack = np.where(live, np.abs(c).max(axis=1, keepdims=True) / (hn * np.sqrt(np.where(live, V, 1.0))), 0.0)
    return ref, bound, compared, slack
