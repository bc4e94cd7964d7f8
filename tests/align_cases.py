"""The cases of the alignment against the beam that tests/test_emu_align.py (CPU emulator, C ABI) and tests/test_align_gpu.py
(hardware, dw.loc.refine_arrivals) both run.  A runner is
    run(buf, ns, nxt, ns2, template, r, start, M, weights, fs, min_coef, subsample) -> (Ti, coef, lag, rho)
where buf is float32 [nch x pitch >= ns] and the block is buf[:, :ns] (pitch > ns: the rows are read in place), nxt is the next
block float32 [nch x pitch2 >= ns2] or None, template float32 [ncalls x L], r int32 [ncalls x nch] the rounded delays, start
int64 [ncalls], weights float32 [nch] or None; the results are NumPy arrays Ti float64 and coef float32 [ncalls x nch], lag
int32 [ncalls x nch] and rho float32 [ncalls x nch x (2M + 1)].  W = the channels per workgroup of d4w_align_limits.

The parity cases give the delay table directly (a base delay plus a small per-channel pattern), so that which lags fall off
the record is decided by the case and not by a geometry."""
import functools

import numpy as np

from tests import known_answers_align as ka
from tests.beam_cases import padded, weight_set

LENGTHS = (1, 2, 63, 64, 65, 200)
LAGS = (0, 1, 31, 32, 33)                                    # 2M + 1 = 63, 65, 67 around one block of 64 lanes
NCH_FORMS = ("1", "W-1", "W", "W+1", "2W+3")
NCALLS = (1, 3)
PITCHES = ("tight", "wide")
WEIGHTS = ("none", "zeros", "one")
STARTS = ("neg", "mid", "seam", "late")                      # "late": every window lies past the end, everything is NaN
DELAYS = ("near", "far")                                     # "far": delays beyond ns, start brought back by their base
NEXTS = ("none", "1", "3", "ns")
AXES = (LENGTHS, LAGS, NCH_FORMS, NCALLS, PITCHES, WEIGHTS, STARTS, DELAYS, NEXTS)
NS = 700
FS = 200.0


def parity_cases():
    """36 tuples (L, M, nch form, ncalls, pitch, weights, start, delays, next, index): the largest corner first, then every
    value of every axis several times over (test_every_axis_value_occurs checks that)."""
    cases = [(200, 33, "2W+3", 3, "wide", "zeros", "seam", "far", "ns", 0)]
    for i in range(1, 36):
        cases.append((LENGTHS[i % 6], LAGS[(i + i // 6) % 5], NCH_FORMS[(i + i // 5) % 5], NCALLS[(i // 2) % 2], PITCHES[(i // 5) % 2],
                      WEIGHTS[(i + i // 9) % 3], STARTS[(i + i // 4) % 4], DELAYS[(i // 7) % 2], NEXTS[(i + i // 8) % 4], i))
    return cases


def case_id(c):
    return "L%d-M%d-nch%s-c%d-%s-w%s-%s-%s-nb%s" % c[:9]


def _nch(form, W):
    return max(1, {"1": 1, "W-1": W - 1, "W": W, "W+1": W + 1, "2W+3": 2 * W + 3}[form])


def make_case(case, W):
    L, M, nchf, ncalls, pitch, wkind, skind, dkind, nkind, i = case
    nch, ns = _nch(nchf, W), NS
    ns2 = {"none": 0, "1": 1, "3": 3, "ns": ns}[nkind]
    rng = np.random.default_rng(9000 + i)
    base = ns + 1234 if dkind == "far" else 40
    r = (base + (7 * np.arange(nch)[None, :] + 3 * np.arange(ncalls)[:, None]) % 11).astype(np.int32)
    # n0 = s + 0 .. 10 over the channels.  "neg": the leading lags fall before the record (all of them where M is 0);
    # "seam": the windows end within 5 samples either side of the end of the block
    s = {"neg": -5 - M // 2, "mid": 150, "seam": ns - L - M - 5, "late": ns + ns2 + M + 5}[skind]
    start = (s - base + np.array([0, -2, 3])[:ncalls] * (skind != "late")).astype(np.int64)
    w = weight_set(wkind, nch, rng)
    x = rng.standard_normal((nch, ns)).astype(np.float32)
    nb = rng.standard_normal((nch, ns2)).astype(np.float32) if ns2 else None
    t = rng.standard_normal((ncalls, L)).astype(np.float32)
    return x, nb, t, r, start, M, w, pitch == "wide"


@functools.lru_cache(maxsize=None)
def reference(case, W):
    """The case, its buffers and its float64 answer, computed once for every test that needs them (left unchanged by all)."""
    x, nb, t, r, start, M, w, wide = make_case(case, W)
    ref = ka.align_ref(x, t, r, start, M, w, nb)
    buf, nbuf = padded(x, wide, w), (padded(nb, wide, w) if nb is not None else None)
    for a in (buf, nbuf, t, r, start, w, ref.rho, ref.A, ref.en, ref.tn):
        if a is not None:
            a.setflags(write=False)
    return buf, x.shape[1], nbuf, (nb.shape[1] if nb is not None else 0), t, r, start, M, w, ref


def check_picks(got, n0, M, fs, min_coef=0.0, subsample=True):
    """The pick re-derived from the returned table: exactly the returned lag, coefficient and arrival time."""
    Ti, coef, lag, rho = got
    assert Ti.dtype == np.float64 and coef.dtype == np.float32 and lag.dtype == np.int32 and rho.dtype == np.float32
    want_lag, want_coef, _, want_Ti = ka.pick_table(rho, n0, M, fs, min_coef, subsample)
    assert ka.same(lag, want_lag) and ka.same(coef, want_coef) and ka.same(Ti, want_Ti)


def check_parity(run, case, W):
    """Runs the case; returns the worst error / tolerance of the table."""
    buf, ns, nbuf, ns2, t, r, start, M, w, ref = reference(case, W)
    got = run(buf, ns, nbuf, ns2, t, r, start, M, w, FS, 0.0, True)
    Ti, coef, lag, rho = got
    assert Ti.shape == r.shape and coef.shape == r.shape and lag.shape == r.shape
    worst = ka.worst_ratio(rho, ref)                         # NaN exactly where no lag fits, no padding and no dead row was read
    print("%s: worst error / tolerance = %.3g, %d of %d entries valid" % (case_id(case), worst, ref.valid.sum(), ref.valid.size))
    assert worst <= 1.0, worst
    check_picks(got, ref.n0, M, FS)
    dead = np.zeros(r.shape[1], dtype=bool) if w is None else w == 0
    assert np.all(np.isnan(Ti[:, dead])) and np.all(np.isnan(coef[:, dead])) and not lag[:, dead].any() and np.all(np.isnan(rho[:, dead]))
    if case[6] == "late":
        assert not ref.valid.any() and np.all(np.isnan(Ti)) and np.all(np.isnan(coef)) and not lag.any()
    if case[6] == "neg" and M >= 31 and not dead.all():
        assert not ref.valid[:, ~dead, 0].any() and ref.valid[:, ~dead, -1].all()     # leading lags are invalid, trailing ones live
    if case[6] == "mid":
        assert ref.valid[:, ~dead].all() and not np.isnan(coef[:, ~dead]).any()
    return worst


# ---- exact known answers -----------------------------------------------------------------------------------------------------
def _scene(nch, ncalls, L, ns=600, seed=5):
    rng = np.random.default_rng(seed + nch + L)
    r = (60 + (5 * np.arange(nch)[None, :] + 2 * np.arange(ncalls)[:, None]) % 13).astype(np.int32)
    start = (100 + 20 * np.arange(ncalls)).astype(np.int64)
    return rng, r, start, rng.standard_normal((nch, ns)).astype(np.float32), rng.standard_normal((ncalls, L)).astype(np.float32)


def check_planted(run, W):
    """A row that is the template planted at lag m0 (zeros around it): m* = m0, |coef - 1| within the tolerance; with the
    maximum at either end of the lag range there is no parabola and Ti = (n0 + m0) / fs exactly."""
    for L, M in ((65, 3), (200, 40)):
        nch = W + 1
        _, r, start, _, t = _scene(nch, 2, L)
        n0 = ka.first_samples(start, r)
        for m0 in (-M, -1, 0, M):
            x = np.zeros((nch, 600), dtype=np.float32)
            for ch in range(nch):
                q = n0[ch % 2, ch] + m0                      # channel ch carries call ch % 2
                x[ch, q:q + L] = t[ch % 2]
            got = run(x, 600, None, 0, t, r, start, M, None, FS, 0.5, True)
            Ti, coef, lag, rho = got
            for ch in range(nch):
                c = ch % 2
                assert lag[c, ch] == m0 and abs(float(coef[c, ch]) - 1.0) <= 2 * (L + 8) * ka.U, (L, M, m0, ch, lag[c, ch], coef[c, ch])
                if abs(m0) == M:
                    assert Ti[c, ch] == float(n0[c, ch] + m0) / FS
                else:
                    assert abs(Ti[c, ch] * FS - float(n0[c, ch] + m0)) <= 0.5
            check_picks(got, n0, M, FS, 0.5)
            assert np.isnan(Ti).any()                        # the other call's channels correlate below min_coef = 0.5


def check_bit_identity(run, W):
    """Bit for bit: a repeated call; one call alone against the same call as row 1 of three; x scaled by 2^-3 and 2^5 and the
    template by 2^4 leave rho (and with it every result) unchanged."""
    for L, M in ((63, 33), (200, 4)):
        nch = 2 * W + 3
        rng, r, start, x, t = _scene(nch, 3, L)
        w = weight_set("zeros", nch, rng)
        first = run(x, 600, None, 0, t, r, start, M, w, FS, 0.0, True)
        assert np.isfinite(first[3][:, w != 0]).all()
        again = run(x, 600, None, 0, t, r, start, M, w, FS, 0.0, True)
        assert all(ka.same(a, b) for a, b in zip(first, again))
        alone = run(x, 600, None, 0, t[1:2], r[1:2], start[1:2], M, w, FS, 0.0, True)
        assert all(ka.same(a[0], b[1]) for a, b in zip(alone, first))
        for p in (-3, 5):
            scaled = run(x * np.float32(2.0 ** p), 600, None, 0, t, r, start, M, w, FS, 0.0, True)
            assert all(ka.same(a, b) for a, b in zip(first, scaled))
        scaled = run(x, 600, None, 0, t * np.float32(16.0), r, start, M, w, FS, 0.0, True)
        assert all(ka.same(a, b) for a, b in zip(first, scaled))


def check_next_block(run, W):
    """refine_arrivals(trace, next_block=b) equals refine_arrivals(concatenate([trace, b])) bit for bit, whatever the pitches."""
    nch, L, M, ns = W + 1, 64, 5, 600
    rng, r, _, x, t = _scene(nch, 2, L)
    start = np.array([100, ns - 60 - L // 2 - 6], dtype=np.int64)            # call 1: the windows straddle the seam
    w = weight_set("zeros", nch, rng)
    for ns2 in (1, 3, ns):
        nb = rng.standard_normal((nch, ns2)).astype(np.float32)
        a = run(padded(x, True), ns, padded(nb, True), ns2, t, r, start, M, w, FS, 0.0, True)
        b = run(np.concatenate([x, nb], axis=1), ns + ns2, None, 0, t, r, start, M, w, FS, 0.0, True)
        assert all(ka.same(p, q) for p, q in zip(a, b))
        alone = run(x, ns, None, 0, t, r, start, M, w, FS, 0.0, True)
        assert ka.same(a[3][0], alone[3][0])
        if ns2 == ns:
            assert np.isfinite(a[3][1][w != 0]).all() and np.isnan(alone[3][1][w != 0]).any()      # the seam needs the next block


def check_nan_sample(run, W):
    """A NaN sample under a non-zero weight: exactly the lags whose window holds it are NaN, they never win, and every other
    entry keeps its bits."""
    nch, L, M = W + 1, 65, 33
    _, r, start, x, t = _scene(nch, 1, L)
    n0 = ka.first_samples(start, r)
    clean = run(x, 600, None, 0, t, r, start, M, None, FS, 0.0, True)
    ch, at = 1, int(n0[0, 1]) + 10                           # inside the windows of the lags m <= 10
    dirty = x.copy()
    dirty[ch, at] = np.nan
    got = run(dirty, 600, None, 0, t, r, start, M, None, FS, 0.0, True)
    m = np.arange(-M, M + 1)
    hit = (int(n0[0, ch]) + m <= at) & (at < int(n0[0, ch]) + m + L)
    assert hit.any() and not hit.all()
    assert np.array_equal(np.isnan(got[3][0, ch]), hit) and ka.same(got[3][0, ch][~hit], clean[3][0, ch][~hit])
    assert not hit[got[2][0, ch] + M] and np.isfinite(got[0][0, ch])
    keep = np.arange(nch) != ch
    assert all(ka.same(a[:, keep], b[:, keep]) for a, b in zip(got, clean))
    check_picks(got, n0, M, FS)


def check_zeros(run, W):
    """A zero block or a zero template: rho = 0 on every valid lag, the first valid lag wins with coefficient 0 and no parabola."""
    nch, L, M = W + 1, 64, 32
    _, r, _, x, t = _scene(nch, 2, L)
    start = np.array([100, -60 - 7], dtype=np.int64)         # call 1: n0 = -7 .. 5, the leading lags are invalid
    n0 = ka.first_samples(start, r)
    for xx, tt in ((np.zeros_like(x), t), (x, np.zeros_like(t)), (np.zeros_like(x), np.zeros_like(t))):
        got = run(xx, 600, None, 0, tt, r, start, M, None, FS, 0.0, True)
        Ti, coef, lag, rho = got
        valid = ~np.isnan(rho)
        assert not rho[valid].any() and not coef.any() and valid[0].all() and not valid[1, :, 0].all()
        first = np.array([[max(-M, -int(n0[c, ch])) for ch in range(nch)] for c in range(2)])
        assert np.array_equal(lag, first) and np.all(lag[0] == -M)
        assert np.array_equal(Ti, (n0.astype(np.float64) + first) / FS)
        check_picks(got, n0, M, FS)


def check_min_coef_and_subsample(run, W):
    """min_coef above and below a coefficient: Ti is NaN exactly where coef < min_coef, nothing else changes; subsample off:
    Ti = (n0 + m*) / fs exactly."""
    nch, L, M = 2 * W + 3, 200, 4
    _, r, start, x, t = _scene(nch, 2, L)
    n0 = ka.first_samples(start, r)
    base = run(x, 600, None, 0, t, r, start, M, None, FS, 0.0, True)
    assert np.isfinite(base[1]).all()
    mid = float(np.sort(base[1].ravel())[base[1].size // 2])
    for thr in (mid, float(np.nextafter(np.float32(mid), np.float32(2.0))), -1.0, 1.5):
        got = run(x, 600, None, 0, t, r, start, M, None, FS, thr, True)
        below = base[1].astype(np.float64) < thr
        assert np.array_equal(np.isnan(got[0]), below) and ka.same(got[0][~below], base[0][~below])
        assert all(ka.same(a, b) for a, b in zip(got[1:], base[1:]))
        check_picks(got, n0, M, FS, thr)
    assert below.all()
    off = run(x, 600, None, 0, t, r, start, M, None, FS, 0.0, False)
    assert all(ka.same(a, b) for a, b in zip(off[1:], base[1:]))
    assert np.array_equal(off[0], (n0.astype(np.float64) + off[2]) / FS)
    inner = np.abs(base[2]) < M
    assert inner.any() and np.any(off[0][inner] != base[0][inner]) and np.all(np.abs(off[0] - base[0]) * FS <= 0.5)
    check_picks(off, n0, M, FS, 0.0, False)
