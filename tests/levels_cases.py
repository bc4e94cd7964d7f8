"""The cases of the received levels that tests/test_emu_levels.py (CPU emulator, C ABI) and tests/test_levels_gpu.py (hardware,
dw.loc.received_levels) both run.  A runner is
    run(buf, ns, nxt, ns2, r, start, L, gap, N, weights) -> (signal, noise, peak)
where buf is float32 [nch x pitch >= ns] and the block is buf[:, :ns] (pitch > ns: the rows are read in place), nxt is the next
block float32 [nch x pitch2 >= ns2] or None, r int32 [ncalls x nch] the rounded delays, start int64 [ncalls], weights float32
[nch] or None; the results are NumPy float32 arrays [ncalls x nch].  W = the channels per workgroup of d4w_level_limits.

The parity cases give the delay table directly (a base delay plus a small per-channel pattern), so that which windows fall off
the record is decided by the case and not by a geometry."""
import functools

import numpy as np

from tests import known_answers_levels as kl
from tests.beam_cases import padded, weight_set

LENGTHS = (1, 2, 63, 64, 65, 129, 200)
NOISES = (0, 1, 64, 65, 130)
GAPS = (0, 3)
NCH_FORMS = ("1", "W-1", "W", "W+1", "2W+3")
NCALLS = (1, 3)
PITCHES = ("tight", "wide")
WEIGHTS = ("none", "zeros", "one")
STARTS = ("neg", "mid", "seam", "late")                      # "late": every window lies past the end, everything is NaN
DELAYS = ("near", "far")                                     # "far": delays beyond ns, start brought back by their base
NEXTS = ("none", "1", "3", "ns")
AXES = (LENGTHS, NOISES, GAPS, NCH_FORMS, NCALLS, PITCHES, WEIGHTS, STARTS, DELAYS, NEXTS)
NS = 700
FS = 200.0


def parity_cases():
    """36 tuples (L, N, gap, nch form, ncalls, pitch, weights, start, delays, next, index): the largest corner first, then every
    value of every axis several times over (test_every_axis_value_occurs checks that)."""
    cases = [(200, 130, 3, "2W+3", 3, "wide", "zeros", "seam", "far", "ns", 0)]
    for i in range(1, 36):
        cases.append((LENGTHS[i % 7], NOISES[(i + i // 7) % 5], GAPS[(i // 3) % 2], NCH_FORMS[(i + i // 5) % 5], NCALLS[(i // 2) % 2],
                      PITCHES[(i // 5) % 2], WEIGHTS[(i + i // 9) % 3], STARTS[(i + i // 4) % 4], DELAYS[(i // 7) % 2], NEXTS[(i + i // 8) % 4], i))
    return cases


def case_id(c):
    return "L%d-N%d-g%d-nch%s-c%d-%s-w%s-%s-%s-nb%s" % c[:10]


def _nch(form, W):
    return max(1, {"1": 1, "W-1": W - 1, "W": W, "W+1": W + 1, "2W+3": 2 * W + 3}[form])


def make_case(case, W):
    L, N, gap, nchf, ncalls, pitch, wkind, skind, dkind, nkind, i = case
    nch, ns = _nch(nchf, W), NS
    ns2 = {"none": 0, "1": 1, "3": 3, "ns": ns}[nkind]
    rng = np.random.default_rng(11000 + i)
    base = ns + 1234 if dkind == "far" else 40
    r = (base + (7 * np.arange(nch)[None, :] + 3 * np.arange(ncalls)[:, None]) % 11).astype(np.int32)
    # n0 = s + 0 .. 10 over the channels.  "neg": the signal window (even index) or the noise window (odd) begins within 5
    # samples either side of the record's first; "seam": the signal window (even) or the noise window (odd) ends within 5
    # samples either side of the end of the block
    s = {"neg": -5 + (gap + N) * (i % 2), "mid": 300, "seam": (ns + gap - 5) if i % 2 else (ns - L - 5), "late": ns + ns2 + gap + N + 5}[skind]
    start = (s - base + np.array([0, -2, 3])[:ncalls] * (skind != "late")).astype(np.int64)
    w = weight_set(wkind, nch, rng)
    x = rng.standard_normal((nch, ns)).astype(np.float32)
    nb = rng.standard_normal((nch, ns2)).astype(np.float32) if ns2 else None
    return x, nb, r, start, L, gap, N, w, pitch == "wide"


@functools.lru_cache(maxsize=None)
def reference(case, W):
    """The case, its buffers and its float64 answer, computed once for every test that needs them (left unchanged by all)."""
    x, nb, r, start, L, gap, N, w, wide = make_case(case, W)
    ref = kl.levels_ref(x, r, start, L, gap, N, w, nb)
    buf, nbuf = padded(x, wide, w), (padded(nb, wide, w) if nb is not None else None)
    for a in (buf, nbuf, r, start, w, ref.signal, ref.noise, ref.peak, ref.tol_signal, ref.tol_noise, ref.valid_signal, ref.valid_noise):
        if a is not None:
            a.setflags(write=False)
    return buf, x.shape[1], nbuf, (nb.shape[1] if nb is not None else 0), r, start, L, gap, N, w, ref


def mixed(case, W):
    """Whether a live channel of the case has one window valid and the other (N >= 1) not."""
    ref = reference(case, W)[10]
    return bool(ref.N >= 1 and np.any(ref.valid_signal != ref.valid_noise))


def check_outputs(got, shape):
    assert len(got) == 3
    for a in got:
        assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == tuple(shape), (a.dtype, a.shape)


def check_parity(run, case, W):
    """Runs the case; returns the worst error / tolerance of signal and noise."""
    buf, ns, nbuf, ns2, r, start, L, gap, N, w, ref = reference(case, W)
    got = run(buf, ns, nbuf, ns2, r, start, L, gap, N, w)
    check_outputs(got, r.shape)
    worst = kl.worst_ratio(got, ref)                         # NaN exactly where no window fits, no padding and no dead row was read
    print("%s: worst error / tolerance = %.3g, %d signal and %d noise windows of %d valid"
          % (case_id(case), worst, ref.valid_signal.sum(), ref.valid_noise.sum(), r.size))
    assert worst <= 1.0, worst
    dead = np.zeros(r.shape[1], dtype=bool) if w is None else w == 0
    assert all(np.all(np.isnan(a[:, dead])) for a in got)
    if N == 0:
        assert np.all(np.isnan(got[1]))
    if case[7] == "late":
        assert not ref.valid_signal.any() and not ref.valid_noise.any() and all(np.all(np.isnan(a)) for a in got)
    if case[7] == "mid":
        assert ref.valid_signal[:, ~dead].all() and (N == 0 or ref.valid_noise[:, ~dead].all())
        assert not np.isnan(got[0][:, ~dead]).any() and not np.isnan(got[2][:, ~dead]).any()
    return worst


def owned(ref, nch, ntot):
    """bool [nch x ntot]: the samples inside a valid window of some call."""
    own = np.zeros((nch, ntot), dtype=bool)
    for c, ch in zip(*np.nonzero(ref.valid_signal)):
        own[ch, ref.n0[c, ch]:ref.n0[c, ch] + ref.L] = True
    for c, ch in zip(*np.nonzero(ref.valid_noise)):
        own[ch, ref.n0[c, ch] - ref.gap - ref.N:ref.n0[c, ch] - ref.gap] = True
    return own


def check_poison(run, case, W):
    """Every sample outside the union of the valid windows set to NaN: the same bits.  No load touches what it does not own."""
    buf, ns, nbuf, ns2, r, start, L, gap, N, w, ref = reference(case, W)
    clean = run(buf, ns, nbuf, ns2, r, start, L, gap, N, w)
    own = owned(ref, buf.shape[0], ns + ns2)
    pb = buf.copy()
    pb[:, :ns][~own[:, :ns]] = np.nan
    pn = None
    if nbuf is not None:
        pn = nbuf.copy()
        pn[:, :ns2][~own[:, ns:]] = np.nan
    dirty = run(pb, ns, pn, ns2, r, start, L, gap, N, w)
    assert all(kl.same(a, b) for a, b in zip(clean, dirty))
    return int(own.sum())


# ---- exact known answers -----------------------------------------------------------------------------------------------------
def _scene(nch, ncalls, ns=600, seed=5, first=200):
    """r, start and a block: n0 = first + 60 .. 72 (+ 20 per call), so that windows of 200 + 3 + 130 samples fit both ways."""
    rng = np.random.default_rng(seed + nch)
    r = (60 + (5 * np.arange(nch)[None, :] + 2 * np.arange(ncalls)[:, None]) % 13).astype(np.int32)
    start = (first + 20 * np.arange(ncalls)).astype(np.int64)
    return rng, r, start, rng.standard_normal((nch, ns)).astype(np.float32)


def check_integers(run, W):
    """Integer samples in [-15, 15]: every partial sum is an integer below 2^24, so signal = float32(E) / float32(L) exactly,
    noise likewise, and peak exactly."""
    for L, gap, N, ns, first in ((200, 3, 130, 700, 200), (65, 0, 64, 700, 200), (1, 3, 1, 700, 200), (4096, 3, 4095, 8600, 4200)):
        nch = W + 1
        rng, r, start, _ = _scene(nch, 2, ns, first=first)
        x = rng.integers(-15, 16, (nch, ns)).astype(np.float32)
        ref = kl.levels_ref(x, r, start, L, gap, N)
        assert ref.valid_signal.all() and ref.valid_noise.all()
        got = run(x, ns, None, 0, r, start, L, gap, N, None)
        check_outputs(got, r.shape)
        es, eq = np.rint(ref.signal * L), np.rint(ref.noise * N)
        assert es.max() < 2 ** 24 and eq.max() < 2 ** 24
        assert kl.same(got[0], es.astype(np.float32) / np.float32(L))
        assert kl.same(got[1], eq.astype(np.float32) / np.float32(N))
        assert kl.same(got[2], ref.peak.astype(np.float32))


def check_zeros_and_ones(run, W):
    """An all-zero block gives 0, 0, 0 on valid windows; a block of ones gives signal = noise = peak = 1 for every length of
    the axes."""
    nch = W + 1
    _, r, start, x = _scene(nch, 2)
    got = run(np.zeros_like(x), 600, None, 0, r, start, 65, 3, 64, None)
    check_outputs(got, r.shape)
    assert all(not a.any() and not np.isnan(a).any() for a in got)
    for i, L in enumerate(LENGTHS):
        N = NOISES[1 + i % 4]
        got = run(np.ones_like(x), 600, None, 0, r, start, L, i % 2, N, None)
        assert all(np.all(a == 1.0) for a in got), (L, N)
    for N in NOISES[1:]:
        got = run(np.ones_like(x), 600, None, 0, r, start, 64, 0, N, None)
        assert all(np.all(a == 1.0) for a in got), N


def check_nan_rows(run, W):
    """A NaN row under weight 0 changes nothing; a NaN between or just outside the windows changes nothing; a NaN inside a
    window makes that window's values NaN and leaves the other window's bits."""
    nch, L, gap, N = W + 1, 65, 3, 64
    rng, r, start, x = _scene(nch, 1)
    w = weight_set("zeros", nch, rng)
    assert (w == 0).any() and w[nch - 1] != 0
    clean = run(x, 600, None, 0, r, start, L, gap, N, w)
    assert np.isfinite(clean[0][:, w != 0]).all() and np.isfinite(clean[1][:, w != 0]).all()
    dirty = x.copy()
    dirty[w == 0] = np.nan
    assert all(kl.same(a, b) for a, b in zip(clean, run(dirty, 600, None, 0, r, start, L, gap, N, w)))
    ch = nch - 1
    n0 = int(kl.first_samples(start, r)[0, ch])
    keep = np.arange(nch) != ch

    def with_nan(at):
        d = x.copy()
        d[ch, at] = np.nan
        got = run(d, 600, None, 0, r, start, L, gap, N, w)
        assert all(kl.same(a[:, keep], b[:, keep]) for a, b in zip(got, clean))
        return [a[0, ch] for a in got]

    for at in (n0 - 1, n0 - gap, n0 - gap - N - 1, n0 + L):   # between the windows, before the noise window, after the signal window
        assert all(kl.same(a, b[0, ch]) for a, b in zip(with_nan(at), clean)), at
    for at in (n0, n0 + L // 2, n0 + L - 1):
        s, q, p = with_nan(at)
        assert np.isnan(s) and np.isnan(p) and kl.same(q, clean[1][0, ch]), at
    for at in (n0 - gap - 1, n0 - gap - N):
        s, q, p = with_nan(at)
        assert np.isnan(q) and kl.same(s, clean[0][0, ch]) and kl.same(p, clean[2][0, ch]), at


def check_bit_identity(run, W):
    """Bit for bit: a repeated call; x scaled by 2^-3 and 2^5 (signal and noise by 4^k, peak by 2^k, exactly); one call alone
    against the same call as row 1 of three; wide pitch against tight; the data moved right by 1, 2, 3 samples with start
    moved along (no dependence on the alignment of a window)."""
    for L, gap, N in ((63, 0, 65), (200, 3, 130), (2, 3, 1)):
        nch = 2 * W + 3
        rng, r, start, x = _scene(nch, 3)
        w = weight_set("zeros", nch, rng)
        first = run(x, 600, None, 0, r, start, L, gap, N, w)
        assert all(np.isfinite(a[:, w != 0]).all() for a in first)
        again = run(x, 600, None, 0, r, start, L, gap, N, w)
        assert all(kl.same(a, b) for a, b in zip(first, again))
        for p in (-3, 5):
            scaled = run(x * np.float32(2.0 ** p), 600, None, 0, r, start, L, gap, N, w)
            assert kl.same(scaled[0], first[0] * np.float32(4.0 ** p)) and kl.same(scaled[1], first[1] * np.float32(4.0 ** p))
            assert kl.same(scaled[2], first[2] * np.float32(2.0 ** p))
        alone = run(x, 600, None, 0, r[1:2], start[1:2], L, gap, N, w)
        assert all(kl.same(a[0], b[1]) for a, b in zip(alone, first))
        wide = run(padded(x, True, w), 600, None, 0, r, start, L, gap, N, w)
        assert all(kl.same(a, b) for a, b in zip(first, wide))
        for s in (1, 2, 3):
            moved = np.zeros_like(x)
            moved[:, s:] = x[:, :-s]
            got = run(moved, 600, None, 0, r, start + s, L, gap, N, w)
            assert all(kl.same(a, b) for a, b in zip(first, got)), s


def check_split(run, W):
    """trace = x[:, :k] with next_block = x[:, k:] equals the unsplit x bit for bit, for k at and next to every end of the two
    windows of channel 0, whatever the pitches."""
    nch, L, gap, N = W + 1, 129, 3, 65
    _, r, start, x = _scene(nch, 3)
    ns = x.shape[1]
    whole = run(x, ns, None, 0, r, start, L, gap, N, None)
    assert all(np.isfinite(a).all() for a in whole)
    n0 = int(kl.first_samples(start, r)[0, 0])
    for i, k in enumerate((n0 - gap - N, n0 - gap - 1, n0, n0 + 1, n0 + L - 1, n0 + L)):
        a, b = np.ascontiguousarray(x[:, :k]), np.ascontiguousarray(x[:, k:])
        got = run(padded(a, i % 2 == 0), k, padded(b, i % 2 == 1), ns - k, r, start, L, gap, N, None)
        assert all(kl.same(p, q) for p, q in zip(whole, got)), k
