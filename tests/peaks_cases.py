"""Inputs, reference and path predictors shared by the peak-picker tests: tests/test_emu_peaks.py (CPU emulator, C ABI on host
pointers) and tests/test_peaks_gpu.py (hardware, C ABI on device pointers and the package).

Reference: scipy.signal.find_peaks(row.astype(float64), prominence=float64 bar)[0], row by row.  Every comparison is exact
equality of the index arrays and of the counts: there is no tolerance anywhere.  Two kinds of row are excluded from the exact
comparison (and only they): a row with isolated NaN samples (SciPy's answer depends on its comparison order: the count lies
in [0, ns // 2] and the indices rise strictly within [1, ns - 2]), and a +inf sample under a +inf bar (SciPy keeps that peak,
the kernel returns none: DESIGN.md, the picker's parity notes; every other index of such a row is still compared).

The predictors restate the decisions of das4whales_amd/csrc/peaks.hip in plain Python: those the host takes in
find_peaks_launch (block size, staged or in place, 16-byte or scalar loads, the window sweep) and, from the samples, the
counts the kernel's own decisions rest on (candidates, hot blocks, per window the busy groups, turning points and maxima).
Each case names the branches it is meant to reach; tests/test_emu_peaks.py asserts that it reaches them and that the whole
table reaches every branch of BRANCHES."""
import collections

import numpy as np
import scipy.signal as sps

# the constants of peaks.hip, restated
MAX_BLOCKS, ROW_LDS, FAN, LIST, WAVE_SIDES = 4096, 16384, 32, 4096, 256
SEG_H, SEG_W, SEG_E, SEG_C, SEG_FEW = 64, 2048, 1024, 512, 24
SEG_S = SEG_W - 2 * SEG_H
LDS_MAX = 150 * 1024
SENTINEL = -77

BRANCHES = frozenset((
    # host forms
    "staged_vec4", "staged_scalar", "inplace_sweep", "inplace_scalar", "bshift6", "bshift7",
    # per row
    "nan_bar", "early_exit", "by_block", "by_block_fallback", "mark4", "mark_scalar", "walk_wave", "walk_lane", "one_list",
    "word_rounds", "window_few", "window_full", "window_listed", "window_not_listed", "resume", "cold_window"))


# ------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------
def reference(row, bar):
    return sps.find_peaks(np.asarray(row, dtype=np.float64), prominence=float(bar))[0]


def check_row(got_idx, got_cnt, row, bar, cap, where=""):
    """One row of a launch against the reference: idx [cap] (filled with SENTINEL before the call), its count."""
    ns = len(row)
    n = int(got_cnt)
    assert n != SENTINEL, ("count not written", where)
    kept = got_idx[:min(n, cap)]
    assert np.all(got_idx[min(max(n, 0), cap):] == SENTINEL), ("written past the count", where)
    finite_nan = np.isnan(row).any() and not np.isnan(row).all()
    if finite_nan:
        assert 0 <= n <= ns // 2, (n, where)
        assert np.all(np.diff(kept) > 0) and (len(kept) == 0 or (kept[0] >= 1 and kept[-1] <= ns - 2)), where
        return
    ref = reference(row, bar)
    if bar == np.inf:
        ref = ref[row[ref] != np.inf]                       # the documented deviation: no pick under a +inf bar
    assert n == len(ref), (n, len(ref), where)
    assert np.array_equal(kept, ref[:cap]), where


# ------------------------------------------------------------------------------------------
# host decisions (find_peaks_launch, find_peaks_prom)
# ------------------------------------------------------------------------------------------
def bshift_of(ns):
    b = 5
    while ((ns + (1 << b) - 1) >> b) > MAX_BLOCKS:
        b += 1
    return b


def lds_bytes(ns, staged=None):
    b = bshift_of(ns)
    nb = (ns + (1 << b) - 1) >> b
    nb2 = (nb + FAN - 1) // FAN
    staged = ns <= ROW_LDS if staged is None else staged
    return 4 * (2 * ((nb + nb2 + 1) & ~1) + 2 * ((((ns + 31) >> 5) + 3) & ~3) + LIST + (ns if staged else 0))


def longest_row():
    """The longest row whose LDS tables fit (the next length is refused)."""
    ns = 1 << 18
    while lds_bytes(ns + 1) <= LDS_MAX:
        ns += 1
    assert all(lds_bytes(n) > LDS_MAX for n in range(ns + 1, ns + 4096)) and lds_bytes(1 << 19) > LDS_MAX
    return ns


Plan = collections.namedtuple("Plan", "bshift nb staged vec4 sweep mark4")


def plan(ns, offset=0, staged=None):
    """offset: floats between a 16-byte boundary and the block's first sample; staged: the D4W_FP_STAGED switch (None: unset)."""
    b = bshift_of(ns)
    st = ns <= ROW_LDS if staged is None else (staged and ns <= ROW_LDS)
    al16 = ns % 4 == 0 and offset % 4 == 0
    vec4 = b == 5 and al16
    return Plan(b, (ns + (1 << b) - 1) >> b, st, vec4, not st and vec4, (ns % 4 == 0) if st else al16)


def _walk_forms(totals):
    out = set()
    for t in totals:
        if t:
            out.add("walk_wave" if 2 * t <= WAVE_SIDES else "walk_lane")
    return out


def row_branches(row, thr, pl):
    """The branches one row takes with the bar thr under the plan pl."""
    host = ("bshift%d" % pl.bshift) if pl.bshift > 5 else \
        ("staged_" if pl.staged else "inplace_") + ("vec4" if pl.vec4 and pl.staged else "sweep" if pl.sweep else "scalar")
    out = {host}
    if thr != thr:
        return out | {"nan_bar"}
    if np.isnan(row).any():
        return out
    ns = len(row)
    r = row.astype(np.float64)
    with np.errstate(invalid="ignore"):
        gmax, gmin = r.max(), r.min()
        if gmax - gmin < thr:
            return out | {"early_exit"}
        if ns < 3:
            return out
        reach = ~(r - thr < gmin)
        cand = np.zeros(ns, dtype=bool)
        cand[1:-1] = (r[:-2] < r[1:-1]) & ~(r[2:] > r[1:-1]) & reach[1:-1]
    nwords = (ns + 31) >> 5
    percand = np.add.reduceat(cand, np.arange(0, ns, 32))
    known = True
    if not pl.sweep:
        total, extra = int(cand.sum()), 0
        if pl.mark4 and pl.bshift == 5:
            pad = np.full(nwords * 32, -np.inf)
            pad[:ns] = r
            with np.errstate(invalid="ignore"):
                nhot = int((~(pad.reshape(-1, 32).max(axis=1) - thr < gmin)).sum())
            if 4 * nhot > pl.nb:
                out |= {"by_block_fallback", "mark4"}
            else:
                out.add("by_block")
                extra = nhot
        else:
            out.add("mark4" if pl.mark4 else "mark_scalar")
    else:
        out |= _windows(r, cand, thr, gmin, ns)
        known = "window_listed" not in out                   # a listed window settles its maxima itself: what is left is not predicted
        total, extra = int(cand.sum()), 0
        if "resume" in out:
            out.add("mark4")
    if known:
        if total + extra <= LIST:
            out.add("one_list")
            out |= _walk_forms([total])
        else:
            out.add("word_rounds")
            out |= _walk_forms(int(percand[w:w + LIST // 16].sum()) for w in range(0, nwords, LIST // 16))
    return out


def _windows(r, cand, thr, gmin, ns):
    """fp_sweep_segments: the decisions of every window of 1920 + 2 x 64 samples."""
    out = set()
    nseg = (ns + SEG_S - 1) // SEG_S
    nblk = (ns + 31) >> 5
    pad = np.full(nblk * 32, -np.inf)
    pad[:ns] = r
    with np.errstate(invalid="ignore"):
        blkhot = ~(pad.reshape(-1, 32).max(axis=1) - thr < gmin)
    few = full = 0
    for s in range(nseg):
        if not blkhot[s * (SEG_S // 32):(s + 1) * (SEG_S // 32)].any():
            out.add("cold_window")
            continue
        lo, hi = s * SEG_S, min((s + 1) * SEG_S, ns)
        core = cand[lo:hi]
        groups = np.add.reduceat(core, np.arange(0, hi - lo, 4)) > 0         # lo is a multiple of 4
        if int(groups.sum()) <= SEG_FEW:
            out.add("window_few")
            few += 1
            if few == 2 and not full:
                if (s + 1) * SEG_S < ns:
                    out.add("resume")
                break
            continue
        full += 1
        out.add("window_full")
        w0 = lo - SEG_H
        win = np.full(SEG_W + 2, np.inf)
        a, b = max(w0, 0), min(w0 + SEG_W, ns)
        win[1 + a - w0:1 + b - w0] = r[a:b]
        v, left, right = win[1:-1], win[:-2], win[2:]
        pos = w0 + np.arange(SEG_W)
        turning = ((v >= left) & (v >= right)) | ((v <= left) & (v <= right)) | (pos == 0) | (pos == ns - 1)
        listed = int(turning.sum()) <= SEG_E and int(core.sum()) <= SEG_C
        out.add("window_listed" if listed else "window_not_listed")
    return out


def branches_of(row, thr, pl):
    return row_branches(np.asarray(row, dtype=np.float32), float(thr), pl)


# ------------------------------------------------------------------------------------------
# row kinds: (ns, seed) -> float32
# ------------------------------------------------------------------------------------------
def _rng(ns, seed):
    # (a SeedSequence, not an int: the table and the branches it is asserted to reach stay pinned under D4W_SEED_SHIFT)
    return np.random.default_rng(np.random.SeedSequence(100003 * seed + ns))


def _smooth(v, k):
    return np.convolve(v, np.ones(k) / k, "same") if len(v) >= k else v


def k_noise(ns, seed):
    return _rng(ns, seed).standard_normal(ns)


def k_quant2(ns, seed):
    return np.round(k_noise(ns, seed) * 2.0) / 2.0


def k_quant3(ns, seed):
    return np.round(k_noise(ns, seed) * 3.0) / 3.0


def k_const(ns, seed):
    return np.full(ns, 0.25)


def k_envelope(ns, seed):
    rng = _rng(ns, seed)
    t = np.arange(ns)
    env = _smooth(0.05 + 0.02 * np.abs(rng.standard_normal(ns)), 9)
    for _ in range(int(rng.integers(3, 14))):
        p, w, a = rng.integers(0, ns), rng.uniform(15, 300), rng.uniform(0.2, 1.0)
        env = env + a * np.exp(-0.5 * ((t - p) / w) ** 2)
    return env


def k_inverted(ns, seed):
    e = k_envelope(ns, seed)
    return e.max() - e


def k_osc(ns, seed):
    rng = _rng(ns, seed)
    t = np.arange(ns)
    slow = 1.2 + np.sin(t * 0.003 + rng.uniform(0, 6)) + 0.3 * _smooth(rng.standard_normal(ns), 31)
    return 0.3 * np.sin(2 * np.pi * t * 23.0 / 200.0) * slow


def k_alternating(ns, seed):
    v = k_noise(ns, seed)
    v[::2] = np.abs(v[::2]) + 4.0
    v[1::2] = -np.abs(v[1::2])
    return v


def k_slow(ns, seed):
    t = np.arange(ns)
    return np.sin(t * 0.0009 + seed) + 0.2 * np.sin(t * 0.7)


def k_ramp(ns, seed):
    return np.linspace(-1.0, 1.0, ns) + 0.05 * np.sin(np.arange(ns) * 0.05 + seed)


def k_burst(ns, seed):
    t = np.arange(ns)
    return 0.01 * k_noise(ns, seed) + 5.0 * np.exp(-0.5 * ((t - 0.6 * ns) / 40.0) ** 2) * np.cos(0.7 * (t - 0.6 * ns))


def k_few_full(ns, seed):
    h = ns // 2
    return np.concatenate([0.2 * k_envelope(ns, seed)[:h], k_osc(ns, seed)[h:] + 0.5])


def k_full_few(ns, seed):
    h = ns // 2
    return np.concatenate([k_osc(ns, seed)[:h] + 0.5, 0.2 * k_envelope(ns, seed)[h:]])


def k_thirds(ns, seed):
    a, b = ns // 3, 2 * (ns // 3)
    e = 0.2 * k_envelope(ns, seed)
    return np.concatenate([e[:a], k_osc(ns, seed)[a:b] + 0.5, e[b:]])


def k_max_first(ns, seed):
    v = k_noise(ns, seed)
    v[0] = 10.0
    return v


def k_max_last(ns, seed):
    v = k_noise(ns, seed)
    v[-1] = 10.0
    return v


def k_peak_at_1(ns, seed):
    v = k_noise(ns, seed)
    v[min(1, ns - 1)] = 10.0
    return v


def k_peak_before_last(ns, seed):
    v = k_noise(ns, seed)
    v[max(ns - 2, 0)] = 10.0
    return v


def k_plateau_ends(ns, seed):
    v = k_noise(ns, seed)
    v[:5] = 9.0
    v[-5:] = 9.0
    return v


def k_plateau_even(ns, seed):
    """Plateaus of 2, 4 and 6 samples: the reported middle rounds down."""
    v = k_noise(ns, seed)
    for k, (at, n) in enumerate(((ns // 5, 2), (ns // 2, 4), (4 * ns // 5, 6), (1, 2), (ns - 3, 2))):
        if 1 <= at and at + n <= ns - 1:
            v[at:at + n] = 7.0 + k
    return v


def _with(v, **at):
    for value, places in at.items():
        for i in places:
            if 0 <= i < len(v):
                v[i] = {"pinf": np.inf, "ninf": -np.inf, "nan": np.nan}[value]
    return v


def k_pinf(ns, seed):
    return _with(k_noise(ns, seed), pinf=[ns // 3])


def k_ninf(ns, seed):
    return _with(k_noise(ns, seed), ninf=[2 * ns // 3])


def k_both_inf(ns, seed):
    return _with(k_noise(ns, seed), pinf=[ns // 3], ninf=[2 * ns // 3] if 2 * ns // 3 != ns // 3 else [])


def k_pinf_at_1(ns, seed):
    return _with(k_noise(ns, seed), pinf=[1])


def k_pinf_smooth(ns, seed):
    return _with(k_envelope(ns, seed), pinf=[ns // 3])


def k_all_nan(ns, seed):
    return np.full(ns, np.nan)


def k_some_nan(ns, seed):
    return _with(k_noise(ns, seed), nan=[ns // 4, ns // 4 + 1, ns // 2, ns - 1])


KINDS = collections.OrderedDict((f.__name__[2:], f) for f in (
    k_noise, k_quant2, k_quant3, k_const, k_envelope, k_inverted, k_osc, k_alternating, k_slow, k_ramp, k_burst, k_few_full,
    k_full_few, k_thirds, k_max_first, k_max_last, k_peak_at_1, k_peak_before_last, k_plateau_ends, k_plateau_even, k_pinf,
    k_ninf, k_both_inf, k_pinf_at_1, k_pinf_smooth, k_all_nan, k_some_nan))
ALL_KINDS = tuple(KINDS)
FEW_KINDS = ("noise", "quant2", "envelope", "osc", "alternating", "plateau_ends", "burst")
BIG_KINDS = ("noise", "envelope", "slow")


def row(kind, ns, seed=0):
    return np.ascontiguousarray(KINDS[kind](ns, seed), dtype=np.float32)


def block(kinds, ns, seed=0):
    return np.stack([row(k, ns, seed + i) for i, k in enumerate(kinds)])


# ------------------------------------------------------------------------------------------
# bars
# ------------------------------------------------------------------------------------------
def row_range(r):
    """max - min of a row in float64 (NaN samples left out; 1 where nothing finite is left)."""
    f = r[np.isfinite(r)].astype(np.float64)
    return float(f.max() - f.min()) if len(f) else 1.0


def bars(x, which):
    """The one-bar launches of a block: 'all' or 'some'; fractions and the exact range are those of row 0 (row 4 where the
    block has an envelope row: the bar 'a fraction of the strongest peak' of the detectors)."""
    span = row_range(x[0])
    env = row_range(x[4]) if len(x) > 4 else span
    out = [0.0, 0.3 * span, 0.45 * env, span, float("nan")]
    if which == "all":
        out += [-1.0, 0.02 * span, 0.9 * span, float(np.nextafter(span, np.inf)), 1e30, float("inf"), float("-inf"), 0.08 * env]
    return out


def row_bars(x):
    """One bar per row, mixed in one launch: 0, negative, NaN, +inf, the row's exact range where float32 holds it, ordinary."""
    out = np.empty(len(x), dtype=np.float32)
    for c, r in enumerate(x):
        span = row_range(r)
        out[c] = (0.0, -1.0, np.nan, np.inf, np.float32(span), 0.3 * span, 0.05 * span, 0.9 * span)[c % 8]
    return out


def float64_product():
    """(scale, value, scale x value in float64, the float32 product, a dip): 8.5 - dip lies between the two products, so a peak
    of 8.5 beside that dip is kept under one of them and dropped under the other."""
    scale, value = 0.1, np.float32(80.000008)
    thr, thr32 = scale * float(value), float(np.float32(scale) * value)
    dip = np.float32(8.5 - 0.5 * (thr + thr32))
    assert thr != thr32 and min(thr, thr32) <= 8.5 - float(dip) < max(thr, thr32)
    return scale, value, thr, thr32, dip


# ------------------------------------------------------------------------------------------
# designed walk rows: exact small integers and halves, one decision per row
# ------------------------------------------------------------------------------------------
DISTANCES = (1, 2, 31, 32, 33, 63, 1023, 1024, 1025, 2047, 2049, None)        # None: to the row end
WALK_BARS = (2.5, 2.1)           # 8 - 2.5 is exact in float32; 8 - 2.1 is 5.9 in float64 and 5.9000001 in float32
PEAK, FILL, STOP, FLOOR, CROWD = 8.0, 7.0, 9.0, -100.0, 140


def dip_values(thr):
    """(the highest dip that still gives the prominence thr, the next float32 above it: one ulp short)."""
    lim = np.float32(PEAK - thr)
    if float(lim) > PEAK - thr:
        lim = np.nextafter(lim, np.float32(-np.inf))
    return lim, np.nextafter(lim, np.float32(np.inf))


def walk_row(ns, p, d, direction, dip_at, dipv, crowd):
    """A peak of 8 at p; towards `direction` the row stays at 7 up to a 9 at distance d (None: up to the row end) but for one
    dip; the other side drops to -100 at once, so this side alone decides.  crowd: 140 further maxima on the other side (the
    row then has more than 128 candidates: a lane per side instead of 16)."""
    x = np.full(ns, FLOOR, dtype=np.float32)
    q = (ns if direction > 0 else -1) if d is None else p + direction * d
    lo, hi = (p + 1, q) if direction > 0 else (q + 1, p)
    x[lo:hi] = FILL
    x[p] = PEAK
    if 0 <= q < ns:
        x[q] = STOP
    if dip_at is not None:
        x[dip_at] = dipv
    if crowd:
        at = p - direction * (4 + 2 * np.arange(CROWD))
        assert at.min() >= 1 and at.max() <= ns - 2
        x[at] = -90.0
    return x


def _placement(p, q, direction, bshift):
    bp, bq = p >> bshift, q >> bshift
    if bp == bq:
        return "same block"
    if bp >> 5 != bq >> 5:
        return "later super-block"
    if bq == bp + direction:
        return "next block"
    if (bq & 31) == (31 if direction > 0 else 0):
        return "last block of the super-block"
    return None


def _dips(p, q, direction, bshift):
    """Positions strictly between p and q: either side of a super-block edge where one lies between, else of a block edge
    (the one farthest from p), else the middle."""
    a, b = min(p, q) + 1, max(p, q) - 1            # the samples between
    if a > b:
        return [None]
    for size in (1 << (bshift + 5), 1 << bshift):
        edges = [e for e in range((a // size + 1) * size, b + 1, size) if a <= e - 1]
        if edges:
            e = edges[-1] if direction > 0 else edges[0]
            return [e - 1, e]
    return [(a + b) // 2]


def designed_rows(ns, full=True, distances=DISTANCES):
    """[(row, description)] for the bars WALK_BARS[k], k = 0, 1: lists [k].  full: every placement of the stopper, both dips
    and both walk forms for every row; else the farthest placement, the first dip, the walk forms in turn."""
    bshift = bshift_of(ns)
    sb = 1 << (bshift + 5)
    margin = 2 * CROWD + 8
    out = [[], []]
    n = 0
    for d in distances:
        for direction in (1, -1):
            found = {}
            for p in range(margin, min(ns - margin, 4 * sb + margin)):
                q = (ns if direction > 0 else -1) if d is None else p + direction * d
                if d is None:
                    if (direction > 0 and ns - p > 3 * sb) or (direction < 0 and p > 3 * sb):
                        continue
                    key = "row end"
                else:
                    if not 1 <= q <= ns - 2:
                        continue
                    key = _placement(p, q, direction, bshift)
                if key and key not in found:
                    found[key] = p
            keys = list(found) if full else list(found)[-1:]
            for key in keys:
                p = found[key]
                q = (ns if direction > 0 else -1) if d is None else p + direction * d
                dips = _dips(p, q, direction, bshift)
                for dip_at in dips if full else dips[:1]:
                    for k, thr in enumerate(WALK_BARS):
                        for short, dipv in enumerate(dip_values(thr)):
                            for crowd in ((False, True) if full else (bool(n & 1),)):
                                n += 1
                                out[k].append((walk_row(ns, p, d, direction, dip_at, dipv, crowd),
                                               "d=%s dir=%+d %s p=%d dip=%s %s%s" % (d, direction, key, p, dip_at,
                                                                                    "one ulp short" if short else "exact",
                                                                                    " crowd" if crowd else "")))
    return out


# ------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name ns kinds bars offset want")

STAGED = (3, 4, 5, 31, 32, 33, 64, 1024, 1025, 2048, 4100, 16383, 16384)
INPLACE = (16385, 16387, 16388, 9 * SEG_S, 9 * SEG_S + 4, 9 * SEG_S + 64, 20000)
LARGE = (131072, 131073, 131076, 262148)
SMALL_INPLACE = (3, 8, 64, 100, 1920, 1984, 2048, 4000, 5764, 12000)          # with D4W_FP_STAGED=0 (one child process)


def _want(ns, offset):
    pl = plan(ns, offset)
    if pl.bshift > 5:
        return {"bshift%d" % pl.bshift, "mark4" if pl.mark4 else "mark_scalar", "walk_lane", "word_rounds"}
    if ns > 100000:                                          # three rows, a few bars: the longest row of 32-sample blocks
        return {"inplace_sweep", "window_few", "window_full", "window_listed", "window_not_listed", "cold_window"} if pl.sweep \
            else {"inplace_scalar", "mark_scalar", "word_rounds", "walk_lane"}
    if pl.staged:
        w = {"staged_vec4" if pl.vec4 else "staged_scalar"}
        if ns >= 1024:
            w |= {"by_block", "by_block_fallback"} if pl.mark4 else {"mark_scalar"}
            w |= {"walk_wave", "walk_lane", "one_list", "early_exit"}
        if ns >= 16383:
            w.add("word_rounds")
        return w
    if pl.sweep:
        return {"inplace_sweep", "window_few", "window_full", "window_listed", "window_not_listed", "resume", "cold_window",
                "mark4"}
    return {"inplace_scalar", "mark_scalar", "word_rounds", "walk_lane", "walk_wave"}


def table():
    cases = []
    for ns in STAGED + INPLACE:
        which = "all" if ns in (33, 2048, 4100, 16388, 20000) else "some"
        cases.append(Case("all kinds", ns, ALL_KINDS, which, 0, _want(ns, 0)))
        if ns % 4 == 0:
            for off in (1, 2, 3):
                cases.append(Case("offset %d" % off, ns, FEW_KINDS, "some", off, _want(ns, off)))
    for ns in LARGE:
        cases.append(Case("large", ns, BIG_KINDS if ns != 131073 else BIG_KINDS[:2], "some", 0, _want(ns, 0)))
        if ns % 4 == 0:
            for off in (1, 2, 3):
                cases.append(Case("large offset %d" % off, ns, BIG_KINDS[:2], "some", off, _want(ns, off)))
    return cases


def case_block(case):
    return block(case.kinds, case.ns, seed=case.ns % 97 + case.offset)


def case_bars(case, x):
    b = bars(x, case.bars)
    if case.ns > 100000:                                     # the longest rows: a few bars
        return b[1:2] if case.offset else b
    return b


def case_branches(case, x, bar_list):
    pl = plan(case.ns, case.offset)
    out = set()
    for thr in bar_list:
        for r in x:
            out |= branches_of(r, thr, pl)
    return out


def aligned(x, offset, alloc):
    """A copy of the block x that starts `offset` floats after a 16-byte boundary.  alloc(n) -> a flat float32 buffer whose
    .ctypes / data pointer arithmetic the caller understands (NumPy here; the hardware tests use their own)."""
    buf = alloc(x.size + 8)
    base = (-(buf.ctypes.data // 4)) % 4
    view = buf[base + offset:base + offset + x.size].reshape(x.shape)
    view[...] = x
    assert (view.ctypes.data % 16) == 4 * (offset % 4)
    return view
