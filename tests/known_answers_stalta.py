"""float64 restatement of the STA/LTA detector and its trigger (csrc/stalta.hip, detect.sta_lta / trigger_onset /
sta_lta_events) and the scene its tests share.  No reference counterpart: the definition is DESIGN.md 3.3c.

With e[i] = x[i]^2 in float64 (x float32), samples before the block at negative i:
    classic     STA[i] = mean e[i-nsta+1 .. i],  LTA[i] = mean e[i-gap-nlta+1 .. i-gap]
                r[i] = STA / LTA where both windows lie in known samples and LTA > (floor A)^2, 0 elsewhere
    recursive   sta[i] = sta[i-1] + (e[i] - sta[i-1]) / nsta, lta likewise; r = sta / lta where nlta samples have been seen and
                lta > (floor A)^2, 0 elsewhere
Window sums are formed DIRECTLY per window (NumPy's pairwise sum over the window's own samples: all terms non-negative, error
~ log2(n) 2^-53 of the sum), never as differences of a cumulative sum.  The recursive form and the trigger are plain loops.

Bound: the kernel may round the two means and the quotient to float32 -- |got - ref| <= 4 x 2^-24 |ref|; where the restatement
gives 0 the kernel must give exactly 0.  The decision LTA > (floor A)^2 is compared on inputs whose LTA keeps 1e-9 relative away
from the bar (tests/stalta_cases.py asserts it)."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

TILE = 2048                  # d4w_stalta_tile()
MAX_WINDOW = 16384           # d4w_stalta_max_window()
FLOOR = 1e-6
RTOL = 4.0 * 2.0 ** -24
CLASSIC, RECURSIVE = 0, 1


def window_sums(e, n, ends):
    """sum e[end - n + 1 .. end] for every end in `ends` (each >= n - 1), every window summed on its own."""
    v = sliding_window_view(e, n)
    out = np.empty(len(ends), dtype=np.float64)
    step = max(1, 4_000_000 // n)
    for a in range(0, len(ends), step):
        out[a:a + step] = v[ends[a:a + step] - n + 1].sum(axis=1)
    return out


def classic(rec, nb, n_prev, nsta, nlta, gap, floor, A):
    """rec: float32 record whose last len(rec) - nb samples are the block, the n_prev <= nb before it known.
    -> (r float64 [ns], LTA float64 [ns] (NaN where no window), bar)."""
    e = np.asarray(rec, dtype=np.float64) ** 2
    ns = len(rec) - nb
    assert 0 <= n_prev <= nb
    i = np.arange(ns)
    known = i - (max(nsta, nlta + gap) - 1) >= -n_prev
    r, lta = np.zeros(ns), np.full(ns, np.nan)
    bar = (floor * float(A)) ** 2
    if known.any():
        at = i[known] + nb
        sta = window_sums(e, nsta, at) / nsta
        lta[known] = window_sums(e, nlta, at - gap) / nlta
        ok = (lta[known] > bar) & (float(A) > 0)
        q = np.zeros(len(at))
        q[ok] = sta[ok] / lta[known][ok]
        r[known] = q
    return r, lta, bar


def recursive(x, nsta, nlta, floor, A, state=(0.0, 0.0, 0)):
    """-> (r float64 [ns], lta [ns], bar, (sta, lta, seen) after the block)"""
    sta, lta, seen = float(state[0]), float(state[1]), int(state[2])
    bar = (floor * float(A)) ** 2
    r, ltas = np.zeros(len(x)), np.zeros(len(x))
    for i, v in enumerate(np.asarray(x, dtype=np.float64)):
        e = v * v
        # sta + (e - sta) / n written without its subtraction: taken literally, e - sta rounds relative to the OLD state, and
        # a quiet sample behind a loud one (n = 1: the answer is e itself) comes out 1e-7 off in float64.  All terms are
        # non-negative here: 3 x 2^-53 per step, decaying like the state itself.
        sta = ((nsta - 1) * sta + e) / nsta
        lta = ((nlta - 1) * lta + e) / nlta
        seen += 1
        ltas[i] = lta
        if seen >= nlta and float(A) > 0 and lta > bar:
            r[i] = sta / lta
    return r, ltas, bar, (sta, lta, seen)


def trigger(r, on, off, active=False):
    """Events of one row: a list of (on, off, peak index, peak) and the flag after the last sample."""
    ev, cur, s = [], None, bool(active)
    if s:
        cur = [-1, None, 0, np.float32(-np.inf)]
    for i, v in enumerate(r):
        s2 = True if v > on else (False if v < off else s)
        if s2 and not s:
            cur = [i, None, i, np.float32(-np.inf)]
        if s2 and v > cur[3]:
            cur[2], cur[3] = i, v
        if s and not s2:
            cur[1] = i
            ev.append(tuple(cur))
            cur = None
        s = s2
    if s:
        cur[1] = len(r)
        ev.append(tuple(cur))
    return ev, s


# ------------------------------------------------------------------------------------------
# the scene: 8 channels x 18000 samples at 200 Hz, five 20 Hz calls per channel, channel 6 a thousand times quieter
# ------------------------------------------------------------------------------------------
FS, NX, NS, NFILE = 200.0, 8, 18000, 6000
CLASSIC_ARGS = dict(nsta=100, nlta=2000, gap=100, thr_on=3.0, thr_off=1.5)
RECURSIVE_ARGS = dict(nsta=100, nlta=2000, gap=0, thr_on=2.5, thr_off=1.2)
CHANNEL0 = [(2878, 3032), (5994, 6158), (8967, 9133), (11944, 12117), (15067, 15238)]


def scene():
    rng = np.random.default_rng(20261021)
    x = rng.standard_normal((NX, NS))
    t = np.arange(200) / FS
    for c in range(NX):
        for k, t0 in enumerate((14.0 + 0.05 * c, 29.6 + 0.03 * c, 44.5, 59.4 + 0.02 * c, 75.0)):
            at = int(round(FS * t0))
            x[c, at:at + 200] += (5.0 + 0.5 * k) * np.hanning(200) * np.sin(2 * np.pi * 20.0 * t)
    x[6] *= 1e-3
    return x.astype(np.float32)
