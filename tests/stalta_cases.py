"""The cases tests/test_emu_stalta.py (CPU emulator build, host pointers) and tests/test_stalta_gpu.py (gfx950) both run through
the C ABI against tests/known_answers_stalta.py.  A backend supplies three callables (arrays are NumPy; the backend gives x, prev
and the ratio a row pitch of its own):
    ratio(x, prev, form, nsta, nlta, gap, floor, scale, rstate, nseen) -> (r [nx, ns] float32, rstate_out [nx, 2] float64)
    trigger(r, on, off, active, cap) -> (ev [nx, cap, 3] int32, peak [nx, cap] float32, counts [nx], active_out [nx])
    fused(x, prev, form, nsta, nlta, gap, floor, scale, rstate, nseen, on, off, active, cap) -> trigger's four
prev: [nx, n_prev] float32 or None; rstate: [nx, 2] float64 or None; on / off: [nx] float64; active: [nx] int32 or None."""
import functools

import numpy as np

from tests import known_answers_stalta as ks

T, W = ks.TILE, ks.MAX_WINDOW
NS_FORMS = {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+37": 2 * T + 37}
PARAMS = {"1-1-0": (1, 1, 0), "1-2-0": (1, 2, 0), "5-64-5": (5, 64, 5), "40-1000-40": (40, 1000, 40), "max": (8, W - 8, 8)}
EXTRA = 50                   # the "longer than needed" tail: this many samples more than nlta + gap - 1
# float32 cannot hold a ratio below its subnormal spacing to a RELATIVE bound (the recursive ratio of a dead stretch decays
# through them): the rounding to float32 is absolute there
TINY = 2.0 ** -149


def records(nlta, gap, ns, seed):
    """Six rows of nlta + gap - 1 + EXTRA + ns samples (the block is the last ns): unit noise, noise on an offset of 200,
    noise x 1e-3, zeros, a ramp, the dropout row."""
    nb = nlta + gap - 1 + EXTRA
    L = nb + ns
    rng = np.random.default_rng(seed)
    rec = np.zeros((6, L))
    rec[0] = rng.standard_normal(L)
    rec[1] = rng.standard_normal(L) + 200.0
    rec[2] = rng.standard_normal(L) * 1e-3
    rec[4] = 0.01 * np.arange(L) - 3.0
    third, dead = L // 3, nlta + gap + 200
    rec[5, :third] = 1e4 * rng.standard_normal(third)
    rec[5, third + dead:] = 0.1 * rng.standard_normal(max(0, L - third - dead))
    return rec.astype(np.float32), nb


def tails(nlta, gap):
    need = nlta + gap - 1
    return sorted({0, 3, need, need + EXTRA})


def assert_close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    lim = ks.RTOL * np.abs(ref) + TINY
    assert np.all(err <= lim), what + (float(np.max(err / np.maximum(np.abs(ref), 1e-300))), np.unravel_index(np.argmax(err - lim), err.shape))
    assert np.all(got[ref == 0] == 0), what + ("a zero of the restatement is not exactly 0",)


def assert_clear_of_bar(lta, bar, what):
    """The condition on the INPUTS: no LTA of the restatement within 1e-9 relative of its floor bar."""
    v = lta[np.isfinite(lta)]
    assert np.all(np.abs(v - bar) > 1e-9 * bar), what


def check_kernel_alone(ratio, form, params, ns_form):
    nsta, nlta, gap = PARAMS[params]
    if form == ks.RECURSIVE:
        gap = 0
    ns = NS_FORMS[ns_form]
    rec, nb = records(nlta, gap, ns, 7919 * nsta + 31 * nlta + ns + form)
    x = np.ascontiguousarray(rec[:, nb:])
    scale = np.abs(x).max(axis=1).astype(np.float32)
    for n_prev in tails(nlta, gap):
        what = (form, params, ns, n_prev)
        if form == ks.CLASSIC:
            prev = np.ascontiguousarray(rec[:, nb - n_prev:nb]) if n_prev else None
            got, _ = ratio(x, prev, form, nsta, nlta, gap, ks.FLOOR, scale, None, 0)
            for c in range(6):
                ref, lta, bar = ks.classic(rec[c], nb, n_prev, nsta, nlta, gap, ks.FLOOR, scale[c])
                if scale[c] > 0:
                    assert_clear_of_bar(lta, bar, what + (c,))
                assert_close(got[c], ref, what + (c,))
                if n_prev < nlta + gap - 1:                  # zeros until the window is full
                    assert np.all(got[c, :nlta + gap - 1 - n_prev] == 0)
        else:
            states = [ks.recursive(rec[c, nb - n_prev:nb], nsta, nlta, ks.FLOOR, 1.0)[3] for c in range(6)]
            rin = np.array([[s[0], s[1]] for s in states], dtype=np.float64) if n_prev else None
            got, rout = ratio(x, None, form, nsta, nlta, 0, ks.FLOOR, scale, rin, n_prev)
            for c in range(6):
                ref, lta, bar, end = ks.recursive(x[c], nsta, nlta, ks.FLOOR, scale[c], states[c])
                if scale[c] > 0:
                    assert_clear_of_bar(lta, bar, what + (c,))
                assert_close(got[c], ref, what + (c,))
                # (float64 on both sides, in another order; a state that has decayed into the subnormals has no relative precision)
                assert np.allclose(rout[c], end[:2], rtol=1e-12, atol=1e-300), what + (c, "state")
    # the dropout row's dead stretch, where the block holds it: exact zeros once the LTA window is inside it
    if form == ks.CLASSIC:
        L = rec.shape[1]
        a, b = L // 3 + nlta + gap - 1 - nb, L // 3 + nlta + gap + 200 - nb
        if 0 <= a < min(b, ns):
            assert np.all(got[5, a:min(b, ns)] == 0)


def check_dead_and_gain(ratio):
    """A row with A = 0 gives zeros whatever it holds; a row scaled by 2^-20 (its scale with it) gives the same bits."""
    nsta, nlta, gap = 5, 64, 5
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 700)).astype(np.float32)
    x[2] = x[1] * np.float32(2.0 ** -20)
    scale = np.array([0.0, 1.0, 2.0 ** -20], dtype=np.float32)
    for form, g in ((ks.CLASSIC, gap), (ks.RECURSIVE, 0)):
        got, _ = ratio(x, None, form, nsta, nlta, g, ks.FLOOR, scale, None, 0)
        assert np.all(got[0] == 0) and np.any(got[1] != 0)
        assert np.array_equal(got[1], got[2])


# ------------------------------------------------------------------------------------------
# the trigger on hand-made ratios
# ------------------------------------------------------------------------------------------
def trigger_rows():
    ns = 2 * T + 100
    r = np.full((10, ns), 2.0, dtype=np.float32)             # between the thresholds 3 / 1.5 wherever nothing is said
    on, off = np.full(10, 3.0), np.full(10, 1.5)
    active = np.zeros(10, dtype=np.int32)
    r[0, 0], r[0, 4], r[0, 10] = 5.0, 7.0, 1.0                # ON at sample 0
    r[1, T - 5], r[1, T + 2], r[1, T + 7] = 4.0, 9.0, 0.0     # an event across one tile boundary
    r[1, 2 * T - 1], r[1, 2 * T], r[1, 2 * T + 1] = 3.5, 3.5, -1.0     # ... and a tie across the next: the first wins
    r[2, T - 100], r[2, T + 900], r[2, 2 * T + 50] = 3.5, 8.0, 1.0     # an event across two boundaries, its peak in the middle tile
    active[3] = 1                                             # active on entry, no OFF: one event (-1, ns)
    r[3, 2 * T + 90] = 2.5
    active[4] = 1                                             # active on entry, OFF at sample 0
    r[4, 0] = 0.5
    r[5, 0::2], r[5, 1::2] = 4.0, 1.0                         # alternating: ceil(ns / 2) events
    r[5, 6] = 6.0
    r[6, 100], r[6, 101:104], r[6, 104], r[6, 110] = 4.0, np.nan, 3.8, 0.0   # NaNs inside an event are KEEP
    r[6, 300], r[6, 301] = np.nan, np.nan                     # ... and outside one
    on[7], off[7] = 3.0, 3.0                                  # thr_on == thr_off: a sample AT the bar keeps the flag
    r[7, 50], r[7, 51], r[7, 52], r[7, 53] = 3.5, 3.0, 2.9, 3.0
    on[8], off[8] = 1.9, 0.5                                  # per-channel bars: this row is active from sample 0 to the end
    # row 9: nothing
    return r, on, off, active


def check_trigger(trigger):
    r, on, off, active = trigger_rows()
    nx, ns = r.shape
    want = [ks.trigger(r[c], on[c], off[c], bool(active[c])) for c in range(nx)]
    assert [len(w[0]) for w in want] == [1, 2, 1, 1, 1, (ns + 1) // 2, 1, 1, 1, 0]
    assert want[3][0][0][:2] == (-1, ns) and want[4][0][0][:3] == (-1, 0, 0) and want[1][0][1][:3] == (2 * T - 1, 2 * T + 1, 2 * T - 1)
    for cap in (4, ns // 2 + 1):
        ev, peak, counts, act = trigger(r, on, off, active, cap)
        assert counts.tolist() == [len(w[0]) for w in want]                  # the need, whatever the cap
        assert act.tolist() == [int(w[1]) for w in want]
        for c in range(nx):
            n = min(cap, len(want[c][0]))
            assert [tuple(e) for e in ev[c, :n].tolist()] == [w[:3] for w in want[c][0][:n]], (cap, c)
            assert np.array_equal(peak[c, :n].view(np.uint32), np.array([w[3] for w in want[c][0][:n]], dtype=np.float32).view(np.uint32)), (cap, c)
    # one row, one sample; and a pitch-free single tile
    for val, flag, exp in ((5.0, 0, [(0, 1, 0)]), (2.0, 0, []), (2.0, 1, [(-1, 1, 0)]), (1.0, 1, [(-1, 0, 0)])):
        ev, peak, counts, act = trigger(np.array([[val]], dtype=np.float32), np.array([3.0]), np.array([1.5]), np.array([flag], dtype=np.int32), 1)
        assert [tuple(e) for e in ev[0, :counts[0]].tolist()] == exp


# ------------------------------------------------------------------------------------------
# the scene
# ------------------------------------------------------------------------------------------
def scene_scale():
    return np.abs(ks.scene()).max(axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene_reference(form):
    """(ratios float64 [8, 18000], events per channel) of the whole record, computed once and left unchanged; asserts the
    condition the event tests rest on -- no ratio of the restatement within 8 x 2^-24 relative of a threshold."""
    x, scale = ks.scene(), scene_scale()
    a = ks.CLASSIC_ARGS if form == ks.CLASSIC else ks.RECURSIVE_ARGS
    rows = []
    for c in range(ks.NX):
        if form == ks.CLASSIC:
            r, lta, bar = ks.classic(x[c], 0, 0, a["nsta"], a["nlta"], a["gap"], ks.FLOOR, scale[c])
        else:
            r, lta, bar, _ = ks.recursive(x[c], a["nsta"], a["nlta"], ks.FLOOR, scale[c])
        assert_clear_of_bar(lta, bar, ("scene", form, c))
        rows.append(r)
    r = np.array(rows)
    for thr in (a["thr_on"], a["thr_off"]):
        assert np.min(np.abs(r - thr)) > 8 * 2.0 ** -24 * thr, (form, thr, float(np.min(np.abs(r - thr)) / thr))
    events = [ks.trigger(r[c].astype(np.float32), a["thr_on"], a["thr_off"])[0] for c in range(ks.NX)]
    assert all(len(e) == 5 for e in events), [len(e) for e in events]
    if form == ks.CLASSIC:
        assert [e[:2] for e in events[0]] == ks.CHANNEL0
    r.setflags(write=False)
    return r, events


def event_table(ev, peak, counts):
    """The rows' events as lists of (on, off, peak index, peak bits)."""
    return [[tuple(e) + (int(np.float32(p).view(np.uint32)),) for e, p in zip(ev[c, :counts[c]].tolist(), peak[c, :counts[c]])]
            for c in range(len(counts))]


def split_at_seams(events):
    """What three files of NFILE samples report for the record's events: one straddling a seam arrives as (on, NFILE) in one file
    and (-1, off) in the next.  -> per file, per channel, a list of (on, off) in the file's own indices."""
    out = [[[] for _ in events] for _ in range(ks.NS // ks.NFILE)]
    for c, evs in enumerate(events):
        for on, off in (e[:2] for e in evs):
            for f in range(len(out)):
                lo, hi = f * ks.NFILE, (f + 1) * ks.NFILE
                # a file reports the event if it starts there, or if the flag is up on entry (an OFF at the file's first
                # sample then closes it at once: (-1, 0))
                if lo <= on < hi or on < lo <= off:
                    out[f][c].append((on - lo if on >= lo else -1, off - lo if off < hi else ks.NFILE))
    return out


def check_scene(ratio, trigger, fused, form):
    """(a) the ratio of the whole record, (b) its events, (c) three files chained by tail / state, (d) the fused form."""
    x, scale = ks.scene(), scene_scale()
    a = ks.CLASSIC_ARGS if form == ks.CLASSIC else ks.RECURSIVE_ARGS
    nsta, nlta, gap = a["nsta"], a["nlta"], a["gap"]
    on, off = np.full(ks.NX, a["thr_on"]), np.full(ks.NX, a["thr_off"])
    ref, events = scene_reference(form)
    cap = 16
    r, _ = ratio(x, None, form, nsta, nlta, gap, ks.FLOOR, scale, None, 0)                       # (a)
    assert_close(r, ref, ("scene", form))
    ev, peak, counts, act = trigger(r, on, off, None, cap)                                       # (b)
    assert counts.tolist() == [5] * ks.NX and not act.any()
    for c in range(ks.NX):
        assert [tuple(e[:2]) for e in ev[c, :5].tolist()] == [e[:2] for e in events[c]], c
        # the peak: the first largest sample of the run in the ratio the trigger was given (the restatement's ratio, rounded
        # on its own, may order two near-equal samples the other way), its value bit for bit
        assert ev[c, :5, 2].tolist() == [b0 + int(np.argmax(r[c, b0:b1])) for b0, b1 in (e[:2] for e in events[c])], c
        assert np.array_equal(peak[c, :5], r[c, ev[c, :5, 2]])
    fv = fused(x, None, form, nsta, nlta, gap, ks.FLOOR, scale, None, 0, on, off, None, cap)      # (d)
    assert event_table(*fv[:3]) == event_table(ev, peak, counts) and np.array_equal(fv[3], act)
    # (c) three files
    want = split_at_seams(events)
    need = nlta + gap - 1
    rstate, active, rows = None, None, []
    for f in range(ks.NS // ks.NFILE):
        blk = np.ascontiguousarray(x[:, f * ks.NFILE:(f + 1) * ks.NFILE])
        prev = np.ascontiguousarray(x[:, max(0, f * ks.NFILE - need):f * ks.NFILE]) if f and form == ks.CLASSIC else None
        rf, rnext = ratio(blk, prev, form, nsta, nlta, gap, ks.FLOOR, scale, rstate, f * ks.NFILE)
        assert_close(rf, ref[:, f * ks.NFILE:(f + 1) * ks.NFILE], ("scene file", form, f))
        evf, pkf, cntf, actf = trigger(rf, on, off, active, cap)
        for c in range(ks.NX):
            assert [tuple(e[:2]) for e in evf[c, :cntf[c]].tolist()] == want[f][c], (form, f, c)
        ff = fused(blk, prev, form, nsta, nlta, gap, ks.FLOOR, scale, rstate, f * ks.NFILE, on, off, active, cap)
        assert event_table(*ff[:3]) == event_table(evf, pkf, cntf) and np.array_equal(ff[3], actf)
        rstate, active = rnext, actf
        rows.append(rf)
    assert any(e[1] == ks.NFILE for evs in want[0] for e in evs) and any(e[0] == -1 for evs in want[2] for e in evs)
