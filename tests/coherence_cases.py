"""The cases of the coherence of located calls (csrc/coherence.hip) that tests/test_emu_coherence.py (CPU emulator, C ABI) and
tests/test_coherence_gpu.py (hardware, dw.loc.beam_coherence) both run, against tests/known_answers_coherence.py.

A runner is
    run(buf, ns, nxt, ns2, ibuf, inxt, delays, order, weights, start, nt, H, peak_range=None)
        -> dict(beam, semblance, phase or None, wsum: float32 [ncalls x nt]; peak float32 [ncalls]; peak_index int32 [ncalls])
where buf is float32 [nch x pitch >= ns] and the block is buf[:, :ns] (pitch > ns: the rows are read in place), nxt the next
block [nch x pitch2 >= ns2] or None, ibuf / inxt the imaginary blocks laid out like buf / nxt or None (no phase), delays r int32
[ncalls x nch] for order 0 and (k int32, f float32) otherwise, weights float32 [nch] or None, start int64 [ncalls].
A beam runner is beam_cases' run(buf, ns, nxt, ns2, delays, order, weights, start, nt, normalize).

The shapes are the smallest at which the kernels can still go wrong: one channel, a few, a second segment of two channels
(130) and a third of one (257); one column, one short of a column tile of 1024, one past it, and two tiles and a bit, so that
windows cross a tile; half windows 0, 3, 40 and the limit.

Condition: the derived semblance tolerance is <= 1e-4 on every compared element of every case (reference() asserts it, so a
larger scene cannot quietly loosen the test); no element is excluded.  Largest bound over the cases below: 6.8e-5 (the limit H = 256, where the window sums alone allow 6.1e-5).
"""
import functools

import numpy as np

from tests import known_answers_beam as kb
from tests import known_answers_coherence as kc
from tests.beam_cases import padded, positions
from tests.known_answers_loc import C0, make_cable

FS = 10.0                                                    # the tables are handed over: the rate only sets the moveout's span
SEMBLANCE_TOL_MAX = 1e-4
H_LIMIT = "limit"

# (nch, nt, ns, ncalls, H, order, weights, start, next block, wide pitch, phase)
#   weights: "none", "mixed" (non-uniform, all > 0), "zeros" (non-uniform with zeros, the rows under them NaN)
#   start: "neg" (before the record), "mid", "end" (the last columns run off the end of the record)
CASES = (
    (1, 1, 1500, 1, 0, 0, "none", "mid", False, False, False),
    (1, 1025, 1600, 2, 3, 1, "none", "neg", True, True, True),
    (5, 1, 1500, 2, 3, 3, "mixed", "mid", False, True, True),
    (5, 1023, 1500, 3, 40, 3, "mixed", "neg", False, True, True),
    (5, 2100, 3000, 1, H_LIMIT, 1, "zeros", "end", True, False, False),
    (130, 1025, 2000, 2, 0, 0, "zeros", "neg", True, True, True),
    (130, 2100, 2500, 1, 40, 3, "none", "end", False, False, False),
    (130, 1025, 1800, 1, H_LIMIT, 3, "mixed", "mid", False, True, True),
    (257, 1023, 1800, 3, 3, 1, "mixed", "end", True, True, True),
    (257, 2100, 2400, 1, 40, 0, "none", "neg", False, False, False),
    (257, 1025, 2000, 2, 0, 3, "zeros", "mid", True, False, True),
    (130, 1023, 1500, 3, 3, 0, "none", "mid", False, False, True),
)
AXES = ((1, 5, 130, 257), (1, 1023, 1025, 2100), None, (1, 2, 3), (0, 3, 40, H_LIMIT), (0, 1, 3), ("none", "mixed", "zeros"),
        ("neg", "mid", "end"), (False, True), (False, True), (False, True))


def case_id(c):
    return "nch%d-nt%d-ns%d-c%d-H%s-o%d-w%s-%s-nb%d-wide%d-ph%d" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], c[10])


def burst(u):
    """A 200-sample tone of period 20 under a Hann window at the (fractional) sample offsets u, 0 outside; float64."""
    live = (u >= 0) & (u <= 199)
    return np.where(live, np.sin(2 * np.pi * u / 20.0) * 0.5 * (1 - np.cos(2 * np.pi * u / 199.0)), 0.0)


def weight_set(kind, nch, rng):
    if kind == "none":
        return None
    w = (rng.integers(1, 9, nch) / 4.0).astype(np.float32) * np.float32(1.1)        # not on a binary grid: the weight sums round
    if kind == "zeros" and nch > 1:
        w[rng.random(nch) < 0.3] = 0.0
        w[0], w[-1] = 0.0, 1.5
    return w


def analytic_imag(whole):
    """imag(hilbert) of every row of the joined record, float32."""
    from scipy import signal
    return np.imag(signal.hilbert(np.asarray(whole, dtype=np.float64), axis=1)).astype(np.float32)


def make_case(case, Hmax):
    nch, nt, ns, ncalls, H, order, wkind, skind, nxt, wide, phase = case
    H = Hmax if H == H_LIMIT else H
    rng = np.random.default_rng(9100 + 7 * nch + nt + 13 * order)
    cable = make_cable("bent" if nch % 2 else "line", max(nch, 2))[:nch]
    t = kb.tau(cable, C0, FS, positions(cable, FS, ncalls, nch))
    delays = kb.rounded(t) if order == 0 else kb.split(t)
    ns2 = 700 if nxt else 0
    ntot = ns + ns2
    base = {"neg": -37, "mid": 100, "end": ntot - nt // 2 - int(np.median(t[0]))}[skind]
    start = (base + np.array([0, -5, 11])[:ncalls]).astype(np.int64)
    w = weight_set(wkind, nch, rng)
    # unit-variance noise plus a coherent burst of amplitude 2 along the moveout of call 0, emitted 60 samples into its beam
    n = np.arange(ntot, dtype=np.float64)
    whole = rng.standard_normal((nch, ntot))
    for ch in range(nch):
        whole[ch] += 2.0 * burst(n - (start[0] + 60 + t[0, ch]))
    whole = whole.astype(np.float32)
    im = analytic_imag(whole) if phase else None
    cut = lambda a: (a[:, :ns].copy(), a[:, ns:].copy() if ns2 else None)
    x, nb = cut(whole)
    ix, inb = cut(im) if phase else (None, None)
    return x, nb, ix, inb, delays, order, w, start, nt, H, wide


@functools.lru_cache(maxsize=None)
def reference(case, Hmax):
    """The case, its buffers and its float64 answer, computed once for every test that needs them (left unchanged by all)."""
    x, nb, ix, inb, delays, order, w, start, nt, H, wide = make_case(case, Hmax)
    ref = kc.coherence_ref(x, delays, order, start, nt, H, w, nb, ix, inb)
    worst = float(ref["tol_semblance"].max())
    assert worst <= SEMBLANCE_TOL_MAX, "the derived semblance tolerance of %s reaches %.3g" % (case_id(case), worst)
    bufs = [padded(a, wide, w) if a is not None else None for a in (x, nb, ix, inb)]
    for a in bufs + [w, start] + list(ref.values()) + list(delays if isinstance(delays, tuple) else (delays,)):
        if a is not None:
            a.setflags(write=False)
    return bufs, x.shape[1], (nb.shape[1] if nb is not None else 0), delays, order, w, start, nt, H, ref


def within(got, ref, tol):
    return kb.worst_ratio(got, ref, tol)


def check_parity(run, beam_run, case, Hmax):
    """Runs the case; returns the worst error / tolerance of (semblance, phase)."""
    (buf, nbuf, ibuf, inbuf), ns, ns2, delays, order, w, start, nt, H, ref = reference(case, Hmax)
    lo, hi = (nt // 3, nt // 3 + max(1, nt // 2)) if nt > 2 else (0, nt)
    got = run(buf, ns, nbuf, ns2, ibuf, inbuf, delays, order, w, start, nt, H, (lo, hi))
    for name in ("beam", "semblance", "wsum"):
        assert got[name].dtype == np.float32 and got[name].shape == ref[name].shape, name
        assert np.all(np.isfinite(got[name])), name          # no padding, no row under weight 0 was read
    # the beam is the beam's own, bit for bit
    assert np.array_equal(got["beam"], beam_run(buf, ns, nbuf, ns2, delays, order, w, start, nt, False))
    assert within(got["beam"], ref["beam"], ref["tol_beam"]) <= 1.0
    assert within(got["wsum"], ref["wsum"], ref["tol_wsum"]) <= 1.0
    ws = within(got["semblance"], ref["semblance"], ref["tol_semblance"])
    err = float(np.abs(got["semblance"] - ref["semblance"]).max())
    print("%s: semblance worst error %.3g, largest tolerance %.3g, worst ratio %.3g" % (case_id(case), err, ref["tol_semblance"].max(), ws))
    assert ws <= 1.0, ws
    assert got["semblance"].min() >= 0.0 and got["semblance"].max() <= 1.0 + 1e-4
    wp = 0.0
    if ibuf is None:
        assert got["phase"] is None
    else:
        assert got["phase"].dtype == np.float32 and np.all(np.isfinite(got["phase"]))
        wp = within(got["phase"], ref["phase"], ref["tol_phase"])
        print("%s: phase worst error %.3g, largest tolerance %.3g, worst ratio %.3g"
              % (case_id(case), np.abs(got["phase"] - ref["phase"]).max(), ref["tol_phase"].max(), wp))
        assert wp <= 1.0, wp
        assert got["phase"].min() >= 0.0 and got["phase"].max() <= 1.0 + 1e-4
    peak, index = kc.first_peak(got["semblance"], lo, hi)
    assert got["peak"].dtype == np.float32 and got["peak_index"].dtype == np.int32
    assert np.array_equal(got["peak"], peak) and np.array_equal(got["peak_index"], index)
    if w is not None and not w.any():
        assert not got["semblance"].any() and not got["beam"].any()
    return ws, wp


# ---- exact known answers -----------------------------------------------------------------------------------------------------
def _integer_scene(nch, signs, seed=5):
    """Small-integer samples (|v| <= 15) repeated on nch channels along an exact integer moveout, zeros elsewhere:
    (x, r, start, nt, the columns that hold signal)."""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 90, (1, nch)).astype(np.int32)
    g = rng.integers(-15, 16, 40).astype(np.float32)
    g[g == 0] = 7.0
    g[10:14] = 0.0                                           # a gap of zeros inside the signal
    ns, start, nt = 400, np.array([20], dtype=np.int64), 120
    x = np.zeros((nch, ns), dtype=np.float32)
    for ch in range(nch):
        x[ch, 20 + 30 + r[0, ch]:20 + 30 + r[0, ch] + 40] = g * signs[ch]
    sig = np.zeros(nt, dtype=bool)
    sig[30:70] = g != 0
    return x, r, start, nt, sig


def _holds(sig, H):
    """Whether the window of every column holds a column of signal."""
    return kc.window_sum(sig.astype(np.float64)[None, :], H)[0] > 0


def check_exact_one(run):
    """Every float32 operation is exact: semblance is 1.0 exactly where the window holds signal and 0.0 exactly elsewhere."""
    x, r, start, nt, sig = _integer_scene(128, np.ones(128, dtype=np.float32))
    for H in (0, 1):
        got = run(x, x.shape[1], None, 0, None, None, r, 0, None, start, nt, H)
        assert np.array_equal(got["semblance"][0], _holds(sig, H).astype(np.float32))
        assert np.array_equal(got["wsum"], np.full((1, nt), 128.0, dtype=np.float32))
        assert np.array_equal(got["peak"], [1.0]) and np.array_equal(got["peak_index"], [np.flatnonzero(_holds(sig, H))[0]])


def check_exact_zero(run):
    """Alternating signs on an even channel count: the beam and the semblance are 0.0 exactly, the phase 0 within its bound."""
    signs = np.where(np.arange(128) % 2, -1.0, 1.0).astype(np.float32)
    x, r, start, nt, sig = _integer_scene(128, signs)
    ix = np.roll(x, 1, axis=1) * np.float32(0.5)             # any imaginary block with the same signs
    for H in (0, 1):
        got = run(x, x.shape[1], None, 0, ix, None, r, 0, None, start, nt, H)
        ref = kc.coherence_ref(x, r, 0, start, nt, H, None, None, ix, None)
        assert not got["semblance"].any() and not got["beam"].any()
        assert np.abs(ref["phase"]).max() <= 1e-12 and np.all(np.abs(got["phase"]) <= ref["tol_phase"])
        assert np.array_equal(got["peak"], [0.0]) and np.array_equal(got["peak_index"], [0])


def check_phase_one(run, S):
    """One analytic signal on all channels, any positive gains: phase is 1 within its bound wherever it is not 0 / 0."""
    rng = np.random.default_rng(3)
    for nch in (7, S + 2):
        r = rng.integers(0, 50, (1, nch)).astype(np.int32)
        gains = (0.1 + 10.0 * rng.random(nch)).astype(np.float32)
        n = np.arange(500, dtype=np.float64)
        x, ix = np.zeros((nch, 500), dtype=np.float32), np.zeros((nch, 500), dtype=np.float32)
        for ch in range(nch):
            env = 1.0 + 0.5 * np.sin(0.013 * (n - r[0, ch]))
            x[ch] = gains[ch] * env * np.cos(0.31 * (n - r[0, ch]) + 0.4)
            ix[ch] = gains[ch] * env * np.sin(0.31 * (n - r[0, ch]) + 0.4)
        start, nt = np.array([5], dtype=np.int64), 300
        w = (0.5 + rng.random(nch)).astype(np.float32)
        got = run(x, 500, None, 0, ix, None, r, 0, w, start, nt, 2)
        ref = kc.coherence_ref(x, r, 0, start, nt, 2, w, None, ix, None)
        # the planted values are float32 roundings of one analytic signal: their phases agree to 2 u of a unit vector's angle
        assert np.all(np.abs(ref["phase"] - 1.0) <= 4 * kc.U)
        assert np.all(np.abs(got["phase"] - 1.0) <= ref["tol_phase"] + 4 * kc.U)


def check_bit_identity(run, Hmax):
    """Bit for bit: a repeated call; the record scaled by 2^-3 and 2^5 (semblance); a call alone against row 1 of three."""
    case = next(c for c in CASES if c[0] == 257 and c[3] == 3)
    (buf, nbuf, ibuf, inbuf), ns, ns2, delays, order, w, start, nt, H, _ = reference(case, Hmax)
    first = run(buf, ns, nbuf, ns2, ibuf, inbuf, delays, order, w, start, nt, H)
    again = run(buf, ns, nbuf, ns2, ibuf, inbuf, delays, order, w, start, nt, H)
    for name in ("beam", "semblance", "phase", "wsum", "peak", "peak_index"):
        assert np.array_equal(first[name], again[name]), name
    assert first["semblance"].any() and first["phase"].any()
    for p in (-3, 5):
        s = np.float32(2.0 ** p)
        scaled = run(buf * s, ns, nbuf * s, ns2, ibuf * s, inbuf * s, delays, order, w, start, nt, H)
        assert np.array_equal(scaled["semblance"], first["semblance"]) and np.array_equal(scaled["beam"], first["beam"] * s)
        assert np.array_equal(scaled["peak"], first["peak"]) and np.array_equal(scaled["peak_index"], first["peak_index"])
    one = tuple(a[1:2] for a in delays) if order else delays[1:2]
    alone = run(buf, ns, nbuf, ns2, ibuf, inbuf, one, order, w, start[1:2], nt, H)
    for name in ("beam", "semblance", "phase", "wsum", "peak", "peak_index"):
        assert np.array_equal(alone[name][0], first[name][1]), name


def check_next_block(run, Hmax):
    """The record in two blocks equals the joined record bit for bit, whatever the pitch of either."""
    case = next(c for c in CASES if c[0] == 130 and c[8] and c[10])
    (buf, nbuf, ibuf, inbuf), ns, ns2, delays, order, w, start, nt, H, _ = reference(case, Hmax)
    whole = np.concatenate([buf[:, :ns], nbuf[:, :ns2]], axis=1)
    iwhole = np.concatenate([ibuf[:, :ns], inbuf[:, :ns2]], axis=1)
    late = start + (ns - 300 - start[0])                    # the moveouts cross the seam
    a = run(buf, ns, nbuf, ns2, ibuf, inbuf, delays, order, w, late, nt, 3)
    b = run(whole, ns + ns2, None, 0, iwhole, None, delays, order, w, late, nt, 3)
    alone = run(buf, ns, None, 0, ibuf, None, delays, order, w, late, nt, 3)
    for name in ("beam", "semblance", "phase", "wsum"):
        assert np.array_equal(a[name], b[name]) and np.all(np.isfinite(a[name])), name
    assert not np.array_equal(a["wsum"], alone["wsum"])      # without the next block the far channels drop out


def check_peak_range(run):
    """peak and peak_index are the first maximum inside the range, not the row's."""
    x, r, start, nt, sig = _integer_scene(128, np.ones(128, dtype=np.float32))
    x[:, :] *= np.float32(1.0)
    x[:64, :] *= np.float32(-1.0)                            # semblance 0 everywhere: every column ties at 0.0
    got = run(x, x.shape[1], None, 0, None, None, r, 0, None, start, nt, 0, (17, 60))
    assert np.array_equal(got["peak"], [0.0]) and np.array_equal(got["peak_index"], [17])
    rng = np.random.default_rng(8)
    y = rng.standard_normal((6, 700)).astype(np.float32)
    rr = np.zeros((2, 6), dtype=np.int32)
    for rg in ((0, 600), (0, 1), (599, 600), (250, 263), (3, 515)):
        got = run(y, 700, None, 0, None, None, rr, 0, None, np.array([0, 50], dtype=np.int64), 600, 3, rg)
        peak, index = kc.first_peak(got["semblance"], *rg)
        assert np.array_equal(got["peak"], peak) and np.array_equal(got["peak_index"], index)


# ---- the scene: a true call and a louder incoherent decoy --------------------------------------------------------------------
SCENE_FS, SCENE_NCH, SCENE_NS, SCENE_H, SCENE_NT, SCENE_LONG = 200.0, 64, 4000, 50, 300, 3600
SCENE_STARTS = (750, 2450)                                   # 50 samples before the emission of the call and of the decoy


@functools.lru_cache(maxsize=None)
def scene():
    """64 channels x 4000 samples of unit-variance noise at 200 Hz on a bent cable of 3 km radius.  A true call: a one-second
    20 Hz burst of amplitude 1 along the exact moveout of position 0, emitted at sample 800.  A decoy: the same burst ten times
    louder around the moveout of position 1 from sample 2500, every channel delayed by its own random -15 .. 15 samples (three
    periods): louder in the beam than the call, and coherent with nothing.
    dict(cable, pos, x float32, clean float32 (the call alone), imag float32, delays (k, f) toward both positions)."""
    from tests.beam_cases import E2E_SOURCE
    rng = np.random.default_rng(4)
    cable = make_cable("bent", SCENE_NCH)
    centre = np.array([38000.0, 23000.0, 0.0])
    cable = centre + (cable - centre) * [0.2, 0.2, 1.0]
    pos = np.array([E2E_SOURCE, (36500.0, 24800.0, -30.0)])
    t = kb.tau(cable, C0, SCENE_FS, pos)
    n = np.arange(SCENE_NS, dtype=np.float64)

    def tone(u):
        live = (u >= 0) & (u <= 199)
        return np.where(live, np.sin(2 * np.pi * u / 10.0) * 0.5 * (1 - np.cos(2 * np.pi * u / 199.0)), 0.0)
    jitter = rng.integers(-15, 16, SCENE_NCH)
    noise = rng.standard_normal((SCENE_NCH, SCENE_NS))
    clean = np.stack([tone(n - (800 + t[0, ch])) for ch in range(SCENE_NCH)])
    decoy = np.stack([10.0 * tone(n - (2500 + t[1, ch] + jitter[ch])) for ch in range(SCENE_NCH)])
    x = (clean + decoy + noise).astype(np.float32)
    out = dict(cable=cable, pos=pos, x=x, clean=clean.astype(np.float32), imag=analytic_imag(x), delays=kb.split(t))
    for a in (x, out["clean"], out["imag"]) + out["delays"]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def scene_reference():
    """The float64 restatement on the scene, once: `gate` = beam_coherence toward both positions over SCENE_NT samples from
    SCENE_STARTS with half window SCENE_H, order 3; `long` = toward position 0 over SCENE_LONG samples from 0 (the decoy lies in
    it, incoherent from there); `clean` = the normalized beam of the call alone over that stretch; and the orderings the tests
    assert of the hardware, shown here first."""
    sc = scene()
    k, f = sc["delays"]
    gate = kc.coherence_ref(sc["x"], (k, f), 3, np.array(SCENE_STARTS), SCENE_NT, SCENE_H, None, None, sc["imag"], None)
    one = (k[:1], f[:1])
    long = kc.coherence_ref(sc["x"], one, 3, np.array([0]), SCENE_LONG, 0, None, None, sc["imag"], None)
    alone = kc.coherence_ref(sc["clean"], one, 3, np.array([0]), SCENE_LONG, 0)
    assert long["wsum"].min() > 0 and np.array_equal(long["wsum"], alone["wsum"])
    clean = alone["beam"] / alone["wsum"]
    lin = long["beam"] / long["wsum"]
    pws = lin * long["phase"] ** 2
    # |d(lin phase^2)| <= dlin phase^2 + |lin| (2 phase dphase + dphase^2), and two roundings of the product and three of the square
    dlin = long["tol_beam"] / long["wsum"] + 2 * kc.U * np.abs(lin)
    dp = long["tol_phase"]
    tol_pws = dlin * long["phase"] ** 2 + np.abs(lin) * (2 * long["phase"] * dp + dp * dp) + 5 * kc.U * np.abs(pws)
    energy = (gate["beam"] ** 2).sum(axis=1)
    peaks = gate["semblance"].max(axis=1)
    assert energy[1] >= energy[0]                            # the decoy is the louder beam (428 662 against 151 095)
    assert peaks[0] - peaks[1] > 0.2                         # and the semblance separates them: 0.3097 against 0.0496
    err_lin, err_pws = ((lin - clean) ** 2).sum(), ((pws - clean) ** 2).sum()
    assert err_pws < 0.5 * err_lin                           # 19.7 against 83.7
    return dict(gate=gate, long=long, clean=clean, lin=lin, dlin=dlin, pws=pws, tol_pws=tol_pws, peaks=peaks, err_lin=err_lin, err_pws=err_pws)
