"""The cases of the delay-and-sum beam that tests/test_emu_beam.py (CPU emulator, C ABI) and tests/test_beam_gpu.py
(hardware, dw.loc.beamform) both run.  A runner is
    run(buf, ns, nxt, ns2, delays, order, weights, start, nt, normalize) -> beam float32 [ncalls x nt]
where buf is float32 [nch x pitch >= ns] and the block is buf[:, :ns] (pitch > ns: the rows are read in place), nxt is the
next block float32 [nch x pitch2 >= ns2] or None, delays is r int32 [ncalls x nch] for order 0 and (k int32, f float32)
otherwise, weights float32 [nch] or None, start int64 [ncalls].  T = d4w_beam_tile, S = the segment of d4w_beam_limits."""
import functools

import numpy as np

from tests import known_answers_beam as kb
from tests.known_answers_loc import C0, make_cable

NT_FORMS = ("1", "T-1", "T", "T+1", "2T+5")
NCH_FORMS = ("1", "2", "S-1", "S", "S+1", "2S+3")
NCALLS = (1, 3)
ORDERS = (0, 1, 3)
NORMALIZE = (False, True)
PITCHES = ("tight", "wide")
WEIGHTS = ("none", "zeros", "one")
STARTS = ("neg", "zero", "seam", "late")                     # "late": every channel runs off the end, all outputs are 0
DELAYS = ("near", "far")                                     # "far": delays larger than ns, start brought back by their median
NEXTS = ("none", "1", "3", "ns")
AXES = (NT_FORMS, NCH_FORMS, NCALLS, ORDERS, NORMALIZE, PITCHES, WEIGHTS, STARTS, DELAYS, NEXTS)
PAD = 5


def parity_cases():
    """40 tuples (nt form, nch form, ncalls, order, normalize, pitch, weights, start, delays, next, index): the largest corner
    first, then every value of every axis several times over (test_every_axis_value_occurs checks that)."""
    cases = [("2T+5", "2S+3", 1, 3, True, "wide", "zeros", "zero", "near", "ns", 0)]
    for i in range(1, 40):
        nchf = NCH_FORMS[(i + i // 6) % 6]
        ntf = NT_FORMS[i % 5]
        if nchf == "2S+3" and ntf == "2T+5":                 # the corner above has that pair; keep the rest quick
            ntf = "T+1"
        cases.append((ntf, nchf, NCALLS[(i // 2) % 2], ORDERS[i % 3], NORMALIZE[(i // 3) % 2], PITCHES[(i // 5) % 2], WEIGHTS[(i + i // 9) % 3],
                      STARTS[(i + i // 4) % 4], DELAYS[(i // 7) % 2], NEXTS[(i + i // 8) % 4], i))
    return cases


def case_id(c):
    return "nt%s-nch%s-c%d-o%d-n%d-%s-w%s-%s-%s-nb%s" % (c[0], c[1], c[2], c[3], int(c[4]), c[5], c[6], c[7], c[8], c[9])


def _dim(form, T, S):
    return {"1": 1, "2": 2, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+5": 2 * T + 5, "S-1": S - 1, "S": S, "S+1": S + 1, "2S+3": 2 * S + 3}[form]


def positions(cable, fs, ncalls, rot):
    """[ncalls x 3]: ON a channel (tau = 0 there: f = 0), and at (m + 0.004) and (m + 0.996) samples of travel east of channel 0
    (f < 0.01 and f > 0.99 there)."""
    forms = [cable[len(cable) // 2].copy(), cable[0] + [(37 + 0.004) * C0 / fs, 0.0, 0.0], cable[0] + [(12 + 0.996) * C0 / fs, 0.0, 0.0]]
    return np.stack([forms[(rot + q) % 3] for q in range(ncalls)])


def weight_set(kind, nch, rng):
    """None or float32 [nch] on a grid of 0.25 (their sums are exact in float32, as the tolerance with normalize supposes)."""
    if kind == "none":
        return None
    if kind == "one":
        w = np.zeros(nch, dtype=np.float32)
        w[nch // 2] = 1.25
        return w
    w = (rng.integers(1, 9, nch) / 4.0).astype(np.float32)
    w[rng.random(nch) < 0.3] = 0.0
    if nch > 1:
        w[0], w[-1] = 0.0, 1.5
    return w


def padded(x, wide, weights=None):
    """The block inside a buffer whose padding (pitch > ns) is NaN; the rows under weight 0 are NaN as well: they must leave no
    trace."""
    buf = np.full((x.shape[0], x.shape[1] + (PAD if wide else 0)), np.nan, dtype=np.float32)
    buf[:, :x.shape[1]] = x
    if weights is not None:
        buf[weights == 0] = np.nan
    return buf


def make_case(case, T, S):
    ntf, nchf, ncalls, order, normalize, pitch, wkind, skind, dkind, nkind, i = case
    nt, nch = _dim(ntf, T, S), _dim(nchf, T, S)
    ns = min(nt + 600, 3000)
    ns2 = {"none": 0, "1": 1, "3": 3, "ns": ns}[nkind]
    rng = np.random.default_rng(7000 + i)
    fs = 50.0 if dkind == "near" else 400.0
    cable = make_cable("bent" if i % 2 else "line", max(nch, 2))[:nch]
    t = kb.tau(cable, C0, fs, positions(cable, fs, ncalls, i))
    delays = kb.rounded(t) if order == 0 else kb.split(t)
    back = int(np.median(t)) if dkind == "far" else 0
    base = {"neg": -37, "zero": 0, "seam": ns - 200, "late": ns + ns2 + 5}[skind]
    start = (base - (back if skind != "late" else 0) + np.array([0, -5, 11])[:ncalls] * (skind != "late")).astype(np.int64)
    w = weight_set(wkind, nch, rng)
    x = rng.standard_normal((nch, ns)).astype(np.float32)
    nb = rng.standard_normal((nch, ns2)).astype(np.float32) if ns2 else None
    return x, nb, delays, order, w, start, nt, normalize, pitch == "wide"


@functools.lru_cache(maxsize=None)
def reference(case, T, S):
    """The case, its buffers and its float64 answer, computed once for every test that needs them (left unchanged by all)."""
    x, nb, delays, order, w, start, nt, normalize, wide = make_case(case, T, S)
    ref, tol, n, _ = kb.beam_ref(x, delays, order, start, nt, w, normalize, nb)
    buf, nbuf = padded(x, wide, w), (padded(nb, wide, w) if nb is not None else None)
    for a in (buf, nbuf, w, start, ref, tol, n) + (delays if isinstance(delays, tuple) else (delays,)):
        if a is not None:
            a.setflags(write=False)
    return buf, x.shape[1], nbuf, (nb.shape[1] if nb is not None else 0), delays, order, w, start, nt, normalize, ref, tol, n


def check_parity(run, case, T, S):
    """Runs the case and returns the worst error / tolerance."""
    buf, ns, nbuf, ns2, delays, order, w, start, nt, normalize, ref, tol, n = reference(case, T, S)
    got = run(buf, ns, nbuf, ns2, delays, order, w, start, nt, normalize)
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert np.all(np.isfinite(got))                          # no padding, no row under weight 0 was read
    worst = kb.worst_ratio(got, ref, tol)
    print("%s: worst error / tolerance = %.3g, contributors %d .. %d" % (case_id(case), worst, n.min(), n.max()))
    assert worst <= 1.0, worst
    if case[7] == "late":
        assert n.max() == 0 and not got.any()
    if w is not None and not w.any():
        assert not got.any()
    return worst


# ---- the delay table ---------------------------------------------------------------------------------------------------------
def delay_scenes():
    """(cable, fs, pos): a few channels up to more than a workgroup of them, one call and several, every position form."""
    out = []
    for kind, nch, fs, ncalls in (("line", 1, 50.0, 1), ("bent", 5, 50.0, 3), ("bent", 67, 200.0, 3), ("line", 400, 200.0, 7)):
        cable = make_cable(kind, max(nch, 2))[:nch]
        out.append((cable, fs, positions(cable, fs, ncalls, 0)))
    return out


def check_delays(delays_fn):
    """delays_fn(cable, c0, fs, pos, rounded) -> (k, f) or r, as NumPy arrays."""
    seen = np.zeros(3, dtype=bool)
    for cable, fs, pos in delay_scenes():
        t = kb.tau(cable, C0, fs, pos)
        k, f = delays_fn(cable, C0, fs, pos, False)
        assert k.dtype == np.int32 and f.dtype == np.float32 and k.shape == t.shape and f.shape == t.shape
        assert np.all(f >= 0) and np.all(f < np.float32(1.0))
        assert np.all(np.abs((k.astype(np.float64) + f.astype(np.float64)) - t) <= 2.0 ** -24 + 4 * 2.0 ** -52 * t)
        r = delays_fn(cable, C0, fs, pos, True)
        assert r.dtype == np.int32 and r.shape == t.shape
        q = t + 0.5
        sure = np.abs(q - np.round(q)) > 1e-9                # away from a tie the rounded delay is beyond doubt
        assert sure.mean() > 0.9 and np.array_equal(r[sure], np.floor(q[sure]).astype(np.int32))
        assert np.all(np.abs(r - q + 0.5) <= 0.5 + 1e-9)
        seen |= [bool((f == 0).any()), bool(((f > 0) & (f < 0.01)).any()), bool((f > 0.99).any())]
    assert seen.all(), seen                                  # f = 0, f < 0.01 and f > 0.99 all occur in the tables


# ---- exact known answers -----------------------------------------------------------------------------------------------------
def _scene(nch, ncalls, ns, fs=50.0, seed=11):
    rng = np.random.default_rng(seed + nch)
    cable = make_cable("bent", max(nch, 2))[:nch]
    t = kb.tau(cable, C0, fs, positions(cable, fs, ncalls, 1))
    return rng, t, rng.standard_normal((nch, ns)).astype(np.float32)


def check_ones(run, S):
    """Ones at start + r[ch]: the beam at j = 0 is exactly nch, and exactly 1 with normalize."""
    for nch in (5, S + 3):
        _, t, _ = _scene(nch, 2, 8)
        r = kb.rounded(t)
        ns = int(r.max()) + 40
        start = np.array([3, 17], dtype=np.int64)
        for c in range(2):
            x = np.zeros((nch, ns), dtype=np.float32)
            x[np.arange(nch), start[c] + r[c]] = 1.0
            for normalize, want in ((False, float(nch)), (True, 1.0)):
                got = run(x, ns, None, 0, r, 0, None, start, 4, normalize)
                assert got[c, 0] == np.float32(want), (nch, c, normalize, got[c, 0])


def check_ramp(run, T, S):
    """x[ch, n] = n: both interpolators reproduce a straight line, beam = sum over the contributors of (n + tau_ch)."""
    nch, ns, nt = S + 2, T + 700, T + 9
    _, t, _ = _scene(nch, 2, 8)
    x = np.broadcast_to(np.arange(ns, dtype=np.float32), (nch, ns)).copy()
    start = np.array([-3, 40], dtype=np.int64)
    for order in (1, 3):
        k, f = kb.split(t)
        ref, tol, n, _ = kb.beam_ref(x, (k, f), order, start, nt, None, False, None)
        n0 = start[:, None] + np.arange(nt)[None, :]
        lo, hi = (-1, 2) if order == 3 else (0, 1)
        want = np.zeros_like(ref)
        for ch in range(nch):
            q = n0 + k[:, ch:ch + 1]
            ok = (q + lo >= 0) & (q + hi < ns)
            want += np.where(ok, q + f[:, ch:ch + 1].astype(np.float64), 0.0)
        assert n.max() == nch and np.all(np.abs(want - ref) <= 1e-9 * (1 + np.abs(want)))
        got = run(x, ns, None, 0, (k, f), order, None, start, nt, False)
        assert np.all(np.abs(got - want) <= tol + 1e-9 * np.abs(want))


def check_zeros(run, T, S):
    nch, ns = S + 1, T + 40
    _, t, _ = _scene(nch, 1, 8)
    x = np.zeros((nch, ns), dtype=np.float32)
    for order in ORDERS:
        d = kb.rounded(t) if order == 0 else kb.split(t)
        for normalize in NORMALIZE:
            got = run(x, ns, None, 0, d, order, None, np.zeros(1, dtype=np.int64), ns, normalize)
            assert got.shape == (1, ns) and not got.any()


def check_nan_rows(run, T, S):
    """A NaN row under weight 0 changes nothing; a NaN under a non-zero weight propagates into what it reaches."""
    nch, ns, nt = S + 1, T + 300, T + 1
    rng, t, x = _scene(nch, 1, T + 300)
    w = weight_set("zeros", nch, rng)
    start = np.zeros(1, dtype=np.int64)
    for order in ORDERS:
        d = kb.rounded(t) if order == 0 else kb.split(t)
        clean = run(x, ns, None, 0, d, order, w, start, nt, False)
        dirty = x.copy()
        dirty[w == 0] = np.nan
        assert np.array_equal(clean, run(dirty, ns, None, 0, d, order, w, start, nt, False)) and np.all(np.isfinite(clean))
        ch = int(np.flatnonzero(w != 0)[1])
        k = int((d if order == 0 else d[0])[0, ch])
        at = k + 20                                          # reached from column 20 (and from its neighbours by the taps)
        dirty = x.copy()
        dirty[ch, at] = np.nan
        got = run(dirty, ns, None, 0, d, order, w, start, nt, False)
        lo, hi = {0: (0, 0), 1: (0, 1), 3: (-1, 2)}[order]
        hit = np.zeros(nt, dtype=bool)
        hit[20 - hi:20 - lo + 1] = True
        assert np.array_equal(np.isnan(got[0]), hit)


def check_bit_identity(run, T, S):
    """Bit for bit: a repeated call; the input scaled by 2^-3 and 2^5; a call alone against the same call as row 1 of three."""
    nch, ns, nt = 2 * S + 3, T + 300, T + 1
    rng, t, x = _scene(nch, 3, T + 300)
    w = weight_set("zeros", nch, rng)
    start = np.array([5, -20, 300], dtype=np.int64)
    for order in ORDERS:
        d = kb.rounded(t) if order == 0 else kb.split(t)
        for normalize in NORMALIZE:
            first = run(x, ns, None, 0, d, order, w, start, nt, normalize)
            assert first.any() and np.array_equal(first, run(x, ns, None, 0, d, order, w, start, nt, normalize))
            for p in (-3, 5):
                scaled = run(x * np.float32(2.0 ** p), ns, None, 0, d, order, w, start, nt, normalize)
                assert np.array_equal(scaled, first * np.float32(2.0 ** p))
            one = tuple(a[1:2] for a in d) if order else d[1:2]
            alone = run(x, ns, None, 0, one, order, w, start[1:2], nt, normalize)
            assert np.array_equal(alone[0], first[1])


def check_next_block(run, T, S):
    """beamform(trace, next_block=b) equals beamform(concatenate([trace, b])) bit for bit, whatever the pitch of either."""
    nch, ns, nt = S + 1, T + 100, 2 * T + 5
    rng, t, x = _scene(nch, 2, T + 100)
    start = np.array([0, ns - 300], dtype=np.int64)
    w = weight_set("zeros", nch, rng)
    for ns2 in (1, 3, ns):
        nb = rng.standard_normal((nch, ns2)).astype(np.float32)
        whole = np.concatenate([x, nb], axis=1)
        for order in ORDERS:
            d = kb.rounded(t) if order == 0 else kb.split(t)
            for normalize in NORMALIZE:
                a = run(padded(x, True), ns, padded(nb, True), ns2, d, order, w, start, nt, normalize)
                b = run(whole, ns + ns2, None, 0, d, order, w, start, nt, normalize)
                assert np.array_equal(a, b) and np.all(np.isfinite(a))
                if ns2 == ns and not normalize:
                    alone = run(x, ns, None, 0, d, order, w, start, nt, normalize)
                    assert not np.array_equal(a, alone)      # without the next block the far channels drop out


def stack_scene(nch, kind="bent"):
    """A 3 x 2 grid and an envelope block for the comparison with stack_grid: (cable, fs, xs, ys, z, env, weights, k_range)."""
    rng = np.random.default_rng(300 + nch)
    cable = make_cable(kind, max(nch, 2))[:nch]
    xs, ys, z = np.array([33000.0, 36500.0, 41000.0]), np.array([20000.0, 25500.0]), -40.0
    env = np.abs(rng.standard_normal((nch, 1500))).astype(np.float32)
    return cable, 50.0, xs, ys, z, env, weight_set("zeros", nch, rng), (-300, 900)


def stack_nodes(xs, ys, z):
    return np.array([[x, y, z] for y in ys for x in xs])


def check_against_stack(run, stack, r, nch, S):
    """stack: the [ny x nx x nt] float32 result of stack_grid for stack_scene(nch) (normalize off); r: the rounded beam delays
    at stack_nodes.  Order 0 toward the nodes: the same bits for nch <= S; within the tolerance beyond S and with normalize."""
    cable, fs, xs, ys, z, env, w, (k0, k1) = stack_scene(nch)
    pos = stack_nodes(xs, ys, z)
    start = np.full(len(pos), k0, dtype=np.int64)
    got = run(env, env.shape[1], None, 0, r, 0, w, start, k1 - k0, False)
    rows = stack.reshape(len(pos), k1 - k0)
    if nch <= S:
        assert np.array_equal(got, rows)
    ref, tol, _, _ = kb.beam_ref(env, r, 0, start, k1 - k0, w, False, None)
    assert kb.worst_ratio(got, ref, tol) <= 1.0 and kb.worst_ratio(rows, ref, tol) <= 1.0
    ref, tol, _, _ = kb.beam_ref(env, r, 0, start, k1 - k0, w, True, None)
    assert kb.worst_ratio(run(env, env.shape[1], None, 0, r, 0, w, start, k1 - k0, True), ref, tol) <= 1.0
    return r


# ---- the end-to-end scene ----------------------------------------------------------------------------------------------------
E2E_FS, E2E_NS, E2E_NCH, E2E_SEED, E2E_AMP = 200.0, 2400, 64, 20, 1.0
E2E_SOURCE, E2E_T0 = (38950.0, 23620.0, -30.0), 2.5125       # between the nodes of the grid; emitted at sample 502.5


def tone_burst(fs=E2E_FS):
    """One second of a 20 Hz tone under a Hann window, float64."""
    n = np.arange(int(fs))
    return np.sin(2 * np.pi * 20.0 * n / fs) * np.hanning(len(n))


def e2e_scene():
    """A 64-channel bent cable of 3 km radius, a 9 x 9 grid of 500 m around it, and a block of unit-variance noise with the
    burst planted at the exact (fractional) moveout of E2E_SOURCE: dict(cable, xs, ys, z, x float32, burst, tau)."""
    rng = np.random.default_rng(E2E_SEED)
    cable = make_cable("bent", E2E_NCH)
    centre = np.array([38000.0, 23000.0, 0.0])
    cable = centre + (cable - centre) * [0.2, 0.2, 1.0]
    xs, ys, z = 38000.0 + 500.0 * (np.arange(9) - 4), 23000.0 + 500.0 * (np.arange(9) - 4), -30.0
    t = kb.tau(cable, C0, E2E_FS, E2E_SOURCE)[0] + E2E_T0 * E2E_FS                 # arrival in samples, fractional
    n = np.arange(E2E_NS, dtype=np.float64)
    x = rng.standard_normal((E2E_NCH, E2E_NS))
    for ch in range(E2E_NCH):
        u = n - t[ch]
        live = (u >= 0) & (u <= E2E_FS - 1)
        x[ch, live] += E2E_AMP * np.sin(2 * np.pi * 20.0 * u[live] / E2E_FS) * 0.5 * (1 - np.cos(2 * np.pi * u[live] / (E2E_FS - 1)))
    return dict(cable=cable, xs=xs, ys=ys, z=z, x=x.astype(np.float32), burst=tone_burst(), tau=t)


def matched_envelope(x, burst):
    """The envelope of every row's cross-correlation with the burst, aligned so that sample i answers a burst starting at i."""
    from scipy import signal
    c = signal.fftconvolve(np.asarray(x, dtype=np.float64), burst[None, ::-1], mode="full", axes=1)[:, len(burst) - 1:]
    return np.abs(signal.hilbert(c, axis=1)).astype(np.float32)


def best_correlation(trace, burst, centre, search=6):
    """The largest Pearson correlation coefficient of the burst with a window of the trace that starts within `search` samples
    of `centre`, float64."""
    trace, best = np.asarray(trace, dtype=np.float64), -1.0
    for s in range(int(centre) - search, int(centre) + search + 1):
        if s < 0 or s + len(burst) > len(trace):
            continue
        best = max(best, float(np.corrcoef(trace[s:s + len(burst)], burst)[0, 1]))
    return best
