"""The cases of the transpose of the beam that tests/test_emu_project.py (CPU emulator, C ABI) and tests/test_project_gpu.py
(hardware, dw.loc.project_calls / subtract_calls) both run.  A runner has three methods:
    fit(buf, ns, nxt, ns2, delays, order, beam, start, weights) -> (amp, coef), float32 [ncalls x nch]
    sub(buf, ns, nxt, ns2, delays, order, beam, start, amp, inplace) -> the residual record float32 [nch x (ns + ns2)]
    beam(buf, ns, nxt, ns2, delays, order, start, nt) -> float32 [ncalls x nt], the plain beam (weights 1, no normalize)
where buf is float32 [nch x pitch >= ns] and the block is buf[:, :ns] (pitch > ns: the rows are used in place), nxt is the next
block float32 [nch x pitch2 >= ns2] or None, delays is r int32 [ncalls x nch] for order 0 and (k int32, f float32) otherwise,
beam float32 [ncalls x L], start int64 [ncalls], weights float32 [nch] or None, amp float32 [ncalls x nch].  sub leaves buf and nxt
as they are (in place it works on a copy) and checks the guard words and the padding around what it writes.  W = the channels
per workgroup of d4w_project_limits.

The parity cases give the delay table directly (a base delay plus a small per-channel pattern, and fractions that are 0, next
to 1 or anywhere), so that which supports fall off the record is decided by the case and not by a geometry."""
import functools

import numpy as np

from tests import known_answers_beam as kb
from tests import known_answers_project as kp
from tests.beam_cases import padded, weight_set

LENGTHS = (1, 2, 63, 64, 65, 129, 200)
ORDERS = (0, 1, 3)
FRACTIONS = ("zero", "one", "any")                           # f = 0, f in [0.99, 1), f anywhere
NCH_FORMS = ("1", "W-1", "W", "W+1", "2W+3")
NCALLS = (1, 3)
PITCHES = ("tight", "wide")
WEIGHTS = ("none", "zeros", "one")
STARTS = ("neg", "mid", "seam", "late")                      # "late": every support lies past the end, everything is NaN
NEXTS = ("none", "1", "3", "ns")
AXES = (LENGTHS, ORDERS, FRACTIONS, NCH_FORMS, NCALLS, PITCHES, WEIGHTS, STARTS, NEXTS)
NS = 700
BASE = 40


def parity_cases():
    """36 tuples (L, order, fractions, nch form, ncalls, pitch, weights, start, next, index): the largest corner first, then
    every value of every axis several times over (test_every_axis_value_occurs checks that)."""
    cases = [(200, 3, "any", "2W+3", 3, "wide", "zeros", "seam", "ns", 0)]
    for i in range(1, 36):
        cases.append((LENGTHS[i % 7], ORDERS[(i + i // 7) % 3], FRACTIONS[(i + i // 3) % 3], NCH_FORMS[(i + i // 5) % 5], NCALLS[(i // 2) % 2],
                      PITCHES[(i // 5) % 2], WEIGHTS[(i + i // 9) % 3], STARTS[(i + i // 4) % 4], NEXTS[(i + i // 8) % 4], i))
    return cases


def case_id(c):
    return "L%d-o%d-f%s-nch%s-c%d-%s-w%s-%s-nb%s" % c[:9]


def _nch(form, W):
    return max(1, {"1": 1, "W-1": W - 1, "W": W, "W+1": W + 1, "2W+3": 2 * W + 3}[form])


def fractions(kind, shape, rng):
    if kind == "zero":
        return np.zeros(shape, dtype=np.float32)
    if kind == "one":
        return (0.99 + 0.0099 * rng.random(shape)).astype(np.float32)
    f = rng.random(shape).astype(np.float32)
    f.flat[0] = 0.0
    f.flat[-1] = np.float32(1.0) - np.float32(2.0 ** -24)     # the largest fraction there is
    return f


def table(order, nch, ncalls, fkind, rng, base=BASE):
    """r, or (k, f): base + 0 .. 10 over the channels, the calls 3 apart."""
    k = (base + (7 * np.arange(nch)[None, :] + 3 * np.arange(ncalls)[:, None]) % 11).astype(np.int32)
    return k if order == 0 else (k, fractions(fkind, k.shape, rng))


def make_case(case, W):
    L, order, fkind, nchf, ncalls, pitch, wkind, skind, nkind, i = case
    nch, ns, Wn = _nch(nchf, W), NS, L + order
    ns2 = {"none": 0, "1": 1, "3": 3, "ns": ns}[nkind]
    rng = np.random.default_rng(13000 + i)
    delays = table(order, nch, ncalls, fkind, rng)
    # lo = s + 0 .. 10 (+ kLo) over the channels.  "neg": the supports begin within 5 samples either side of the record's
    # first; "seam": they end within 5 samples either side of the end of the block; the calls lie 0, -2 and 3 samples apart, so
    # that their supports overlap on every channel
    s = {"neg": -5, "mid": 300, "seam": ns - Wn - 5, "late": ns + ns2 + 5}[skind]
    start = (s - BASE + np.array([0, -2, 3])[:ncalls] * (skind != "late")).astype(np.int64)
    w = weight_set(wkind, nch, rng)
    x = rng.standard_normal((nch, ns)).astype(np.float32)
    nb = rng.standard_normal((nch, ns2)).astype(np.float32) if ns2 else None
    beam = rng.standard_normal((ncalls, L)).astype(np.float32)
    return x, nb, delays, order, beam, start, w, pitch == "wide"


@functools.lru_cache(maxsize=None)
def reference(case, W):
    """The case, its buffers and its float64 answers, computed once for every test that needs them (left unchanged by all):
    the fit, and the subtraction of float32(the fit's amp) with one entry set to 0 (a call that is not to be subtracted)."""
    x, nb, delays, order, beam, start, w, wide = make_case(case, W)
    fit = kp.fit_ref(x, delays, order, start, beam, w, nb)
    amp = fit.amp.astype(np.float32)
    if fit.valid.sum() >= 2:
        amp[tuple(np.argwhere(fit.valid)[-1])] = 0.0
    y, tol, reached = kp.subtract_ref(x, delays, order, start, beam, amp, nb)
    buf, nbuf = padded(x, wide, w), (padded(nb, wide, w) if nb is not None else None)
    for a in (buf, nbuf, start, w, beam, amp, y, tol, reached) + (delays if isinstance(delays, tuple) else (delays,)):
        if a is not None:
            a.setflags(write=False)
    return SimpleCase(buf=buf, ns=x.shape[1], nbuf=nbuf, ns2=(nb.shape[1] if nb is not None else 0), delays=delays, order=order, beam=beam,
                      start=start, w=w, fit=fit, amp=amp, y=y, tol=tol, reached=reached)


class SimpleCase:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def record(self, buf=None, nbuf=None):
        """The record the buffers hold, float32 [nch x (ns + ns2)] (the padding left out)."""
        buf, nbuf = self.buf if buf is None else buf, self.nbuf if nbuf is None else nbuf
        return buf[:, :self.ns] if nbuf is None else np.concatenate([buf[:, :self.ns], nbuf[:, :self.ns2]], axis=1)


def check_fit_outputs(got, shape):
    assert len(got) == 2
    for a in got:
        assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == tuple(shape), (a.dtype, a.shape)


def check_parity(run, case, W):
    """Runs the case: the fit, the subtraction out of place and in place.  Returns the worst error / tolerance of (the fit,
    the subtraction)."""
    k = reference(case, W)
    got = run.fit(k.buf, k.ns, k.nbuf, k.ns2, k.delays, k.order, k.beam, k.start, k.w)
    check_fit_outputs(got, k.fit.amp.shape)
    wf = kp.worst_fit(got, k.fit)
    dead = np.zeros(k.buf.shape[0], dtype=bool) if k.w is None else k.w == 0
    assert all(np.all(np.isnan(a[:, dead])) for a in got)
    if case[7] == "late":
        assert not k.fit.valid.any() and all(np.all(np.isnan(a)) for a in got)
    if case[7] == "mid":
        assert k.fit.valid[:, ~dead].all() and not np.isnan(got[0][:, ~dead]).any() and not np.isnan(got[1][:, ~dead]).any()
    out = run.sub(k.buf, k.ns, k.nbuf, k.ns2, k.delays, k.order, k.beam, k.start, k.amp, False)
    ws = kp.worst_subtract(out, k.y, k.tol, k.reached, k.record())
    inp = run.sub(k.buf, k.ns, k.nbuf, k.ns2, k.delays, k.order, k.beam, k.start, k.amp, True)
    assert kp.same(out, inp)                                 # in place and out of place: the same bits
    print("%s: worst error / tolerance: fit %.3g, subtraction %.3g; %d of %d windows valid, %d samples reached"
          % (case_id(case), wf, ws, k.fit.valid.sum(), k.fit.valid.size, k.reached.sum()))
    assert wf <= 1.0 and ws <= 1.0, (wf, ws)
    return wf, ws


def owned(k):
    """bool [nch x ntot]: the samples inside a valid support of a live channel."""
    own = np.zeros(k.y.shape, dtype=bool)
    for c, ch in zip(*np.nonzero(k.fit.valid)):
        own[ch, k.fit.lo[c, ch]:k.fit.lo[c, ch] + k.fit.W] = True
    return own


def check_poison(run, case, W):
    """Every sample outside the union of the valid supports set to NaN: the fit keeps its bits (no load touches what it does
    not own), the subtraction out of place copies the poison and keeps its bits inside the supports, in place it leaves it."""
    k = reference(case, W)
    own = owned(k)
    pb = k.buf.copy()
    pb[:, :k.ns][~own[:, :k.ns]] = np.nan
    pn = None
    if k.nbuf is not None:
        pn = k.nbuf.copy()
        pn[:, :k.ns2][~own[:, k.ns:]] = np.nan
    clean = run.fit(k.buf, k.ns, k.nbuf, k.ns2, k.delays, k.order, k.beam, k.start, k.w)
    dirty = run.fit(pb, k.ns, pn, k.ns2, k.delays, k.order, k.beam, k.start, k.w)
    assert all(kp.same(a, b) for a, b in zip(clean, dirty))
    ref = run.sub(k.buf, k.ns, k.nbuf, k.ns2, k.delays, k.order, k.beam, k.start, k.amp, False)
    for inplace in (False, True):
        got = run.sub(pb, k.ns, pn, k.ns2, k.delays, k.order, k.beam, k.start, k.amp, inplace)
        assert np.all(np.isnan(got[~own])) and kp.same(got[own], ref[own]), inplace
    assert not (k.reached & ~own).any()
    return int(own.sum())


# ---- exact known answers -----------------------------------------------------------------------------------------------------
def _scene(nch, ncalls, order, ns=600, seed=5, fkind="any"):
    """A table, starts and a block: the supports begin at 200 + 40 .. 50 (+ 20 per call) and lengths up to 203 fit."""
    rng = np.random.default_rng(seed + nch + order)
    delays = table(order, nch, ncalls, fkind, rng)
    start = (200 + 20 * np.arange(ncalls)).astype(np.int64)
    return rng, delays, start, rng.standard_normal((nch, ns)).astype(np.float32)


def check_identical_channels(run, W):
    """The same small-integer waveform on every channel along integer delays, order 0, and its normalized beam (the waveform
    itself, exactly): every sum is an integer below 2^24, so num = den and amp = 1 exactly, coef = 1 within
    2 (2^-24 + 2^-25) (den xx = den^2 rounded, its root, the division) and the residual is exactly 0 under the supports."""
    for L in (1, 64, 200):
        nch, ns = 2 * W + 3, 600
        rng, r, start, _ = _scene(nch, 1, 0, ns)
        wave = rng.integers(-15, 16, L).astype(np.float32)
        wave[0] = 7.0
        x = np.zeros((nch, ns), dtype=np.float32)
        lo = kp.support_lo(start, r.astype(np.int64), 0)
        for ch in range(nch):
            x[ch, lo[0, ch]:lo[0, ch] + L] = wave
        beam = run.beam(x, ns, None, 0, r, 0, start, L) / np.float32(nch)
        assert kp.same(beam[0], wave)
        amp, coef = run.fit(x, ns, None, 0, r, 0, beam, start, None)
        assert kp.same(amp, np.ones((1, nch), dtype=np.float32))
        assert np.all(np.abs(coef.astype(np.float64) - 1.0) <= 3 * kp.U), np.abs(coef - 1).max()
        for inplace in (False, True):
            y = run.sub(x, ns, None, 0, r, 0, beam, start, amp, inplace)
            assert not y.any()


def check_power_of_two(run, W):
    """A channel scaled by 2^k: amp scales by 2^k exactly, coef keeps its bits."""
    for order, L in ((0, 65), (1, 200), (3, 63)):
        nch = W + 1
        rng, delays, start, x = _scene(nch, 2, order)
        beam = rng.standard_normal((2, L)).astype(np.float32)
        first = run.fit(x, 600, None, 0, delays, order, beam, start, None)
        assert all(np.isfinite(a).all() for a in first)
        scale = (2.0 ** np.array([-3, 5, 0, 1, -7, 2, 9, -1, 4, -2, 3])[np.arange(nch) % 11]).astype(np.float32)
        got = run.fit(x * scale[:, None], 600, None, 0, delays, order, beam, start, None)
        assert kp.same(got[0], first[0] * scale[None, :]) and kp.same(got[1], first[1])


def check_zero_beam(run, W):
    """A zero beam: amp = coef = 0, and y = x bit for bit whatever amp says (the NaN padding of a row included); a NaN sample
    under a zero beam still gives NaN."""
    for order in ORDERS:
        nch = W + 1
        rng, delays, start, x = _scene(nch, 2, order)
        x[0, 300] = np.nan
        beam = np.zeros((2, 65), dtype=np.float32)
        amp, coef = run.fit(x, 600, None, 0, delays, order, beam, start, None)
        assert np.all(np.isnan(amp[:, 0])) and np.all(np.isnan(coef[:, 0])) and not amp[:, 1:].any() and not coef[:, 1:].any()
        assert not np.isnan(amp[:, 1:]).any() and not np.isnan(coef[:, 1:]).any()
        for inplace in (False, True):
            assert kp.same(run.sub(x, 600, None, 0, delays, order, beam, start, amp, inplace), x)
            assert kp.same(run.sub(x, 600, None, 0, delays, order, beam, start, np.full_like(amp, 3.0), inplace), x)


def check_nan_samples(run, W):
    """A NaN just outside a support changes nothing; inside, it makes that (call, channel) NaN and leaves the others' bits;
    a NaN row under weight 0 changes nothing; a NaN or zero amp subtracts nothing."""
    order, L, nch = 3, 65, W + 1
    rng, delays, start, x = _scene(nch, 1, order)
    beam = rng.standard_normal((1, L)).astype(np.float32)
    w = weight_set("zeros", nch, rng)
    clean = run.fit(x, 600, None, 0, delays, order, beam, start, w)
    assert np.isfinite(clean[0][:, w != 0]).all() and np.isnan(clean[0][:, w == 0]).all()
    dirty = x.copy()
    dirty[w == 0] = np.nan
    assert all(kp.same(a, b) for a, b in zip(clean, run.fit(dirty, 600, None, 0, delays, order, beam, start, w)))
    ch = nch - 1
    lo = int(kp.support_lo(start, delays[0].astype(np.int64), order)[0, ch])
    keep = np.arange(nch) != ch
    for at, inside in ((lo - 1, False), (lo + L + order, False), (lo, True), (lo + L // 2, True), (lo + L + order - 1, True)):
        d = x.copy()
        d[ch, at] = np.nan
        got = run.fit(d, 600, None, 0, delays, order, beam, start, w)
        assert all(kp.same(a[:, keep], b[:, keep]) for a, b in zip(got, clean)), at
        assert all(np.isnan(a[0, ch]) if inside else kp.same(a[0, ch], b[0, ch]) for a, b in zip(got, clean)), at
    amp = clean[0].copy()
    amp[0, ch] = 0.0
    y = run.sub(x, 600, None, 0, delays, order, beam, start, amp, False)
    assert kp.same(y[ch], x[ch]) and kp.same(y[w == 0], x[w == 0]) and not kp.same(y, x)
    amp[0, :] = np.inf
    assert kp.same(run.sub(x, 600, None, 0, delays, order, beam, start, amp, True), x)


def check_batch_and_split(run, W):
    """Bit for bit: a repeated call; one call alone against the same call as row 1 of three (the fit), and against the batch
    with the other rows' amp set to NaN (the subtraction); wide pitch against tight; the record split anywhere into
    trace + next_block, whatever the pitches."""
    for order, L in ((0, 129), (1, 63), (3, 200)):
        nch = 2 * W + 3
        rng, delays, start, x = _scene(nch, 3, order)
        ns = x.shape[1]
        beam = rng.standard_normal((3, L)).astype(np.float32)
        w = weight_set("zeros", nch, rng)
        first = run.fit(x, ns, None, 0, delays, order, beam, start, w)
        assert all(np.isfinite(a[:, w != 0]).all() for a in first)
        assert all(kp.same(a, b) for a, b in zip(first, run.fit(x, ns, None, 0, delays, order, beam, start, w)))
        one = delays[1:2] if order == 0 else (delays[0][1:2], delays[1][1:2])
        alone = run.fit(x, ns, None, 0, one, order, beam[1:2], start[1:2], w)
        assert all(kp.same(a[0], b[1]) for a, b in zip(alone, first))
        assert all(kp.same(a, b) for a, b in zip(first, run.fit(padded(x, True, w), ns, None, 0, delays, order, beam, start, w)))
        amp = np.where(np.isnan(first[0]), np.float32(0.5), first[0])          # the dead channels are subtracted from as well
        whole = run.sub(x, ns, None, 0, delays, order, beam, start, amp, False)
        assert kp.same(whole, run.sub(x, ns, None, 0, delays, order, beam, start, amp, False))
        only = np.full_like(amp, np.nan)
        only[1] = amp[1]
        assert kp.same(run.sub(x, ns, None, 0, delays, order, beam, start, only, False),
                       run.sub(x, ns, None, 0, one, order, beam[1:2], start[1:2], amp[1:2], True))
        lo = int(kp.support_lo(start, (delays if order == 0 else delays[0]).astype(np.int64), order)[0, 0])
        for i, k in enumerate((lo, lo + 1, lo + (L + order) // 2, lo + L + order - 1, lo + L + order, 1, ns - 1)):
            a, b = np.ascontiguousarray(x[:, :k]), np.ascontiguousarray(x[:, k:])
            pa, pb = padded(a, i % 2 == 0), padded(b, i % 2 == 1)
            assert all(kp.same(p, q) for p, q in zip(first, run.fit(padded(a, i % 2 == 0, w), k, padded(b, i % 2 == 1, w), ns - k, delays, order,
                                                                     beam, start, w))), k
            for inplace in (False, True):
                assert kp.same(whole, run.sub(pa, k, pb, ns - k, delays, order, beam, start, amp, inplace)), (k, inplace)


def check_call_order(run, W):
    """The calls are subtracted in increasing order.  x = 1 under two overlapping order-0 supports, call P with amp 2^-25 and
    call Q with amp 1/2, both beams 1: (P, Q) gives float32(1 - 2^-25) = 1 (the tie goes to the even neighbour), then 1/2;
    (Q, P) gives 1/2, then 1/2 - 2^-25, which float32 holds.  Every product and sum is exact in float64, so the step-by-step
    restatement has the device's bits for both orders, and they differ."""
    nch, ns, L = W + 1, 300, 70
    r = np.array([[10 + ch for ch in range(nch)], [14 + ch for ch in range(nch)]], dtype=np.int32)
    start = np.array([50, 50], dtype=np.int64)
    x = np.ones((nch, ns), dtype=np.float32)
    beam = np.ones((2, L), dtype=np.float32)
    amp = np.array([[2.0 ** -25] * nch, [0.5] * nch], dtype=np.float32)
    pq = run.sub(x, ns, None, 0, r, 0, beam, start, amp, False)
    qp = run.sub(x, ns, None, 0, r[::-1].copy(), 0, beam, start, amp[::-1].copy(), False)
    assert kp.same(pq, kp.subtract_steps_f32(x, r, 0, start, beam, amp))
    assert kp.same(qp, kp.subtract_steps_f32(x, r[::-1], 0, start, beam, amp[::-1]))
    both = slice(50 + 14, 50 + 10 + L)                       # channel 0: where the two supports overlap
    assert np.all(pq[0, both] == 0.5) and np.all(qp[0, both] == np.float32(0.5 - 2.0 ** -25))
    assert kp.same(run.sub(x, ns, None, 0, r, 0, beam, start, amp, True), pq)


def check_transpose(run, W):
    """The dot-product test that ties project.hip to beam.hip: sum_ch num[c, ch] = sum_j beam(x)[c, j] b[c, j] for calls whose
    windows are all valid.  The restatement holds it to float64 rounding; on the device num is amp x den (den from the
    restatement), within sum_ch tol_amp den, and the beam within known_answers_beam's tolerance: the two sides differ by at
    most sum_ch tol_amp den + sum_j tol_beam |b|.  Returns the worst difference / bound."""
    worst = 0.0
    for order, L in ((0, 64), (1, 129), (3, 200)):
        nch = 2 * W + 3
        rng, delays, start, x = _scene(nch, 3, order)
        ns = x.shape[1]
        b = rng.standard_normal((3, L)).astype(np.float32)
        fit = kp.fit_ref(x, delays, order, start, b)
        assert fit.valid.all()
        bref, btol, n, _ = kb.beam_ref(x, delays, order, start, L)
        assert n.min() == nch
        left, right = fit.num.sum(1), (bref * b.astype(np.float64)).sum(1)
        scale = (np.abs(bref) * np.abs(b)).sum(1)
        assert np.all(np.abs(left - right) <= 1e-12 * scale), (left, right)
        amp, _ = run.fit(x, ns, None, 0, delays, order, b, start, None)
        bdev = run.beam(x, ns, None, 0, delays, order, start, L)
        dl = (amp.astype(np.float64) * fit.den).sum(1)
        dr = (bdev.astype(np.float64) * b.astype(np.float64)).sum(1)
        bound = (fit.tol_amp * fit.den).sum(1) + (btol * np.abs(b)).sum(1) + 1e-12 * scale
        ratio = float((np.abs(dl - dr) / bound).max())
        print("order %d: |sum_ch num - <beam, b>| / bound = %.3g" % (order, ratio))
        assert ratio <= 1.0, (order, dl, dr, bound)
        worst = max(worst, ratio)
    return worst


def check_tiles(run, W):
    """A record of several subtraction tiles (2048 samples each) and a beam of more than one LDS piece of the fit (1024
    terms): supports across the tile borders at 4096 and 8192 and across the seam, two of them overlapping around 8192, and
    long stretches that no call reaches.  The fit and both subtractions against the restatement."""
    worst = 0.0
    for order, L in ((1, 1500), (3, 129), (0, 1024)):
        nch, ns, ns2 = W + 1, 12500, 700
        rng = np.random.default_rng(31 + order)
        delays = table(order, nch, 4, "any", rng)
        start = (np.array([4096 - 60, 8192 - L // 2, 8192 - 3, ns - max(40, L - 300)]) - BASE).astype(np.int64)
        x, nb = rng.standard_normal((nch, ns)).astype(np.float32), rng.standard_normal((nch, ns2)).astype(np.float32)
        beam = rng.standard_normal((4, L)).astype(np.float32)
        fit = kp.fit_ref(x, delays, order, start, beam, None, nb)
        assert fit.valid.all()
        got = run.fit(x, ns, nb, ns2, delays, order, beam, start, None)
        amp = got[0].copy()
        y, tol, reached = kp.subtract_ref(x, delays, order, start, beam, amp, nb)
        assert not reached[:, :4000].any() and reached[:, 4096 - 1:4096 + 1].all() and reached[:, 8192 - 1:8192 + 1].all() and reached[:, ns - 1:ns + 1].all()
        out = run.sub(x, ns, nb, ns2, delays, order, beam, start, amp, False)
        wf, ws = kp.worst_fit(got, fit), kp.worst_subtract(out, y, tol, reached, np.concatenate([x, nb], axis=1))
        print("tiles, order %d, L = %d: worst error / tolerance: fit %.3g, subtraction %.3g" % (order, L, wf, ws))
        assert wf <= 1.0 and ws <= 1.0
        assert kp.same(out, run.sub(x, ns, nb, ns2, delays, order, beam, start, amp, True))
        worst = max(worst, wf, ws)
    return worst
