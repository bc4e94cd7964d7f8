"""GPU tests of the transpose of the beam (csrc/project.hip) through das4whales_amd.loc.project_calls / subtract_calls /
remove_calls, alternately with CUDA views and NumPy arrays.  The cases and the exact answers are those of
tests/project_cases.py, which the CPU emulator runs as well (tests/test_emu_project.py); the reference is the float64
restatement of tests/known_answers_project.py, with the tolerances derived there.  No case is skipped or excluded.

Measured on an MI355X, worst error / tolerance: over the 36 parity cases fit 0.0356 and subtraction 0.898; the multi-tile cases
fit 0.0027 and subtraction 0.988; the dot-product test against beamform 0.00151 / 0.00034 / 0.00028 for order 0 / 1 / 3.
End to end (test_end_to_end_remove_the_loud_call): in the restatement the relative error energy of B's beam is 0.1254 before
and 0.003987 after removing A (a factor of 31.4; amp x 16 / gain of A between 1.024 and 1.094); the device's beam, fit and
residual lie at 0.069, 0.0046 and 0.52 of their derived bounds, and B's beam from the device's residual has 0.003987 as well.
"""
import numpy as np
import pytest
import torch

from tests import known_answers_beam as kb
from tests import known_answers_project as kp
from tests import project_cases as pc
from tests.known_answers_loc import C0, make_cable

pytestmark = pytest.mark.gpu
FS = 200.0


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available()
    import das4whales_amd as dw
    return dw


@pytest.fixture(scope="module")
def W(dw):
    return dw.loc.project_limits()[2]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else t


class DeviceRun:
    """The runner of project_cases on dw.loc.  "tensor": the buffers go to the device as they are and the blocks are
    column-sliced views of them, used in place through their pitch; "numpy": the blocks are handed over as NumPy arrays (the
    subtraction in place always takes views: there is nothing else to write into)."""

    def __init__(self, dw, container="tensor"):
        self.dw, self.container = dw, container

    def _geometry(self, delays, order):
        k = delays if order == 0 else delays[0]
        nch = k.shape[1]
        return make_cable("line", max(nch, 2))[:nch], np.zeros((k.shape[0], 3))         # not used: the table is given

    def _blocks(self, buf, ns, nxt, ns2, tensor):
        if tensor:
            return cuda(buf)[:, :ns], (cuda(nxt)[:, :ns2] if nxt is not None else None)
        return buf[:, :ns], (nxt[:, :ns2] if nxt is not None else None)

    def _tables(self, delays, order, tensor):
        if not tensor:
            return delays
        return cuda(delays) if order == 0 else tuple(cuda(t) for t in delays)

    def fit(self, buf, ns, nxt, ns2, delays, order, beam, start, weights):
        t = self.container == "tensor"
        cable, pos = self._geometry(delays, order)
        x, b = self._blocks(buf, ns, nxt, ns2, t)
        out = self.dw.loc.project_calls(x, FS, cable, C0, pos, cuda(beam) if t else beam, cuda(start) if t else start, order,
                                        (cuda(weights) if t else weights) if weights is not None else None, b, delays=self._tables(delays, order, t))
        assert all((isinstance(o, torch.Tensor) and o.is_cuda and o.dtype == torch.float32) if t else isinstance(o, np.ndarray) for o in out)
        return tuple(host(o) for o in out)

    def sub(self, buf, ns, nxt, ns2, delays, order, beam, start, amp, inplace):
        t = inplace or self.container == "tensor"
        cable, pos = self._geometry(delays, order)
        x, b = self._blocks(buf, ns, nxt, ns2, t)
        whole = (x._base, b._base if b is not None else None) if t else None
        out = self.dw.loc.subtract_calls(x, FS, cable, C0, pos, cuda(beam) if t else beam, cuda(start) if t else start, cuda(amp) if t else amp, order,
                                         b, inplace, delays=self._tables(delays, order, t))
        out = out if isinstance(out, tuple) else (out,)
        assert len(out) == (1 if nxt is None else 2)
        if inplace:
            assert out[0] is x and (b is None or out[1] is b)
        if t:                                                # the buffers the views live in: the padding keeps its bits
            for w, given, n in zip(whole, (buf, nxt), (ns, ns2)):
                if w is not None:
                    assert kp.same(w.cpu().numpy()[:, n:], np.ascontiguousarray(given[:, n:]))
                    if not inplace:
                        assert kp.same(w.cpu().numpy(), np.ascontiguousarray(given))
        return np.concatenate([host(o) for o in out], axis=1)

    def beam(self, buf, ns, nxt, ns2, delays, order, start, nt):
        cable, pos = self._geometry(delays, order)
        x, b = self._blocks(buf, ns, nxt, ns2, False)
        return self.dw.loc.beamform(x, FS, cable, C0, pos, start, nt, order, None, False, b, delays=delays)[0]


def test_limits(dw):
    max_calls, max_length, W = dw.loc.project_limits()
    assert max_calls >= 64 and max_length >= 1 << 20 and W >= 2


WORST = {"fit": 0.0, "sub": 0.0}


@pytest.mark.parametrize("case", pc.parity_cases(), ids=pc.case_id)
def test_parity(dw, W, case):
    wf, ws = pc.check_parity(DeviceRun(dw, "tensor" if case[9] % 2 else "numpy"), case, W)
    WORST["fit"], WORST["sub"] = max(WORST["fit"], wf), max(WORST["sub"], ws)
    print("worst so far: fit %.3g, subtraction %.3g" % (WORST["fit"], WORST["sub"]))


@pytest.mark.parametrize("case", pc.parity_cases()[::3], ids=pc.case_id)
def test_poison(dw, W, case):
    pc.check_poison(DeviceRun(dw, "numpy" if case[9] % 2 else "tensor"), case, W)


def test_identical_channels(dw, W):
    pc.check_identical_channels(DeviceRun(dw), W)
    pc.check_identical_channels(DeviceRun(dw, "numpy"), W)


def test_power_of_two_scaling(dw, W):
    pc.check_power_of_two(DeviceRun(dw, "numpy"), W)


def test_zero_beam(dw, W):
    pc.check_zero_beam(DeviceRun(dw), W)


def test_nan_samples_rows_and_amplitudes(dw, W):
    pc.check_nan_samples(DeviceRun(dw, "numpy"), W)


def test_batch_and_split_independence(dw, W):
    pc.check_batch_and_split(DeviceRun(dw), W)
    pc.check_batch_and_split(DeviceRun(dw, "numpy"), W)


def test_call_order(dw, W):
    pc.check_call_order(DeviceRun(dw), W)
    pc.check_call_order(DeviceRun(dw, "numpy"), W)


def test_transpose_of_the_beam(dw, W):
    pc.check_transpose(DeviceRun(dw), W)


def test_more_than_one_tile_and_lds_piece(dw, W):
    pc.check_tiles(DeviceRun(dw), W)
    pc.check_tiles(DeviceRun(dw, "numpy"), W)


def test_more_than_one_tile_and_the_callers_stream(dw, W):
    """A record of five subtraction tiles (2048 samples each; the last 700 samples in the next block), supports across the
    tile borders at 4096 and 8192 and the seam; delays built inside against delays given; the work ordered on the caller's stream."""
    nch, ns, ns2, L, order = 2 * W + 3, 8777, 700, 129, 3
    rng = np.random.default_rng(77)
    cable = np.stack([10.0 * np.arange(nch), np.zeros(nch), np.full(nch, -50.0)], axis=1)       # moveouts of 25 .. 70 samples
    pos = np.array([[-200.0, 100.0, -10.0], [50.0, 300.0, -10.0], [400.0, -250.0, -10.0]])
    x, nb = rng.standard_normal((nch, ns)).astype(np.float32), rng.standard_normal((nch, ns2)).astype(np.float32)
    beam = rng.standard_normal((3, L)).astype(np.float32)
    k, f = dw.loc.beam_delays(cable, C0, FS, pos)
    start = np.array([4096 - 60, 8192 - 3, ns - 40]) - np.median(k, axis=1).astype(np.int64)
    fit = kp.fit_ref(x, (k, f), order, start, beam, None, nb)
    assert fit.valid.all()
    inside = dw.loc.project_calls(x, FS, cable, C0, pos, beam, start, order, next_block=nb)
    given = dw.loc.project_calls(x, FS, cable, C0, pos, beam, start, order, next_block=nb, delays=(k, f))
    assert all(kp.same(a, b) for a, b in zip(inside, given)) and kp.worst_fit(inside, fit) <= 1.0
    y, tol, reached = kp.subtract_ref(x, (k, f), order, start, beam, inside[0], nb)
    out = dw.loc.subtract_calls(x, FS, cable, C0, pos, beam, start, inside[0], order, nb)
    assert kp.worst_subtract(np.concatenate(out, axis=1), y, tol, reached, np.concatenate([x, nb], axis=1)) <= 1.0
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        xt, nt = cuda(x) * 2.0, cuda(nb) * 2.0
        amp, coef = dw.loc.project_calls(xt, FS, cable, C0, cuda(pos), cuda(beam), cuda(start), order, next_block=nt)
        res = dw.loc.subtract_calls(xt, FS, cable, C0, pos, cuda(beam), start, amp, order, nt, inplace=True)
        halves = [r * 0.5 for r in res]
    side.synchronize()
    assert res[0] is xt and res[1] is nt and kp.same(amp.cpu().numpy(), inside[0] * np.float32(2)) and kp.same(coef.cpu().numpy(), inside[1])
    assert kp.same(np.concatenate([h.cpu().numpy() for h in halves], axis=1), np.concatenate(out, axis=1))


def test_remove_calls_across_the_seam_in_both_containers(dw):
    """remove_calls on the smallest record that can still go wrong: 5 channels, 64 samples, a next block of 9, two calls with
    a start each, the second call's supports across the seam (and one of them off the end of the record).  Once with NumPy
    arrays and once with column-sliced CUDA views and a tensor start: the same bits in both containers, out of place and in
    place, and the beam, the fit and the residual within the derived bounds of the float64 restatement, carried through the
    chain as in test_end_to_end_remove_the_loud_call.  min_coef=None: no amplitude is masked."""
    nch, ns, ns2, L, order = 5, 64, 9, 12, 1
    rng = np.random.default_rng(5)
    cable = np.stack([30.0 * np.arange(nch), np.zeros(nch), np.full(nch, -20.0)], axis=1)       # moveouts of 6 .. 16 samples
    pos = np.array([[10.0, 40.0, -5.0], [100.0, -60.0, -5.0]])
    buf, nbuf = rng.standard_normal((nch, ns + 3)).astype(np.float32), rng.standard_normal((nch, ns2 + 2)).astype(np.float32)
    x, nb = buf[:, :ns], nbuf[:, :ns2]
    delays = dw.loc.beam_delays(cable, C0, FS, pos)
    start = np.array([20, ns - 8], dtype=np.int64) - np.median(delays[0], axis=1).astype(np.int64)
    # the float64 restatement of the chain
    beam_r, tol_b, _, _ = kb.beam_ref(x, delays, order, start, L, None, True, nb)
    fit = kp.fit_ref(x, delays, order, start, beam_r, None, nb)
    assert fit.valid[0].all() and fit.valid[1].any() and not fit.valid[1].all()
    assert (fit.valid & (fit.lo < ns) & (fit.lo + fit.W > ns)).any()                            # a support across the seam
    dfit = kp.fit_ref(x, delays, order, start, beam_r, None, nb, beam_tol=tol_b)
    y, tol_y, reached = kp.subtract_ref(x, delays, order, start, beam_r, fit.amp, nb, amp_tol=dfit.tol_amp, beam_tol=tol_b)
    # NumPy in, NumPy out
    got = dw.loc.remove_calls(x, FS, cable, C0, pos, start, L, order, None, next_block=nb, return_parts=True)
    assert len(got) == 5 and all(isinstance(o, np.ndarray) and o.dtype == np.float32 for o in got)
    res, res2, beam, amp, coef = got
    rb, rf = kb.worst_ratio(beam, beam_r, tol_b), kp.worst_fit((amp, coef), dfit)
    ry = kp.worst_subtract(np.concatenate([res, res2], axis=1), y, tol_y, reached, np.concatenate([x, nb], axis=1))
    print("device / bound: beam %.3g, fit %.3g, residual %.3g" % (rb, rf, ry))
    assert rb <= 1.0 and rf <= 1.0 and ry <= 1.0
    # column-sliced CUDA views and a tensor start: tensors on the device with the same bits
    xt, nt = cuda(buf)[:, :ns], cuda(nbuf)[:, :ns2]
    gt = dw.loc.remove_calls(xt, FS, cable, C0, pos, cuda(start), L, order, None, next_block=nt, return_parts=True)
    assert all(isinstance(o, torch.Tensor) and o.is_cuda for o in gt) and all(kp.same(host(a), b) for a, b in zip(gt, got))
    assert kp.same(host(xt._base), buf) and kp.same(host(nt._base), nbuf)                       # out of place: the views keep their bits
    out = dw.loc.remove_calls(xt, FS, cable, C0, pos, cuda(start), L, order, None, next_block=nt, inplace=True)
    assert out[0] is xt and out[1] is nt and kp.same(host(xt), res) and kp.same(host(nt), res2)
    assert kp.same(host(xt._base)[:, ns:], buf[:, ns:]) and kp.same(host(nt._base)[:, ns2:], nbuf[:, ns2:])      # the padding too


# ---- end to end --------------------------------------------------------------------------------------------------------------
def sweep(n=200):
    """A Hann-windowed 25 -> 15 Hz sweep of n samples at FS."""
    t = np.arange(n) / FS
    return np.hanning(n) * np.sin(2 * np.pi * (25.0 * t - 0.5 * (10.0 / (n / FS)) * t * t))


def two_call_scene():
    """64-channel line cable, 60 m spacing, 4096 samples at 200 Hz, c0 = 1500 m/s, white noise sigma = 0.2; call A, amplitude
    8 .. 24 over the channels, at (1500, 800, -30); call B, amplitude 1, emitted 40 samples later at (2600, -1200, -30)."""
    nch, ns, c0 = 64, 4096, 1500.0
    rng = np.random.default_rng(20260)
    cable = np.stack([60.0 * np.arange(nch), np.zeros(nch), np.full(nch, -100.0)], axis=1)
    pos = np.array([[1500.0, 800.0, -30.0], [2600.0, -1200.0, -30.0]])
    start = np.array([1000, 1040], dtype=np.int64)
    s = sweep()
    tau = kb.tau(cable, c0, FS, pos)
    n = np.arange(ns)
    clean = np.zeros((2, nch, ns))
    gain = np.stack([np.linspace(8.0, 24.0, nch), np.ones(nch)])
    for c in range(2):
        for ch in range(nch):
            clean[c, ch] = gain[c, ch] * np.interp(n - start[c] - tau[c, ch], np.arange(len(s)), s, left=0.0, right=0.0)
    x = (clean.sum(0) + 0.2 * rng.standard_normal((nch, ns))).astype(np.float32)
    return x, clean, cable, c0, pos, start, tau


def test_end_to_end_remove_the_loud_call(dw):
    """The two-call scene through remove_calls (order 1, length 230: the 200-sample sweep and a margin).  In the float64
    restatement of the whole chain (beam of A, fit, subtraction; then the beam toward B) the relative error energy of B's beam
    against B's noise-free beam falls from "before" to "after" removing A: the test asserts after < before and prints
    both.  The device's beam, amp and residual each lie within the derived bound of the restatement's: the beam within
    known_answers_beam's tolerance, amp within tol_amp with the beam's tolerance carried through (fit_ref's beam_tol), the
    residual within tol_y with both carried through (subtract_ref's amp_tol and beam_tol)."""
    x, clean, cable, c0, pos, start, tau = two_call_scene()
    order, L = 1, 230
    delays = kb.split(tau)
    A, B = slice(0, 1), slice(1, 2)
    dA, dB = (delays[0][A], delays[1][A]), (delays[0][B], delays[1][B])
    # the float64 restatement of the chain
    beamA, tolA, nA, _ = kb.beam_ref(x, dA, order, start[A], L, None, True)
    fit = kp.fit_ref(x, dA, order, start[A], beamA)
    assert fit.valid.all() and fit.coef.min() > 0
    y, _, _ = kp.subtract_ref(x, dA, order, start[A], beamA, fit.amp)
    truthB = kb.beam_ref(clean[1], dB, order, start[B], L, None, True)[0]
    before = kb.beam_ref(x, dB, order, start[B], L, None, True)[0]
    after = kb.beam_ref(y, dB, order, start[B], L, None, True)[0]
    eb, ea = (((b - truthB) ** 2).sum() / (truthB ** 2).sum() for b in (before, after))
    rel = fit.amp[0] * 16.0 / np.linspace(8.0, 24.0, 64)     # the normalized beam carries the mean gain, 16
    print("restatement: relative error energy of B's beam %.4g before, %.4g after removing A (factor %.3g); amp x 16 / gain of A %.4f .. %.4f"
          % (eb, ea, eb / ea, rel.min(), rel.max()))
    assert ea < eb
    # the device
    res, beam, amp, coef = dw.loc.remove_calls(x, FS, cable, c0, pos[0], int(start[0]), L, order, return_parts=True)
    assert isinstance(res, np.ndarray) and res.shape == x.shape and res.dtype == np.float32 and beam.shape == (1, L)
    rb = kb.worst_ratio(beam, beamA, tolA)
    dfit = kp.fit_ref(x, dA, order, start[A], beamA, beam_tol=tolA)
    rf = kp.worst_fit((amp, coef), dfit)
    yd, told, reached = kp.subtract_ref(x, dA, order, start[A], beamA, fit.amp, amp_tol=dfit.tol_amp, beam_tol=tolA)
    ry = kp.worst_subtract(res, yd, told, reached, x)
    print("device / bound: beam %.3g, fit %.3g, residual %.3g" % (rb, rf, ry))
    assert rb <= 1.0 and rf <= 1.0 and ry <= 1.0
    # the same through tensors, in place, with the second call's beam taken from the residual on the device
    xt = cuda(x)
    out = dw.loc.remove_calls(xt, FS, cable, c0, pos[0], int(start[0]), L, order, inplace=True)
    assert out is xt and kp.same(xt.cpu().numpy(), res)
    bB = dw.loc.beamform(xt, FS, cable, c0, pos[1], int(start[1]), L, order, normalize=True)[0].cpu().numpy()
    ed = ((bB[0] - truthB[0]) ** 2).sum() / (truthB[0] ** 2).sum()
    print("device: relative error energy of B's beam after removing A %.4g" % ed)
    assert ed < eb
