"""GPU tests of the alignment against the beam (csrc/align.hip) through das4whales_amd.loc.refine_arrivals, with NumPy input and
with CUDA tensor input.  The cases and the exact answers are those of tests/align_cases.py, which the CPU emulator runs as well
(tests/test_emu_align.py); the reference is the float64 restatement of tests/known_answers_align.py.

Tolerance, derived: |rho - rho_ref| <= (L + 8) 2^-24 (A / sqrt(tn en) + |rho_ref|) with A = sum |t| |x|; invalid lags NaN exactly,
zero-energy entries 0 exactly; the lag, the coefficient and the arrival time exactly those the pick rule gives on the returned
table.  No case is skipped or excluded.

End to end (test_end_to_end_refined_arrivals_are_sub_sample, bc.e2e_scene(), fixed seed), measured on an MI355X: the standard
deviation about the mean of Ti fs - tau over the 64 channels is 8.155 samples for locate_stack's envelope maxima and 0.187 for
the refined arrivals; the horizontal position error goes from 1.80 m to 0.93 m.  Worst error / tolerance of the coefficient
table over the parity cases on hardware: 0.111.
"""
import numpy as np
import pytest
import torch

from tests import align_cases as ac
from tests import beam_cases as bc
from tests import known_answers_align as ka
from tests.known_answers_loc import C0, make_cable

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available()
    import das4whales_amd as dw
    return dw


@pytest.fixture(scope="module")
def W(dw):
    return dw.loc.align_limits()[3]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_run(dw, container="tensor"):
    """The runner of align_cases on dw.loc.refine_arrivals.  "tensor": the buffers go to the device as they are and the block is
    a column-sliced view of them, read in place through its pitch; "numpy": the block is handed over as a NumPy array."""
    def run(buf, ns, nxt, ns2, template, r, start, M, weights, fs, min_coef, subsample):
        nch = buf.shape[0]
        cable = make_cable("line", max(nch, 2))[:nch]        # not used: the table is given
        pos = np.zeros((r.shape[0], 3))
        if container == "tensor":
            x = cuda(buf)[:, :ns]
            b = cuda(nxt)[:, :ns2] if nxt is not None else None
            out = dw.loc.refine_arrivals(x, fs, cable, C0, pos, cuda(template), cuda(start), M, min_coef, cuda(weights) if weights is not None else None,
                                         b, subsample, True, delays=cuda(r))
            assert all(isinstance(o, torch.Tensor) and o.is_cuda for o in out)
            assert [o.dtype for o in out] == [torch.float64, torch.float32, torch.int32, torch.float32]
            return tuple(o.cpu().numpy() for o in out)
        out = dw.loc.refine_arrivals(buf[:, :ns], fs, cable, C0, pos, template, start, M, min_coef, weights,
                                     nxt[:, :ns2] if nxt is not None else None, subsample, True, delays=r)
        assert all(isinstance(o, np.ndarray) for o in out)
        return out
    return run


@pytest.mark.parametrize("case", ac.parity_cases(), ids=ac.case_id)
def test_parity(dw, W, case):
    ac.check_parity(gpu_run(dw, "tensor" if case[9] % 4 else "numpy"), case, W)


def test_planted_template(dw, W):
    ac.check_planted(gpu_run(dw), W)


def test_bit_identity(dw, W):
    ac.check_bit_identity(gpu_run(dw), W)


def test_next_block_is_the_concatenation(dw, W):
    ac.check_next_block(gpu_run(dw), W)
    ac.check_next_block(gpu_run(dw, "numpy"), W)


def test_nan_sample(dw, W):
    ac.check_nan_sample(gpu_run(dw), W)


def test_zero_block_and_zero_template(dw, W):
    ac.check_zeros(gpu_run(dw), W)


def test_min_coef_and_subsample(dw, W):
    ac.check_min_coef_and_subsample(gpu_run(dw, "numpy"), W)


def test_the_limits_run(dw, W):
    """L = 4096 with M = 255 (the largest LDS image, above the 64 KiB a kernel gets without asking) on one channel more than a
    workgroup, windows across the seam and off the end."""
    _, L, M, _ = dw.loc.align_limits()
    nch, ns = W + 1, L + 500
    rng = np.random.default_rng(3)
    x, nb = rng.standard_normal((nch, ns)).astype(np.float32), rng.standard_normal((nch, 100)).astype(np.float32)
    t = rng.standard_normal((1, L)).astype(np.float32)
    r = (300 + 17 * np.arange(nch)[None, :]).astype(np.int32)
    start = np.zeros(1, dtype=np.int64)
    got = gpu_run(dw)(x, ns, nb, 100, t, r, start, M, None, ac.FS, 0.0, True)
    ref = ka.align_ref(x, t, r, start, M, None, nb)
    assert ref.valid.any() and not ref.valid.all() and ka.worst_ratio(got[3], ref) <= 1.0
    ac.check_picks(got, ref.n0, M, ac.FS)


def test_delays_given_against_built_inside_and_containers(dw, W):
    """delays= given and built inside: the same bits; NumPy in -> NumPy out, tensors in -> tensors on the caller's stream; one
    call given as vectors; no call, no launch."""
    nch, ns, L, M, fs = 2 * W + 3, 900, 65, 6, 50.0
    rng = np.random.default_rng(9)
    cable = make_cable("bent", nch)
    pos = bc.positions(cable, fs, 3, 0)
    x = rng.standard_normal((nch, ns)).astype(np.float32)
    t = rng.standard_normal((3, L)).astype(np.float32)
    r = dw.loc.beam_delays(cable, C0, fs, pos, rounded=True)
    start = (np.array([100, 0, 250]) - np.median(r, axis=1).astype(np.int64))
    inside = dw.loc.refine_arrivals(x, fs, cable, C0, pos, t, start, M, -1.0, return_all=True)
    given = dw.loc.refine_arrivals(x, fs, cable, C0, pos, t, start, M, -1.0, return_all=True, delays=r)
    assert all(isinstance(o, np.ndarray) for o in inside) and all(ka.same(a, b) for a, b in zip(inside, given))
    ref = ka.align_ref(x, t, r, start, M)
    assert ref.valid.any() and not ref.valid.all() and ka.worst_ratio(inside[3], ref) <= 1.0
    ac.check_picks(inside, ref.n0, M, fs, -1.0)
    two = dw.loc.refine_arrivals(x, fs, cable, C0, pos, t, start, M, -1.0)
    assert len(two) == 2 and ka.same(two[0], inside[0]) and ka.same(two[1], inside[1])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                            # a stream of the caller's: the work is ordered on it
        xt = cuda(x) * 8.0                                   # a power of two: the same table
        out = dw.loc.refine_arrivals(xt, fs, cable, C0, cuda(pos), cuda(t), cuda(start), M, -1.0, return_all=True)
        rho2 = out[3] * 1.0
    side.synchronize()
    assert all(o.is_cuda for o in out) and ka.same(rho2.cpu().numpy(), inside[3]) and ka.same(out[0].cpu().numpy(), inside[0])
    one = dw.loc.refine_arrivals(x, fs, cable, C0, pos[1], t[1], int(start[1]), M, -1.0, return_all=True)
    assert one[0].shape == (1, nch) and all(ka.same(a[0], b[1]) for a, b in zip(one, inside))
    none = dw.loc.refine_arrivals(x, fs, cable, C0, np.zeros((0, 3)), np.zeros((0, L), dtype=np.float32), 0, M, return_all=True)
    assert [o.shape for o in none] == [(0, nch), (0, nch), (0, nch), (0, nch, 2 * M + 1)]
    f64 = dw.loc.refine_arrivals(x.astype(np.float64), fs, cable, C0, pos, t, start, M, -1.0)    # anything else: a float32 copy
    assert ka.same(f64[0], inside[0])


def test_a_tensor_start_with_a_numpy_trace_and_views_across_the_seam(dw):
    """The smallest record that can still go wrong: 5 channels, 64 samples, a next block of 9, two calls with a start each, the
    second call's windows across the seam and partly off the end.  With NumPy arrays, with NumPy blocks and a tensor start (any
    tensor in -> tensors out), and with column-sliced CUDA views throughout: the same bits, and within the derived tolerance of
    the float64 restatement."""
    nch, ns, ns2, L, M, fs = 5, 64, 9, 10, 2, 200.0
    rng = np.random.default_rng(15)
    cable = np.stack([30.0 * np.arange(nch), np.zeros(nch), np.full(nch, -20.0)], axis=1)       # moveouts of 6 .. 16 samples
    pos = np.array([[10.0, 40.0, -5.0], [100.0, -60.0, -5.0]])
    buf, nbuf = rng.standard_normal((nch, ns + 3)).astype(np.float32), rng.standard_normal((nch, ns2 + 2)).astype(np.float32)
    x, nb = buf[:, :ns], nbuf[:, :ns2]
    t = rng.standard_normal((2, L)).astype(np.float32)
    r = dw.loc.beam_delays(cable, C0, fs, pos, rounded=True)
    start = np.array([20, ns - 8], dtype=np.int64) - np.median(r, axis=1).astype(np.int64)
    ref = ka.align_ref(x, t, r, start, M, None, nb)
    q = np.array(ref.n0.tolist(), dtype=np.int64)[:, :, None] + np.arange(-M, M + 1)
    assert ref.valid[0].all() and not ref.valid[1].all() and (ref.valid & (q < ns) & (q + L > ns)).any()      # a window across the seam
    host = dw.loc.refine_arrivals(x, fs, cable, C0, pos, t, start, M, -1.0, next_block=nb, return_all=True)
    assert all(isinstance(o, np.ndarray) for o in host) and ka.worst_ratio(host[3], ref) <= 1.0
    ac.check_picks(host, ref.n0, M, fs, -1.0)
    mixed = dw.loc.refine_arrivals(x, fs, cable, C0, pos, t, cuda(start), M, -1.0, next_block=nb, return_all=True)
    views = dw.loc.refine_arrivals(cuda(buf)[:, :ns], fs, cable, C0, cuda(pos), cuda(t), cuda(start), M, -1.0, next_block=cuda(nbuf)[:, :ns2],
                                   return_all=True, delays=cuda(r))
    for out in (mixed, views):
        assert all(isinstance(o, torch.Tensor) and o.is_cuda for o in out)
        assert all(ka.same(o.cpu().numpy(), h) for o, h in zip(out, host))


def test_bad_arguments(dw):
    nch, ns, L = 5, 64, 8
    base = dict(trace=np.ones((nch, ns), dtype=np.float32), fs=50.0, cable_pos=make_cable("line", nch), c0=C0, pos=np.zeros((2, 3)),
                template=np.ones((2, L), dtype=np.float32), start=np.zeros(2, dtype=np.int64), max_lag=2)
    assert dw.loc.refine_arrivals(**base)[0].shape == (2, nch)
    for kw in (dict(template=np.ones((2, L))), dict(template=np.ones((3, L), dtype=np.float32)), dict(template=np.ones((2, 0), dtype=np.float32)),
               dict(max_lag=-1), dict(max_lag=1.5), dict(max_lag=dw.loc.align_limits()[2] + 1), dict(min_coef=float("nan")), dict(start=1.5),
               dict(delays=np.zeros((2, nch), dtype=np.int64)), dict(delays=np.zeros((2, nch - 1), dtype=np.int32)), dict(fs=0.0),
               dict(weights=np.ones(4)), dict(next_block=np.ones((4, 9), dtype=np.float32)), dict(pos=np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            dw.loc.refine_arrivals(**dict(base, **kw))


def _spread(Ti, fs, tau):
    """(standard deviation about the mean of Ti fs - tau over the channels with an arrival, their number)."""
    d = (Ti * fs - tau)[~np.isnan(Ti)]
    return float(np.std(d - d.mean())), len(d)


def test_end_to_end_refined_arrivals_are_sub_sample(dw):
    """A 20 Hz tone burst under unit-variance noise on a 64-channel bent cable (bc.e2e_scene()): matched-filter envelopes ->
    locate_stack -> solve_lq_batch(fix_z) -> beamform(order=3, 20 samples of lead) -> refine_arrivals(max_lag=4) ->
    solve_lq_batch.  The arrival-time error about its mean must fall strictly below that of locate_stack's envelope maxima and
    below one sample, and the second solve must not be more than 1 m further from the source than the first."""
    sc = bc.e2e_scene()
    cable, xs, ys, z, x, burst, tau = (sc[k] for k in ("cable", "xs", "ys", "z", "x", "burst", "tau"))
    fs = bc.E2E_FS
    env = bc.matched_envelope(x, burst)
    Ti, info = dw.loc.locate_stack(env, fs, cable, C0, xs, ys, z, 900.0, 30, 0.0)
    assert Ti.shape == (1, bc.E2E_NCH)
    n = dw.loc.solve_lq_batch(Ti, cable, C0, fix_z=True, first_guess=info["first_guess"])
    lead = 20
    start = np.round(n[:, 3] * fs).astype(np.int64) - lead
    beam, _ = dw.loc.beamform(x, fs, cable, C0, n[:, :3], start=start, length=len(burst) + 2 * lead, order=3)
    Ti2, coef = dw.loc.refine_arrivals(x, fs, cable, C0, n[:, :3], beam, start, 4)
    before, nb = _spread(Ti[0], fs, tau)
    after, na = _spread(Ti2[0], fs, tau)
    print("arrival-time error about its mean, samples: locate_stack %.3f (%d channels), refined %.3f (%d channels, median coefficient %.3f)"
          % (before, nb, after, na, float(np.nanmedian(coef))))
    n2 = dw.loc.solve_lq_batch(Ti2, cable, C0, fix_z=True, first_guess=n)
    e1 = float(np.hypot(n[0, 0] - bc.E2E_SOURCE[0], n[0, 1] - bc.E2E_SOURCE[1]))
    e2 = float(np.hypot(n2[0, 0] - bc.E2E_SOURCE[0], n2[0, 1] - bc.E2E_SOURCE[1]))
    print("horizontal position error, m: first solve %.2f, after refinement %.2f" % (e1, e2))
    assert na >= bc.E2E_NCH // 2
    assert after < before
    assert after < 1.0
    assert e2 <= e1 + 1.0
