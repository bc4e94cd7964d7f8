"""GPU tests of the delay-and-sum beam (csrc/beam.hip) through das4whales_amd.loc: beam_delays and beamform, with NumPy input
and with CUDA tensor input.  The cases and the exact answers are those of tests/beam_cases.py, which the CPU emulator runs as
well (tests/test_emu_beam.py); the reference is the float64 restatement of tests/known_answers_beam.py.

Tolerance, derived: |beam - ref| <= (n + 16) 2^-24 A with n the contributing channels and A the sum of the absolute terms;
with normalize that bound over the weight sum plus 2 x 2^-24 |ref|.  No case is skipped or excluded.
"""
import numpy as np
import pytest
import torch

from tests import beam_cases as bc
from tests import known_answers_beam as kb
from tests.known_answers_loc import C0, make_cable

pytestmark = pytest.mark.gpu
FS = 50.0                                                    # the runner hands the delay table over: the rate only scales the times


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available()
    import das4whales_amd as dw
    return dw


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_run(dw, container="tensor"):
    """The runner of beam_cases on dw.loc.beamform.  "tensor": the buffers go to the device as they are and the block is a
    column-sliced view of them, read in place through its pitch; "numpy": the block is handed over as a NumPy array."""
    def run(buf, ns, nxt, ns2, delays, order, weights, start, nt, normalize):
        nch = buf.shape[0]
        cable = make_cable("line", max(nch, 2))[:nch]        # not used: the table is given
        pos = np.zeros(((delays if order == 0 else delays[0]).shape[0], 3))
        if container == "tensor":
            x = cuda(buf)[:, :ns]
            b = cuda(nxt)[:, :ns2] if nxt is not None else None
            d = cuda(delays) if order == 0 else tuple(cuda(a) for a in delays)
            beam, times = dw.loc.beamform(x, FS, cable, C0, pos, start=cuda(start), length=nt, order=order,
                                          weights=cuda(weights) if weights is not None else None, normalize=normalize, next_block=b, delays=d)
            assert isinstance(beam, torch.Tensor) and beam.is_cuda and beam.dtype == torch.float32
            assert isinstance(times, torch.Tensor) and times.is_cuda and times.dtype == torch.float64
            beam, times = beam.cpu().numpy(), times.cpu().numpy()
        else:
            beam, times = dw.loc.beamform(buf[:, :ns], FS, cable, C0, pos, start=start, length=nt, order=order, weights=weights,
                                          normalize=normalize, next_block=nxt[:, :ns2] if nxt is not None else None, delays=delays)
            assert isinstance(beam, np.ndarray) and beam.dtype == np.float32 and isinstance(times, np.ndarray) and times.dtype == np.float64
        assert np.array_equal(times, (np.asarray(start)[:, None] + np.arange(nt)[None, :]) / FS)
        return beam
    return run


def gpu_delays(dw):
    def delays(cable, c0, fs, pos, rounded):
        return dw.loc.beam_delays(cable, c0, fs, pos, rounded=rounded)
    return delays


@pytest.fixture(scope="module")
def dims(dw):
    max_calls, max_length, S, T = dw.loc.beam_limits()
    return T, S


@pytest.mark.parametrize("case", bc.parity_cases(), ids=bc.case_id)
def test_parity(dw, dims, case):
    bc.check_parity(gpu_run(dw, "tensor" if case[10] % 4 else "numpy"), case, *dims)


def test_delay_table(dw):
    bc.check_delays(gpu_delays(dw))


def test_delay_containers(dw):
    cable, fs, pos = bc.delay_scenes()[2]
    k, f = dw.loc.beam_delays(cable, C0, fs, pos)
    r = dw.loc.beam_delays(cable, C0, fs, pos, rounded=True)
    kt, ft = dw.loc.beam_delays(cuda(cable), C0, fs, cuda(pos))
    rt = dw.loc.beam_delays(cable, C0, fs, cuda(pos), True)
    for a, b, dtype in ((k, kt, torch.int32), (f, ft, torch.float32), (r, rt, torch.int32)):
        assert isinstance(a, np.ndarray) and isinstance(b, torch.Tensor) and b.is_cuda and b.dtype == dtype
        assert np.array_equal(a, b.cpu().numpy())
    k1, f1 = dw.loc.beam_delays(cable, C0, fs, pos[1])       # one position as a vector: still [1 x channel]
    assert k1.shape == (1, len(cable)) and np.array_equal(k1[0], k[1]) and np.array_equal(f1[0], f[1])
    k0, f0 = dw.loc.beam_delays(cable, C0, fs, np.zeros((0, 3)))
    assert k0.shape == (0, len(cable)) and f0.shape == (0, len(cable)) and k0.dtype == np.int32 and f0.dtype == np.float32


@pytest.mark.parametrize("nch", [5, "S", "S+1"])
def test_rounded_delays_are_the_stack_table_and_order_0_its_columns(dw, dims, nch):
    S = dims[1]
    nch = {"S": S, "S+1": S + 1}.get(nch, nch)
    cable, fs, xs, ys, z, env, w, k_range = bc.stack_scene(nch)
    table = dw.loc.delay_table(cable, C0, fs, xs, ys, z)
    r = dw.loc.beam_delays(cable, C0, fs, bc.stack_nodes(xs, ys, z), rounded=True)
    assert np.array_equal(r, table.reshape(-1, nch))
    stack, _ = dw.loc.stack_grid(env, fs, cable, C0, xs, ys, z, weights=w, k_range=k_range)
    bc.check_against_stack(gpu_run(dw), stack, r, nch, S)


def test_ones(dw, dims):
    bc.check_ones(gpu_run(dw), dims[1])


def test_ramp(dw, dims):
    bc.check_ramp(gpu_run(dw), *dims)


def test_zeros(dw, dims):
    bc.check_zeros(gpu_run(dw), *dims)


def test_nan_rows(dw, dims):
    bc.check_nan_rows(gpu_run(dw), *dims)


def test_bit_identity(dw, dims):
    bc.check_bit_identity(gpu_run(dw), *dims)


def test_next_block_is_the_concatenation(dw, dims):
    bc.check_next_block(gpu_run(dw), *dims)
    bc.check_next_block(gpu_run(dw, "numpy"), *dims)


def test_delays_given_against_built_inside_and_containers(dw, dims):
    """delays= given and built inside: the same bits; NumPy in -> NumPy out, tensors in -> tensors on the current stream."""
    T, S = dims
    nch, ns, nt = S + 5, T + 200, T + 3
    rng = np.random.default_rng(9)
    cable = make_cable("bent", nch)
    pos = bc.positions(cable, FS, 3, 0)
    x = rng.standard_normal((nch, ns)).astype(np.float32)
    start = np.array([0, -30, 250])
    side = torch.cuda.Stream()
    for order in bc.ORDERS:
        d = dw.loc.beam_delays(cable, C0, FS, pos, rounded=order == 0)
        inside, times = dw.loc.beamform(x, FS, cable, C0, pos, start, nt, order)
        given, _ = dw.loc.beamform(x, FS, cable, C0, pos, start, nt, order, delays=d)
        assert isinstance(inside, np.ndarray) and inside.dtype == np.float32 and inside.shape == (3, nt) and inside.any()
        assert times.dtype == np.float64 and np.array_equal(times, (start[:, None] + np.arange(nt)[None, :]) / FS)
        assert np.array_equal(inside, given)
        ref, tol, _, _ = kb.beam_ref(x, d, order, start, nt)
        assert kb.worst_ratio(inside, ref, tol) <= 1.0
        with torch.cuda.stream(side):                        # a stream of the caller's: the work is ordered on it
            xt = cuda(x) * 2.0
            beam_t, times_t = dw.loc.beamform(xt, FS, cable, C0, cuda(pos), cuda(start), nt, order)
            twice = beam_t * 0.5
        side.synchronize()
        assert beam_t.is_cuda and times_t.is_cuda and np.array_equal(twice.cpu().numpy(), inside)
    one, t1 = dw.loc.beamform(x, FS, cable, C0, pos[1], start=-30, length=nt)     # one position as a vector, an int start
    assert one.shape == (1, nt) and np.array_equal(one[0], dw.loc.beamform(x, FS, cable, C0, pos, start, nt)[0][1]) and t1[0, 0] == -30 / FS
    full, tf = dw.loc.beamform(x, FS, cable, C0, pos[:1])    # the default length: the samples of the trace
    assert full.shape == (1, ns) and tf.shape == (1, ns)
    none, tn = dw.loc.beamform(x, FS, cable, C0, np.zeros((0, 3)), length=7)      # no call: no launch
    assert none.shape == (0, 7) and none.dtype == np.float32 and tn.shape == (0, 7) and tn.dtype == np.float64
    f64, _ = dw.loc.beamform(x.astype(np.float64), FS, cable, C0, pos, start, nt)            # anything else: a float32 copy
    assert np.array_equal(f64, dw.loc.beamform(x, FS, cable, C0, pos, start, nt)[0])


def test_bad_arguments(dw):
    nch, ns = 5, 64
    cable = make_cable("line", nch)
    x = np.ones((nch, ns), dtype=np.float32)
    pos = np.zeros((2, 3))
    base = dict(trace=x, fs=50.0, cable_pos=cable, c0=C0, pos=pos)
    k, f = np.zeros((2, nch), dtype=np.int32), np.zeros((2, nch), dtype=np.float32)
    assert dw.loc.beamform(**base, delays=(k, f))[0].shape == (2, ns)
    for kw in (dict(order=2), dict(order=-1), dict(order=1.5), dict(length=0), dict(length=-3), dict(length=2.5), dict(trace=np.ones((4, ns), dtype=np.float32)),
               dict(trace=np.ones(ns)), dict(next_block=np.ones((4, 9), dtype=np.float32)), dict(next_block=np.ones(9)), dict(fs=0.0),
               dict(fs=float("nan")), dict(fs=float("inf")), dict(c0=-1.0), dict(c0=float("nan")), dict(pos=np.zeros((2, 2))), dict(pos=np.zeros(4)),
               dict(start=np.zeros(3, dtype=np.int64)), dict(start=np.zeros((2, 1), dtype=np.int64)), dict(start=1.5), dict(weights=np.ones(4)),
               dict(cable_pos=np.zeros((5, 2))), dict(delays=(k[:1], f[:1])), dict(delays=(k, f.astype(np.float64))), dict(delays=(k,)),
               dict(order=0, delays=f), dict(order=0, delays=k[:, :4]), dict(pos=np.zeros((dw.loc.beam_limits()[0] + 1, 3)))):
        with pytest.raises(ValueError):
            dw.loc.beamform(**dict(base, **kw))
    for kw in (dict(fs=0.0), dict(c0=float("inf")), dict(pos=np.zeros((2, 2))), dict(cable_pos=np.zeros((5, 2)))):
        with pytest.raises(ValueError):
            dw.loc.beam_delays(**dict(dict(cable_pos=cable, c0=C0, fs=50.0, pos=pos), **kw))


def test_end_to_end_beam_beats_the_best_channel(dw):
    """A 20 Hz tone burst under unit-variance noise on a 64-channel bent cable: matched-filter envelopes -> locate_stack ->
    solve_lq_batch -> beamform(order=3).  The beam's correlation coefficient with the planted burst exceeds the best single
    channel's (float64, fixed seed; the float64 restatement of the same chain gives 0.937 against 0.530 for this seed)."""
    sc = bc.e2e_scene()
    cable, xs, ys, z, x, burst = (sc[k] for k in ("cable", "xs", "ys", "z", "x", "burst"))
    fs = bc.E2E_FS
    env = bc.matched_envelope(x, burst)
    Ti, info = dw.loc.locate_stack(env, fs, cable, C0, xs, ys, z, 900.0, 30, 0.0)
    assert Ti.shape == (1, bc.E2E_NCH)
    n = dw.loc.solve_lq_batch(Ti, cable, C0, fix_z=True, first_guess=info["first_guess"])
    assert np.hypot(n[0, 0] - bc.E2E_SOURCE[0], n[0, 1] - bc.E2E_SOURCE[1]) < 100.0 and abs(n[0, 3] - bc.E2E_T0) < 0.05
    lead = 50
    start = np.round(n[:, 3] * fs).astype(np.int64) - lead
    beam, times = dw.loc.beamform(x, fs, cable, C0, n[:, :3], start=start, length=len(burst) + 2 * lead, order=3, normalize=True)
    got = bc.best_correlation(beam[0], burst, lead)
    single = max(bc.best_correlation(x[ch], burst, round(sc["tau"][ch])) for ch in range(bc.E2E_NCH))
    print("correlation with the burst: beam %.4f, best single channel %.4f" % (got, single))
    assert got > single
