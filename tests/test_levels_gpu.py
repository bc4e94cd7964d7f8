"""GPU tests of the received levels (csrc/levels.hip) through das4whales_amd.loc.received_levels, with NumPy input and with CUDA
tensor input.  The cases and the exact answers are those of tests/levels_cases.py, which the CPU emulator runs as well
(tests/test_emu_levels.py); the reference is the float64 restatement of tests/known_answers_levels.py.

Tolerance, derived: |signal - ref| <= (L + 8) 2^-24 ref and |noise - ref| <= (N + 8) 2^-24 ref; peak exactly; NaN exactly where
the definition says; entries whose reference is 0 exactly 0.  No case is skipped or excluded.

Measured on an MI355X: worst error / tolerance of signal and noise over the parity cases 0.101.  End to end
(test_end_to_end_spreading_law): restatement k = 1.999999999 and SL within 4.8e-8 dB of the known answer; device
|k - k_ref| = 1.4e-8 against a bound of 6.3e-6 and |SL - SL_ref| = 5.5e-7 dB against 2.7e-4.
"""
import numpy as np
import pytest
import torch

from tests import known_answers_beam as kb
from tests import known_answers_levels as kl
from tests import levels_cases as lc
from tests.known_answers_loc import C0, make_cable

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available()
    import das4whales_amd as dw
    return dw


@pytest.fixture(scope="module")
def W(dw):
    return dw.loc.level_limits()[2]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_run(dw, container="tensor"):
    """The runner of levels_cases on dw.loc.received_levels.  "tensor": the buffers go to the device as they are and the block is
    a column-sliced view of them, read in place through its pitch; "numpy": the block is handed over as a NumPy array."""
    def run(buf, ns, nxt, ns2, r, start, L, gap, N, weights):
        nch = buf.shape[0]
        cable = make_cable("line", max(nch, 2))[:nch]        # not used: the table is given
        pos = np.zeros((r.shape[0], 3))
        if container == "tensor":
            x = cuda(buf)[:, :ns]
            b = cuda(nxt)[:, :ns2] if nxt is not None else None
            out = dw.loc.received_levels(x, lc.FS, cable, C0, pos, cuda(start), L, N, gap, cuda(weights) if weights is not None else None, b,
                                         delays=cuda(r))
            assert all(isinstance(o, torch.Tensor) and o.is_cuda and o.dtype == torch.float32 for o in out)
            return tuple(o.cpu().numpy() for o in out)
        out = dw.loc.received_levels(buf[:, :ns], lc.FS, cable, C0, pos, start, L, N, gap, weights, nxt[:, :ns2] if nxt is not None else None,
                                     delays=r)
        assert all(isinstance(o, np.ndarray) for o in out)
        return out
    return run


def test_limits(dw):
    max_calls, max_length, W = dw.loc.level_limits()
    assert max_calls >= 64 and max_length >= 1 << 20 and W >= 2


@pytest.mark.parametrize("case", lc.parity_cases(), ids=lc.case_id)
def test_parity(dw, W, case):
    lc.check_parity(gpu_run(dw, "tensor" if case[10] % 2 else "numpy"), case, W)


@pytest.mark.parametrize("case", lc.parity_cases()[::3], ids=lc.case_id)
def test_poison(dw, W, case):
    lc.check_poison(gpu_run(dw, "numpy" if case[10] % 2 else "tensor"), case, W)


def test_integer_samples(dw, W):
    lc.check_integers(gpu_run(dw), W)


def test_zero_block_and_ones(dw, W):
    lc.check_zeros_and_ones(gpu_run(dw, "numpy"), W)


def test_nan_rows_and_samples(dw, W):
    lc.check_nan_rows(gpu_run(dw), W)


def test_bit_identity(dw, W):
    lc.check_bit_identity(gpu_run(dw), W)
    lc.check_bit_identity(gpu_run(dw, "numpy"), W)


def test_split_is_the_concatenation(dw, W):
    lc.check_split(gpu_run(dw), W)
    lc.check_split(gpu_run(dw, "numpy"), W)


def test_delays_given_against_built_inside_and_containers(dw, W):
    """delays= given and built inside: the same bits; NumPy in -> NumPy out, tensors in -> tensors on the caller's stream; one
    call given as a vector; no call, no launch."""
    nch, ns, L, N, gap, fs = 2 * W + 3, 900, 65, 64, 3, 50.0
    rng = np.random.default_rng(9)
    cable = make_cable("bent", nch)
    pos = cable[[1, nch // 2, nch - 2]] + np.array([300.0, -200.0, 50.0])
    x = rng.standard_normal((nch, ns)).astype(np.float32)
    r = dw.loc.beam_delays(cable, C0, fs, pos, rounded=True)
    assert np.array_equal(r, kb.rounded(kb.tau(cable, C0, fs, pos)))
    start = (np.array([100, 0, 400]) - np.median(r, axis=1).astype(np.int64))
    inside = dw.loc.received_levels(x, fs, cable, C0, pos, start, L, N, gap)
    given = dw.loc.received_levels(x, fs, cable, C0, pos, start, L, N, gap, delays=r)
    assert all(isinstance(o, np.ndarray) for o in inside) and all(kl.same(a, b) for a, b in zip(inside, given))
    ref = kl.levels_ref(x, r, start, L, gap, N)
    assert ref.valid_signal.any() and not ref.valid_noise.all() and kl.worst_ratio(inside, ref) <= 1.0
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                            # a stream of the caller's: the work is ordered on it
        xt = cuda(x) * 8.0
        out = dw.loc.received_levels(xt, fs, cable, C0, cuda(pos), cuda(start), L, N, gap)
        sig = out[0] * (1.0 / 64.0)
    side.synchronize()
    assert all(o.is_cuda and o.dtype == torch.float32 for o in out) and kl.same(sig.cpu().numpy(), inside[0])
    one = dw.loc.received_levels(x, fs, cable, C0, pos[1], int(start[1]), L, N, gap)
    assert one[0].shape == (1, nch) and all(kl.same(a[0], b[1]) for a, b in zip(one, inside))
    none = dw.loc.received_levels(x, fs, cable, C0, np.zeros((0, 3)), 0, L, N, gap)
    assert [o.shape for o in none] == [(0, nch)] * 3 and all(o.dtype == np.float32 for o in none)
    bare = dw.loc.received_levels(x, fs, cable, C0, pos, start, L)
    assert np.all(np.isnan(bare[1])) and kl.same(bare[0], inside[0]) and kl.same(bare[2], inside[2])
    lev, snr = dw.loc.levels_db(out[0], out[1])              # tensors on the device stay there
    assert lev.is_cuda and snr.is_cuda and lev.dtype == torch.float64
    host = dw.loc.levels_db(inside[0], inside[1])
    assert np.allclose(snr.cpu().numpy(), host[1], rtol=0, atol=1e-9, equal_nan=True)


def test_end_to_end_spreading_law(dw):
    """One call 300 m east and 2000 m south of channel 33 of the 67-channel line cable, at z = -30: every row is zero except
    float32(burst 4096 / range) at 20 + r[ch], burst 65 integers in [-15, 15].  received_levels (table built inside) -> levels_db ->
    fit_spreading gives k = 2 and SL = 10 log10(mean(burst^2) 4096^2).  The float64 restatement of the scene meets both to 1e-6;
    the device stays within the slope and intercept perturbations of a least-squares line under errors of at most
    delta = (10 / ln 10) (L + 8) 2^-24 dB per point: |k - k_ref| <= delta / std(u), |SL - SL_ref| <= delta (1 + |mean(u)| / std(u)),
    u = 10 log10(range)."""
    nch, fs, L, first = 67, 200.0, 65, 20
    cable = make_cable("line", nch)
    pos = np.array([cable[33, 0] + 300.0, cable[33, 1] - 2000.0, -30.0])
    rng = np.random.default_rng(2024)
    burst = rng.integers(-15, 16, L).astype(np.float64)
    rge = np.sqrt(((cable - pos) ** 2).sum(1))
    r = kb.rounded(kb.tau(cable, C0, fs, pos[None, :]))
    ns = first + int(r.max()) + L + 7
    x = np.zeros((nch, ns), dtype=np.float32)
    for ch in range(nch):
        x[ch, first + r[0, ch]:first + r[0, ch] + L] = (burst * 4096.0 / rge[ch]).astype(np.float32)
    u = 10.0 * np.log10(rge)
    SL_true = 10.0 * np.log10(np.mean(burst ** 2) * 4096.0 ** 2)
    # the float64 restatement of the scene, fitted by NumPy's own least squares
    ref = kl.levels_ref(x, r, np.array([first]), L, 0, 0)
    assert ref.valid_signal.all()
    slope, icpt = np.polyfit(u, 10.0 * np.log10(ref.signal[0]), 1)
    k_ref, SL_ref = -slope, icpt
    print("restatement: k = %.9f, SL = %.9f (true %.9f)" % (k_ref, SL_ref, SL_true))
    assert abs(k_ref - 2.0) < 1e-6 and abs(SL_ref - SL_true) < 1e-6
    sig, noi, pk = dw.loc.received_levels(x, fs, cable, C0, pos, first, length=L)
    assert np.all(np.isnan(noi)) and kl.same(pk, ref.peak.astype(np.float32))
    lev = dw.loc.levels_db(sig)
    SL, k, used = dw.loc.fit_spreading(lev, cable, pos)
    delta = (10.0 / np.log(10.0)) * (L + 8) * 2.0 ** -24
    dk, dSL = abs(k[0] - k_ref), abs(SL[0] - SL_ref)
    print("device: k = %.9f (|k - k_ref| = %.3g, bound %.3g), SL = %.9f (|SL - SL_ref| = %.3g, bound %.3g)"
          % (k[0], dk, delta / np.std(u), SL[0], dSL, delta * (1 + abs(np.mean(u)) / np.std(u))))
    assert used.dtype == np.int32 and used[0] == 67
    assert dk <= delta / np.std(u)
    assert dSL <= delta * (1.0 + abs(np.mean(u)) / np.std(u))


def test_bad_arguments(dw):
    nch, ns = 5, 64
    base = dict(trace=np.ones((nch, ns), dtype=np.float32), fs=50.0, cable_pos=make_cable("line", nch), c0=C0, pos=np.zeros((2, 3)),
                start=np.zeros(2, dtype=np.int64), length=8)
    assert dw.loc.received_levels(**base)[0].shape == (2, nch)
    for kw in (dict(length=0), dict(length=1.5), dict(noise_length=-1), dict(gap=-1), dict(gap=0.5), dict(start=1.5),
               dict(delays=np.zeros((2, nch), dtype=np.int64)), dict(delays=np.zeros((2, nch - 1), dtype=np.int32)), dict(fs=0.0),
               dict(weights=np.ones(4)), dict(next_block=np.ones((4, 9), dtype=np.float32)), dict(pos=np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            dw.loc.received_levels(**dict(base, **kw))
