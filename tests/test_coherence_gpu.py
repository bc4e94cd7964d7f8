"""GPU tests of the coherence of located calls (csrc/coherence.hip) through das4whales_amd.loc: beam_coherence and
beamform_pws, with NumPy input and with CUDA tensor input.  The cases and the exact answers are those of
tests/coherence_cases.py, which the CPU emulator runs as well (tests/test_emu_coherence.py); the reference is the float64
restatement of tests/known_answers_coherence.py, with its derived tolerances (semblance: <= 1e-4 on every element).
"""
import numpy as np
import pytest
import torch

from tests import coherence_cases as cc
from tests.known_answers_loc import C0, make_cable

pytestmark = pytest.mark.gpu
FS = cc.FS                                                   # the runners hand the delay table over: the rate only scales the times


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available()
    import das4whales_amd as dw
    return dw


@pytest.fixture(scope="module")
def Hmax(dw):
    return dw.loc.coherence_limits()[2]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _geometry(delays, order, nch):
    cable = make_cable("line", max(nch, 2))[:nch]            # not used: the table is given
    return cable, np.zeros(((delays if order == 0 else delays[0]).shape[0], 3))


def gpu_run(dw, container="tensor"):
    """The runner of coherence_cases on dw.loc.beam_coherence.  "tensor": the buffers go to the device as they are and the
    blocks are column-sliced views of them, read in place through their pitch; "numpy": NumPy arrays in, NumPy arrays out."""
    def run(buf, ns, nxt, ns2, ibuf, inxt, delays, order, weights, start, nt, H, peak_range=None):
        cable, pos = _geometry(delays, order, buf.shape[0])
        if container == "tensor":
            view = lambda a, n: cuda(a)[:, :n] if a is not None else None
            d = cuda(delays) if order == 0 else tuple(cuda(a) for a in delays)
            r = dw.loc.beam_coherence(view(buf, ns), FS, cable, C0, pos, start=cuda(start), length=nt, half_window=H, order=order,
                                      weights=cuda(weights) if weights is not None else None, next_block=view(nxt, ns2), imag=view(ibuf, ns),
                                      next_imag=view(inxt, ns2), peak_range=peak_range, delays=d)
            for name, dtype in (("beam", torch.float32), ("semblance", torch.float32), ("wsum", torch.float32), ("times", torch.float64),
                                ("peak", torch.float32), ("peak_index", torch.int32)) + ((("phase", torch.float32),) if ibuf is not None else ()):
                y = getattr(r, name)
                assert isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == dtype, name
            out = {k: (v.cpu().numpy() if v is not None else None) for k, v in r._asdict().items()}
        else:
            cut = lambda a, n: a[:, :n] if a is not None else None
            r = dw.loc.beam_coherence(cut(buf, ns), FS, cable, C0, pos, start=start, length=nt, half_window=H, order=order, weights=weights,
                                      next_block=cut(nxt, ns2), imag=cut(ibuf, ns), next_imag=cut(inxt, ns2), peak_range=peak_range, delays=delays)
            out = r._asdict()
            assert all(isinstance(v, np.ndarray) for v in out.values() if v is not None)
        assert np.array_equal(out["times"], (np.asarray(start)[:, None] + np.arange(nt)[None, :]) / FS)
        return out
    return run


def gpu_beam(dw):
    def run(buf, ns, nxt, ns2, delays, order, weights, start, nt, normalize):
        cable, pos = _geometry(delays, order, buf.shape[0])
        return dw.loc.beamform(buf[:, :ns], FS, cable, C0, pos, start=start, length=nt, order=order, weights=weights, normalize=normalize,
                               next_block=nxt[:, :ns2] if nxt is not None else None, delays=delays)[0]
    return run


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_parity(dw, Hmax, case):
    cc.check_parity(gpu_run(dw, "numpy" if cc.CASES.index(case) % 3 == 0 else "tensor"), gpu_beam(dw), case, Hmax)


def test_exact_one(dw):
    cc.check_exact_one(gpu_run(dw))


def test_exact_zero(dw):
    cc.check_exact_zero(gpu_run(dw, "numpy"))


def test_phase_one(dw):
    cc.check_phase_one(gpu_run(dw), dw.loc.coherence_limits()[3])


def test_bit_identity(dw, Hmax):
    cc.check_bit_identity(gpu_run(dw), Hmax)


def test_next_block_is_the_concatenation(dw, Hmax):
    cc.check_next_block(gpu_run(dw), Hmax)
    cc.check_next_block(gpu_run(dw, "numpy"), Hmax)


def test_peak_range(dw):
    cc.check_peak_range(gpu_run(dw))


def test_imag_true_is_hilbert_imag_passed_explicitly_and_delays_built_inside(dw):
    """imag=True forms dsp.hilbert_imag of each block here: the same bits as passing it; delays built inside: the same bits as
    given; a stream of the caller's; one position as a vector; no call: no launch."""
    sc = cc.scene()
    x, nb = sc["x"][:, :2500], sc["x"][:, 2500:]
    cable, pos = sc["cable"], sc["pos"]
    start = np.array([2300, 2200])                           # the moveouts cross into the next block
    args = dict(start=start, length=400, half_window=20, order=3, next_block=nb)
    hx, hnb = dw.dsp.hilbert_imag(x), dw.dsp.hilbert_imag(nb)
    a = dw.loc.beam_coherence(x, cc.SCENE_FS, cable, C0, pos, imag=True, **args)
    b = dw.loc.beam_coherence(x, cc.SCENE_FS, cable, C0, pos, imag=hx, next_imag=hnb, delays=dw.loc.beam_delays(cable, C0, cc.SCENE_FS, pos), **args)
    assert a.phase.any() and a.semblance.any() and a.phase.max() <= 1.0 + 1e-4
    for name in cc_fields():
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = dw.loc.beam_coherence(cuda(x), cc.SCENE_FS, cable, C0, cuda(pos), start=cuda(start), length=400, half_window=20, order=3,
                                  next_block=cuda(nb), imag=True)
    side.synchronize()
    for name in cc_fields():
        assert getattr(t, name).is_cuda and np.array_equal(getattr(t, name).cpu().numpy(), getattr(a, name)), name
    one = dw.loc.beam_coherence(x, cc.SCENE_FS, cable, C0, pos[1], start=2200, length=400, half_window=20, order=3, next_block=nb, imag=True)
    assert one.semblance.shape == (1, 400) and np.array_equal(one.semblance[0], a.semblance[1]) and one.peak[0] == a.peak[1]
    none = dw.loc.beam_coherence(x, cc.SCENE_FS, cable, C0, np.zeros((0, 3)), length=7)
    assert none.beam.shape == (0, 7) and none.semblance.dtype == np.float32 and none.phase is None and none.peak.shape == (0,)
    assert none.peak_index.dtype == np.int32 and none.times.shape == (0, 7)


def cc_fields():
    return ("beam", "semblance", "phase", "wsum", "times", "peak", "peak_index")


def test_bad_weights_in_a_device_tensor_are_refused_before_any_launch(dw):
    x = np.ones((5, 64), dtype=np.float32)
    cable = make_cable("line", 5)
    for w in ([1, 1, -1, 1, 1], [1, float("nan"), 1, 1, 1], [1, 1, 1, 1, float("inf")]):
        with pytest.raises(ValueError):
            dw.loc.beam_coherence(x, 50.0, cable, C0, np.zeros((1, 3)), weights=torch.tensor(w, dtype=torch.float32).cuda())


def test_peak_separates_the_call_from_a_louder_decoy(dw):
    """The decoy beams louder than the call and the semblance still tells them apart, by the margin the restatement shows."""
    sc, ref = cc.scene(), cc.scene_reference()
    r = dw.loc.beam_coherence(sc["x"], cc.SCENE_FS, sc["cable"], C0, sc["pos"], start=np.array(cc.SCENE_STARTS), length=cc.SCENE_NT,
                              half_window=cc.SCENE_H, order=3, imag=sc["imag"])
    g = ref["gate"]
    for name in ("beam", "semblance", "phase", "wsum"):
        assert cc.within(getattr(r, name), g[name], g["tol_" + name]) <= 1.0, name
    energy = (r.beam.astype(np.float64) ** 2).sum(axis=1)
    print("beam energy %s, semblance peaks %s (restatement %s)" % (energy, r.peak, ref["peaks"]))
    assert energy[1] >= energy[0]
    assert r.peak[0] > r.peak[1]
    assert np.all(np.abs(r.peak - ref["peaks"]) <= g["tol_semblance"].max() + 2.0 ** -24)
    thr = 0.5 * (ref["peaks"][0] + ref["peaks"][1])
    assert list(r.peak >= thr) == [True, False]              # the gate of INTEGRATION.md


def test_phase_weighted_stack_is_closer_to_the_clean_call_than_the_linear_beam(dw):
    sc, ref = cc.scene(), cc.scene_reference()
    args = (sc["x"], cc.SCENE_FS, sc["cable"], C0, sc["pos"][0])
    pws, times = dw.loc.beamform_pws(*args, start=0, length=cc.SCENE_LONG, order=3, imag=sc["imag"])
    lin, _ = dw.loc.beamform(*args, start=0, length=cc.SCENE_LONG, order=3, normalize=True)
    assert pws.dtype == np.float32 and pws.shape == (1, cc.SCENE_LONG) and np.array_equal(times, np.arange(cc.SCENE_LONG)[None, :] / cc.SCENE_FS)
    assert cc.within(pws, ref["pws"], ref["tol_pws"]) <= 1.0 and cc.within(lin, ref["lin"], ref["dlin"]) <= 1.0
    err_lin, err_pws = ((lin - ref["clean"]) ** 2).sum(), ((pws - ref["clean"]) ** 2).sum()
    print("error energy against the clean call: linear %.2f, phase-weighted %.2f (restatement %.2f, %.2f)" % (err_lin, err_pws, ref["err_lin"], ref["err_pws"]))
    assert err_pws < err_lin
    # power = 0 is the normalized beam, and tensors in give tensors out
    p0, _ = dw.loc.beamform_pws(*args, start=0, length=cc.SCENE_LONG, power=0.0, order=3, imag=sc["imag"])
    assert np.array_equal(p0, lin)
    pt, tt = dw.loc.beamform_pws(cuda(sc["x"]), cc.SCENE_FS, sc["cable"], C0, sc["pos"][0], start=0, length=cc.SCENE_LONG, order=3, imag=cuda(sc["imag"]))
    assert pt.is_cuda and tt.is_cuda and np.array_equal(pt.cpu().numpy(), pws)
