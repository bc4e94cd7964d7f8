"""GPU tests of the window-normalised matched filter: d4w_nmf_normalise_f32 alone through the C ABI, detect.compute_nmf_correlograms
with NumPy and with CUDA tensor input, and stream.FileStream(nmf=True) -- the cases of tests/nmf_cases.py (which
tests/test_emu_nmf.py runs on the CPU emulator build) against the float64 restatement of tests/known_answers_nmf.py.
Bounds: derived there (float32 samples, float32 final scale), plus the correlator's own parity tolerance for the public call."""
import numpy as np
import pytest
import torch

from tests import known_answers_nmf as kn
from tests import nmf_cases as nc

pytestmark = pytest.mark.gpu
CONTAINERS = ("numpy", "tensor")


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available()
    import das4whales_amd as dw
    return dw


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_kernel(dw, x, head, n_next, mean, mx, cs, ms, norms, center, floor, want_max):
    from das4whales_amd._lib import lib, check
    nx, ns = x.shape
    xd, md, ad = cuda(x), cuda(np.asarray(mean, dtype=np.float64)), cuda(np.asarray(mx, dtype=np.float32))
    hd = cuda(head) if head is not None else None
    outs = [cuda(c) for c in cs]
    rmax = [torch.full((nx,), float("nan"), dtype=torch.float32, device="cuda") for _ in cs] if want_max else None
    check(lib.d4w_nmf_normalise_f32(xd.data_ptr(), nx, ns, hd.data_ptr() if hd is not None else None, hd.shape[1] if hd is not None else 0,
                                    n_next, md.data_ptr(), ad.data_ptr(), len(ms), ms[0], ms[-1], norms[0], norms[-1], int(center), floor,
                                    outs[0].data_ptr(), outs[1].data_ptr() if len(outs) > 1 else None,
                                    rmax[0].data_ptr() if rmax else None, rmax[1].data_ptr() if rmax and len(rmax) > 1 else None,
                                    torch.cuda.current_stream().cuda_stream))
    return [o.cpu().numpy() for o in outs], ([r.cpu().numpy() for r in rmax] if rmax else None)


def gpu_public(dw, container, x, templates, center, floor, head):
    if container == "tensor":
        got = dw.detect.compute_nmf_correlograms(cuda(x), templates, center=center, floor=floor, next_head=cuda(head) if head is not None else None)
        assert all(isinstance(g, torch.Tensor) and g.is_cuda for g in got)
        return [g.cpu().numpy() for g in got]
    got = dw.detect.compute_nmf_correlograms(x, templates, center=center, floor=floor, next_head=head)
    assert all(isinstance(g, np.ndarray) for g in got)
    return got


def test_constants(dw):
    from das4whales_amd._lib import lib
    assert lib.d4w_nmf_tile() == kn.TILE
    assert lib.d4w_nmf_max_support() == nc.MAX_SUPPORT >= lib.d4w_xcorr_mm_max_support()


@pytest.mark.parametrize("ns_form", nc.NS_FORMS)
@pytest.mark.parametrize("support", list(nc.SUPPORTS))
def test_kernel_alone(dw, support, ns_form):
    nc.check_kernel_alone(lambda *a: gpu_kernel(dw, *a), support, ns_form)


@pytest.mark.parametrize("container", CONTAINERS)
def test_public_call_on_the_scene(dw, container):
    nc.check_public_on_scene(lambda *a: gpu_public(dw, container, *a))


@pytest.mark.parametrize("container", CONTAINERS)
def test_properties_on_the_scene(dw, container):
    nc.check_properties(lambda *a: gpu_public(dw, container, *a),
                        pick_times=lambda c, thr: dw.detect.pick_times(c, thr),
                        reference_correlogram=lambda x, t: dw.detect.compute_cross_correlogram(x, t))


def test_pair_sits_back_to_back_and_single_call(dw):
    x, head = kn.scene()
    tp = kn.templates()
    hf, lf = dw.detect.compute_nmf_correlograms(cuda(x), [tp["hf"], tp["lf"]], next_head=cuda(head))
    both = dw.detect.stacked_pair(hf, lf)
    assert both is not None and both.shape == (16, kn.NS)
    assert torch.equal(both[:8], hf) and torch.equal(both[8:], lf)
    one = dw.detect.compute_nmf_correlogram(cuda(x), tp["hf"], next_head=cuda(head))
    ref, bound, _, slack = nc.scene_reference("hf")
    assert np.all(np.abs(one.cpu().numpy().astype(np.float64) - ref) <= bound + nc.TOL * slack)
    picks = dw.detect.pick_times_env(hf, 0.6)                # the result goes to the pickers as it is
    assert len(picks) == 8


def test_row_maxima_epilogue(dw):
    x, head = kn.scene()
    tp = kn.templates()
    xd, hd = cuda(x), cuda(head)
    parts = [dw.detect._nmf_parts(tp[k]) for k in ("hf", "lf")]
    outs, rmax = dw.detect._nmf_device(xd, [h for h, _ in parts], [n for _, n in parts], next_head=hd, want_row_max=True)
    for o, r in zip(outs, rmax):
        assert np.array_equal(r.cpu().numpy(), o.cpu().numpy().max(axis=1))
    assert dw.detect.correlogram_max(outs[0], row_max=rmax[0]) == float(outs[0].max())
    thr = dw.detect.Threshold(0.8, dw.detect.correlogram_max(outs[0], row_max=rmax[0], on_device=True))
    assert float(thr) == pytest.approx(0.8 * float(outs[0].max()))


def test_file_stream_nmf(dw):
    """Three files of the scene's shape: every file's result equals compute_nmf_correlograms of its filtered version with the
    next one's head, the last file cut short; the default stream's output is what _matched_filter gives, untouched."""
    x, _ = kn.scene()
    tp = kn.templates()
    rng = np.random.default_rng(70)
    files = [x] + [rng.standard_normal(x.shape).astype(np.float32) * s for s in (1.0, 40.0)]
    files[2][:, :300] += files[0][:, 900:1200]               # something for file 1's last lags to find in file 2's head
    templates = [tp["hf"], tp["lf"]]
    st = dw.stream.FileStream(kn.FS, 14, 30, templates=templates, halo=1024, nmf=True)
    plain = dw.stream.FileStream(kn.FS, 14, 30, templates=templates, halo=1024)
    res, res_plain = [], []
    for f in files:
        res += st.push(f)
        res_plain += plain.push(f)
    res += st.flush()
    res_plain += plain.flush()
    assert [r["index"] for r in res] == [0, 1, 2] == [r["index"] for r in res_plain]
    longest = max(len(kn.support(t)) for t in templates)
    for i, (r, rp) in enumerate(zip(res, res_plain)):
        assert "correlograms" not in r and "nmf" not in rp
        assert torch.equal(r["filtered"], rp["filtered"])
        nxt = res[i + 1]["filtered"][:, :longest - 1] if i + 1 < len(res) else None
        want = dw.detect.compute_nmf_correlograms(r["filtered"], templates, next_head=nxt)
        for got, w, rm in zip(r["nmf"], want, r["row_max"]):
            assert torch.equal(got, w)
            assert torch.equal(rm, got.max(dim=1).values)
        taps = [dw.detect._normalised_support(t) for t in templates]
        tails = [dw.detect._tail_coef(t) for t in templates]
        was, was_max = dw.detect._matched_filter(rp["filtered"], taps, tails, next_head=res_plain[i + 1]["filtered"] if i + 1 < len(res) else None,
                                                 want_row_max=True)
        for got, w, rm, wm in zip(rp["correlograms"], was, rp["row_max"], was_max):
            assert torch.equal(got, w) and torch.equal(rm, wm)
    # the call at the end of file 0's row 7 is completed from file 1 ... by noise here: what matters is that the last lags differ
    cut = dw.detect.compute_nmf_correlograms(res[0]["filtered"], templates)
    assert not torch.equal(cut[0][:, -longest:], res[0]["nmf"][0][:, -longest:])
    opts = dw.stream.FileStream(kn.FS, 14, 30, templates=templates, nmf={"center": False, "floor": 1e-5})
    assert opts.nmf == {"center": False, "floor": 1e-5}
    with pytest.raises(ValueError):
        dw.stream.FileStream(kn.FS, 14, 30, templates=templates, nmf={"centre": False})
