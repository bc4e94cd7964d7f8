"""The f-k mask designs, the closed-form fold, the self-designing fk_filt, the Gaussian blur and the small helpers of
design.hip on gfx950 at the cases of tests/design_cases.py -- odd shapes, band edges that move the column loops, grid points
exactly on a speed edge, the blur around its switch to the overlap-save form -- against the float64 oracle
(tests/test_oracle_design_edges.py pins it to the real reference bit for bit; tests/test_emu_design_edges.py runs the same
cases on the CPU build of the kernels)."""
import numpy as np
import pytest
import torch

from oracle import d4w_oracle as orc
from tests import design_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available()
    import das4whales_amd as dw_
    return dw_


@pytest.fixture(scope="module")
def lib(dw):
    from das4whales_amd import _device as dev
    from das4whales_amd._lib import check, lib as lib_
    return lib_, check, dev


# ---- a. every design at every case ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(dc.CASES))
def test_designs_vs_oracle(dw, case):
    shape = dc.CASES[case][0]
    if case in dc.TIE_CASES:
        assert dc.tie_counts(case) == dc.TIE_COUNTS[case] and min(dc.tie_counts(case)) > 0     # a tie case has ties
    for name in dc.DESIGNS:
        if not dc.has_design(case, name):
            with pytest.raises(ValueError, match="even number of time samples"):
                dc.call(dw.dsp, name, case)
            continue
        mask = dc.call(dw.dsp, name, case)
        m = np.asarray(mask) if name == "classic" else mask.todense()
        ref = dc.oracle(case, name)
        assert m.shape == shape == mask.shape and m.dtype == np.float64
        e = float(np.max(np.abs(m - ref)))
        print("%s %s: max abs err %.3e" % (case, name, e))
        assert e < dc.BOUNDS[name], (case, name, e)
        if case in dc.EDGE_CASES and name in dc.CLOSED:
            wrong, left_out, points = dc.sides_agree(m, ref)
            assert left_out <= 0.01 * points                    # (the oracle alone: tests/test_oracle_design_edges.py)
            assert wrong == 0, (case, name, wrong)
        # sparse.COO duck typing (tools.disp_comprate, fk_filter_sparsefilt)
        assert mask.nnz == np.count_nonzero(mask.todense()) and len(mask.data) == mask.nnz and mask.data.ndim == 1


# ---- b. closed form into the plan == dense mask into the plan ---------------------------------------------------------------
def fold_both_ways(dw, case, opts, name, eps):
    shape = dc.get(case)[0]
    x = torch.from_numpy(dc.fold_block(shape)).cuda()
    plan = dw.dsp.FkPlan(shape[0], shape[1], opts=opts)
    designed = dc.call(dw.dsp, name, case)
    assert isinstance(designed, dw.dsp.DesignedMask) and designed._tensor is None
    plan.set_mask(designed, prune_eps=eps)
    assert designed._tensor is None                             # folded from the closed form: still no dense mask
    y1, live1, order1 = plan.apply(x), plan.live_rows(), plan.order()["order"]
    plan.set_mask(designed.tensor, prune_eps=eps)
    y2, live2, order2 = plan.apply(x), plan.live_rows(), plan.order()["order"]
    assert torch.equal(y1, y2), (case, opts, name, eps)
    assert live1 == live2 and order1 == order2
    e = dc.rel(y1.cpu().numpy(), orc.fk_filter_filt(x.cpu().numpy(), dc.oracle(case, name)))
    print("%s %s %s eps %g: %s, %d live rows, rel err %.2e" % (case, opts, name, eps, order1, live1, e))
    assert e < 1e-5, (case, opts, name, eps, e)
    return order1


@pytest.mark.parametrize("case,opts", dc.FOLDS)
def test_closed_form_fold_equals_dense_fold(dw, case, opts):
    for name, eps in dc.FOLD_MODES:
        fold_both_ways(dw, case, opts, name, eps)


def test_fold_covers_both_pass_orders(dw):
    """The 130 x 600 case has shape-specialised kernels (built with the package): with the scripts' hybrid_ninf mask the plan
    runs the time phase first; the same mask on a shape without them (63 x 400) keeps the channel-first order."""
    from das4whales_amd import fkjit
    assert fkjit.is_specialised(*dc.CASES["wide"][0]), "build() compiles the 130 x 600 kernels"
    assert fold_both_ways(dw, "wide", None, "ninf", 0.0) == "time-first"
    assert fold_both_ways(dw, "low_band", None, "ninf", 0.0) == "channel-first"


def test_fold_refuses_the_blurred_designs(dw):
    plan = dw.dsp.FkPlan(18, 48)
    m = dw.dsp.DesignedMask(3, (18, 48), 4 * dc.DX, 1.0 / 200.0, [1350., 1450., 14., 30.], 0, 0)
    with pytest.raises(ValueError, match="closed form"):
        plan.set_mask(m)


# ---- c. fk_filt -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dc.FKFILT_SHAPES)
def test_fk_filt_odd_and_mixed_shapes(dw, shape):
    x = dc.fkfilt_block(shape)
    ref = orc.fk_filt(x, *dc.FKFILT_ARGS)
    y = dw.dsp.fk_filt(x, *dc.FKFILT_ARGS)
    assert isinstance(y, np.ndarray) and y.shape == shape and y.dtype == np.float64
    yt = dw.dsp.fk_filt(torch.from_numpy(x).cuda(), *dc.FKFILT_ARGS)
    assert torch.is_tensor(yt) and yt.is_cuda and tuple(yt.shape) == shape
    e, et = dc.rel(y, ref), dc.rel(yt.cpu().numpy(), ref)
    print("fk_filt %s: rel err %.2e (ndarray), %.2e (CUDA tensor)" % (shape, e, et))
    assert e < 1e-5 and et < 1e-5


@pytest.mark.parametrize("shape", [(40, 480), (41, 480)])
def test_fk_filt_fused_normalisation_equals_separate(dw, lib, shape):
    """d4w_minmax_f32 + the affine fold (FkPlan.set_mask_normalised) against d4w_minmax_normalise_f32 + the plain fold."""
    lib_, check, dev = lib
    nx, ns = shape
    tint, fs, xint, dx, c_min, c_max = dc.FKFILT_ARGS
    x = torch.from_numpy(dc.fkfilt_block(shape).astype(np.float32)).cuda()
    g = dw.dsp._gaussian_filter(dw.dsp._design(5, shape, [0, 0, xint], dx, fs / tint, [c_min, c_max]), 20)
    mm = torch.empty(2, dtype=torch.float32, device="cuda")
    check(lib_.d4w_minmax_f32(dev.ptr(g), g.numel(), dev.ptr(mm), dev.stream_ptr(g)))
    assert float(mm[0]) == float(g.min()) and float(mm[1]) == float(g.max()) and float(mm[1]) > float(mm[0])
    plan = dw.dsp.FkPlan(nx, ns)
    plan.set_mask_normalised(g)
    y1 = plan.apply(x)
    gn = g.clone()
    check(lib_.d4w_minmax_normalise_f32(dev.ptr(gn), gn.numel(), dev.stream_ptr(gn)))
    assert abs(float(gn.min())) < 1e-6 and abs(float(gn.max()) - 1.0) < 1e-6
    plan.set_mask(gn)
    y2 = plan.apply(x)
    assert torch.equal(y1, y2)
    assert dc.rel(y1.cpu().numpy(), orc.fk_filt(x.cpu().numpy(), *dc.FKFILT_ARGS)) < 1e-5


@pytest.mark.parametrize("shape", [(2, 4), (1, 4), (2, 5)])
def test_fk_filt_constant_mask(dw, shape):
    """NaN wherever the reference's is.  1 x 4 (the one wavenumber is 0: both wedges are equal) and the reference's own
    2 x 5 give a wedge of zeros, (g - min) / (max - min) is 0 / 0: NaN everywhere, through the fused normalisation of the
    even path and through d4w_minmax_normalise_f32 of the odd one.  At 2 x 4 the sigma-20 blur of the two wedge points
    wraps the 2 x 4 grid twenty times and is flat to 5.4e-6 around 0.25, not constant: a finite result in both."""
    x = np.random.default_rng(24).standard_normal(shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = orc.fk_filt(x, *dc.FKFILT_ARGS)
    assert bool(np.all(np.isnan(ref))) == (shape != (2, 4)) and bool(np.any(np.isnan(ref))) == (shape != (2, 4))
    got = dw.dsp.fk_filt(x, *dc.FKFILT_ARGS)
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))


# ---- d. the blur alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dc.BLUR_SHAPES)
def test_blur_alone(dw, shape):
    x = torch.from_numpy(dc.blur_input(shape)).cuda()
    for sigma in dc.BLUR_SIGMAS:
        y = dw.dsp._gaussian_filter(x, sigma).cpu().numpy()
        e = float(np.max(np.abs(y - dc.blur_reference(shape, sigma))))
        print("%s sigma %g: max abs err %.3e" % (shape, sigma, e))
        assert e < dc.BLUR_BOUND, (shape, sigma, e)


def test_blur_refuses_a_radius_it_cannot_carry(dw):
    with pytest.raises(ValueError, match="needs radius 129"):
        dw.dsp._gaussian_filter(torch.from_numpy(dc.blur_input((5, 3))).cuda(), 32.2)


def test_blur_form_switches_at_2048_columns(dw):
    """An impulse under the sigma-3 blur (radius 12).  The LDS kernel sums tap x sample products: exact zeros wherever no tap
    meets the impulse.  The overlap-save form leaves the rounding of its transforms in the block that holds the impulse.
    Both are within the bound; which one ran shows in the zeros."""
    from scipy import ndimage
    for ns, fft in ((2047, False), (2048, True)):
        x = np.zeros((30, ns), dtype=np.float32)
        x[15, 1000] = 1.0
        y = dw.dsp._gaussian_filter(torch.from_numpy(x).cuda(), 3.0).cpu().numpy()
        assert np.max(np.abs(y - ndimage.gaussian_filter(x.astype(np.float64), 3.0))) < dc.BLUR_BOUND
        far = y[:, np.abs(np.arange(ns) - 1000) > 12]
        assert bool(np.any(far != 0)) == fft, (ns, float(np.max(np.abs(far))))


def test_blur_back_to_back_with_other_taps_on_one_stream(dw):
    """The overlap-save form keeps one tap vector per device and re-uploads it when sigma changes: sigma 20, 3, 20 queued
    on one stream without a synchronisation in between."""
    shape = (30, 2049)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        x = torch.from_numpy(dc.blur_input(shape)).cuda()
        ys = [dw.dsp._gaussian_filter(x, s) for s in (20.0, 3.0, 20.0)]
    st.synchronize()
    for y, s in zip(ys, (20.0, 3.0, 20.0)):
        assert float(np.max(np.abs(y.cpu().numpy() - dc.blur_reference(shape, s)))) < dc.BLUR_BOUND, s
    assert torch.equal(ys[0], ys[2])


# ---- e. flip sum and taper --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dc.FLIP_SHAPES)
def test_flip_sum(dw, lib, shape):
    lib_, check, dev = lib
    m = (np.random.default_rng(shape[0] + shape[1]).random(shape) * 3 - 1).astype(np.float32)
    t = torch.from_numpy(m).cuda()
    out = torch.empty_like(t)
    check(lib_.d4w_flip_sum_f32(dev.ptr(t), dev.ptr(out), shape[0], shape[1], dev.stream_ptr(t)))
    assert np.array_equal(out.cpu().numpy(), dc.flip_sum_reference(m))


@pytest.mark.parametrize("ns", dc.TAPER_NS)
def test_taper_data(dw, ns):
    x = np.random.default_rng(ns).standard_normal((3, ns)) + 2.0
    ref = orc.taper_data(x)
    a = x.copy()
    assert dw.dsp.taper_data(a) is a                             # in place, like the reference
    assert np.max(np.abs(a - ref)) <= 1e-6 * np.max(np.abs(ref))
    t = torch.from_numpy(x.astype(np.float32)).cuda()
    v = t._version
    assert dw.dsp.taper_data(t) is t and t._version > v
    assert np.max(np.abs(t.cpu().numpy() - ref)) <= 1e-6 * np.max(np.abs(ref))
