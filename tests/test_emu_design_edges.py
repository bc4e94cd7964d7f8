"""The cases of tests/design_cases.py on the CPU emulator build of design.hip / design_eval.h / the closed-form fold of
fk_filter.hip (fk_dist.hip for the slab fold), against the float64 oracle: what tests/test_design_edges_gpu.py runs on gfx950, so that a failure there can
be told from a failure of the C code."""
import ctypes

import numpy as np
import pytest

from oracle import d4w_oracle as orc
from tests import design_cases as dc
from tests.emu_util import load_emu, vp

cv, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double


@pytest.fixture(scope="module")
def emu():
    lib = load_emu()
    lib.d4w_design_mask_f32.argtypes = [ci, ci, ci, cd, cd, cv, ci, ci, cv, cv, cv]
    lib.d4w_gaussian_filter_f32.argtypes = [cv, cv, cv, ci, ci, cd, cv]
    lib.d4w_flip_sum_f32.argtypes = [cv, cv, ci, ci, cv]
    lib.d4w_fk_set_mask_design_f32.argtypes = [cv, ci, cd, cd, cv, ci, ci, cv, cd, cv]
    lib.d4w_fk_set_mask_dense_pruned_f32.argtypes = [cv, cv, cd, cv]
    return lib


def dense(lib, shape, mode, step, dt, params, i0, i1, hrow):
    out = np.empty(shape, dtype=np.float32)
    p8 = np.zeros(8)
    p8[:len(params)] = params
    rc = lib.d4w_design_mask_f32(mode, shape[0], shape[1], step, dt, vp(p8), i0, i1, vp(hrow) if hrow is not None else None,
                                 vp(out), None)
    assert rc == 0, lib.d4w_last_error()
    return out


def gauss(lib, m, sigma):
    out, tmp = np.empty_like(m), np.empty_like(m)
    rc = lib.d4w_gaussian_filter_f32(vp(m), vp(out), vp(tmp), m.shape[0], m.shape[1], sigma, None)
    return rc, out


def flip_sum(lib, m):
    out = np.empty_like(m)
    assert lib.d4w_flip_sum_f32(vp(m), vp(out), m.shape[0], m.shape[1], None) == 0, lib.d4w_last_error()
    return out


def design(lib, case, name):
    """The whole of a public designer, as dsp.py chains the kernels."""
    m = dense(lib, dc.CASES[case][0], *dc.kernel_args(case, name))
    if name in ("gs", "ninf_gs"):
        rc, m = gauss(lib, m, 20.0)
        assert rc == 0, lib.d4w_last_error()
    return flip_sum(lib, m) if name == "ninf_gs" else m


@pytest.mark.parametrize("case", list(dc.CASES))
def test_designs_vs_oracle(emu, case):
    for name in dc.DESIGNS:
        if not dc.has_design(case, name):
            continue
        m, ref = design(emu, case, name), dc.oracle(case, name)
        e = float(np.max(np.abs(m - ref)))
        print("%s %s: max abs err %.3e" % (case, name, e))
        assert e < dc.BOUNDS[name], (case, name, e)
        if case in dc.EDGE_CASES and name in dc.CLOSED:
            wrong, left_out, points = dc.sides_agree(m, ref)
            assert wrong == 0, (case, name, wrong)


@pytest.mark.parametrize("shape", dc.BLUR_SHAPES)
def test_blur_alone(emu, shape):
    x = dc.blur_input(shape)
    for sigma in dc.BLUR_SIGMAS:
        rc, y = gauss(emu, x, sigma)
        assert rc == 0, emu.d4w_last_error()
        e = float(np.max(np.abs(y - dc.blur_reference(shape, sigma))))
        print("%s sigma %g: max abs err %.3e" % (shape, sigma, e))
        assert e < dc.BLUR_BOUND, (shape, sigma, e)


def test_blur_refuses_a_radius_it_cannot_carry(emu):
    rc, _ = gauss(emu, dc.blur_input((5, 3)), 32.2)             # radius 129 > 128
    assert rc != 0 and b"needs radius 129" in emu.d4w_last_error()


@pytest.mark.parametrize("shape", dc.FLIP_SHAPES)
def test_flip_sum(emu, shape):
    m = (np.random.default_rng(shape[0] + shape[1]).random(shape) * 3 - 1).astype(np.float32)
    assert np.array_equal(flip_sum(emu, m), dc.flip_sum_reference(m))


def fold_both_ways(lib, shape, opts, mode, eps, step, dt, params, i0, i1, hrow):
    """(output with the closed form folded, output with the dense mask folded, live rows of both, pass order of both)"""
    lib.d4w_fk_plan_order.argtypes = [cv, cv, cv]
    x = dc.fold_block(shape)
    mask = dense(lib, shape, mode, step, dt, params, i0, i1, hrow)
    p8 = np.zeros(8)
    p8[:len(params)] = params
    o = (ci * 6)(*opts) if opts else None
    ys, live, order = [], [], []
    for closed in (True, False):
        plan = cv()
        assert lib.d4w_fk_plan_create_ex(shape[0], shape[1], o, ctypes.byref(plan)) == 0, lib.d4w_last_error()
        if closed:
            rc = lib.d4w_fk_set_mask_design_f32(plan, mode, step, dt, vp(p8), i0, i1, vp(hrow) if hrow is not None else None, eps, None)
        else:
            rc = lib.d4w_fk_set_mask_dense_pruned_f32(plan, vp(mask), eps, None)
        assert rc == 0, lib.d4w_last_error()
        y = np.empty_like(x)
        assert lib.d4w_fk_apply_f32(plan, vp(x), vp(y), 0, None) == 0, lib.d4w_last_error()
        info, b = (ci * 6)(), (cd * 2)()
        assert lib.d4w_fk_plan_order(plan, info, b) == 0
        live.append(lib.d4w_fk_plan_live_rows(plan))
        order.append(info[0])
        lib.d4w_fk_plan_destroy(plan)
        ys.append(y)
    return x, ys, live, order


@pytest.mark.parametrize("case,opts", dc.FOLDS)
def test_closed_form_fold_equals_dense_fold(emu, case, opts):
    shape = dc.get(case)[0]
    for name, eps in dc.FOLD_MODES:
        mode = dc.kernel_args(case, name)[0]
        x, ys, live, order = fold_both_ways(emu, shape, opts, mode, eps, *dc.kernel_args(case, name)[1:])
        assert np.array_equal(ys[0], ys[1]), (case, mode, eps)
        assert live[0] == live[1] and order[0] == order[1]
        e = dc.rel(ys[0], orc.fk_filter_filt(x, dc.oracle(case, name)))
        print("%s %s %s eps %g: %s, %d live rows, rel err %.2e" % (case, opts, name, eps, "time-first" if order[0] else "channel-first",
                                                                  live[0], e))
        assert e < 1e-5, (case, name, eps, e)


def test_blur_form_switches_at_2048_columns(emu):
    """An impulse under the sigma-3 blur (radius 12).  The LDS kernel sums tap x sample products: exact zeros wherever no tap
    meets the impulse.  The overlap-save form leaves the rounding of its transforms in the block that holds the impulse.
    Both are within the bound; which one ran shows in the zeros."""
    for ns, fft in ((2047, False), (2048, True)):
        x = np.zeros((30, ns), dtype=np.float32)
        x[15, 1000] = 1.0
        rc, y = gauss(emu, x, 3.0)
        assert rc == 0, emu.d4w_last_error()
        from scipy import ndimage
        assert np.max(np.abs(y - ndimage.gaussian_filter(x.astype(np.float64), 3.0))) < dc.BLUR_BOUND
        far = y[:, np.abs(np.arange(ns) - 1000) > 12]
        assert bool(np.any(far != 0)) == fft, (ns, float(np.max(np.abs(far))))
