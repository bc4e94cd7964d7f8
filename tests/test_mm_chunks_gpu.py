"""The matched filter's chunk walk on the GPU (csrc/xcorr_mm.hip; the cases of tests/test_emu_mm_chunks.py): row counts
around a grid of 512 workgroups (fewer rows than workgroups, one more, a last round that is a sixth full), row lengths around
one and two groups of 4096 lags.  detect.compute_cross_correlograms(y, [hf, lf]) against float64, against the two one-template
calls, and the two-template kernel against the two one-template launches bit for bit.

Bounds (tests/test_rowops_gpu.py): 1e-6 of a white row's own maximum, 1e-5 (that file's TOL, the drifting-rows test) of every
other row's."""
import numpy as np
import pytest
import torch

from tests import mm_chunk_cases as cs

pytestmark = pytest.mark.gpu
WHITE, TOL = 1e-6, 1e-5
CASES = [(1, 4095), (3, 4096), (511, 4100), (513, 8191), (3, 8192), (600, 8193), (513, 12000), (1, 16385), (600, 16385)]
CHECKED = 12         # rows compared with float64 per case: the first and the last ones (the ragged last round)


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import das4whales_amd as dw_
    return dw_


def bounds(kinds):
    return np.array([WHITE if k == "white" else TOL for k in kinds])


@pytest.mark.parametrize("nx,ns", CASES)
def test_public_pair_call_on_every_row_kind_and_length(dw, nx, ns):
    idx = CASES.index((nx, ns))
    sup = cs.SUPPORTS[idx % 2]
    x = cs.rows(nx, ns, seed=2000 + idx, first_kind=idx)
    kinds = cs.kinds(nx, idx)
    tpls = [cs.template(ns, sup[t], zero_mean=False, seed=7 * idx + t) for t in range(2)]
    xd = torch.from_numpy(x).cuda()
    got = dw.detect.compute_cross_correlograms(xd, tpls)
    sel = np.unique(np.r_[np.arange(min(nx, CHECKED)), np.arange(max(nx - CHECKED, 0), nx)])
    for t in range(2):
        y = got[t].cpu().numpy()
        e = cs.row_err(y[sel], cs.reference(x[sel], tpls[t], True))
        print("nx %d ns %d template %d: worst white row %.2e, worst other row %.2e" % (
            nx, ns, t, max([v for v, r in zip(e, sel) if kinds[r] == "white"], default=0.0),
            max([v for v, r in zip(e, sel) if kinds[r] != "white"], default=0.0)))
        assert np.all(e < bounds([kinds[r] for r in sel])), (t, e)
        one = dw.detect.compute_cross_correlogram(xd, tpls[t])
        e1 = cs.row_err(one.cpu().numpy(), y.astype(np.float64))
        assert np.all(e1 < bounds(kinds)), (t, e1.max())
    # chunks of 8192 lags (two templates) and of 4096 (one): the same arithmetic for every lag
    for with_tail in (False, True):
        tt = [cs.taps_and_tail(tp, with_tail) for tp in tpls]
        taps, tails = [a for a, _ in tt], ([b for _, b in tt] if with_tail else None)
        pair = dw.detect._xcorr_device(xd, taps, normalize=True, method="mm", tails=tails)
        for t in range(2):
            (single,) = dw.detect._xcorr_device(xd, [taps[t]], normalize=True, method="mm", tails=[tails[t]] if with_tail else None)
            assert torch.equal(single, pair[t]), (with_tail, t, float((single - pair[t]).abs().max()))


@pytest.mark.parametrize("ns", [4100, 8193, 12000])
def test_rows_without_statistics_scale_every_group_alone(dw, ns):
    rng = np.random.default_rng(ns)
    nx = 513
    x = rng.standard_normal((nx, ns)) * np.where(np.arange(ns) < 4500, 1.0, 1e-3)[None, :] * 37.0
    x = np.ascontiguousarray(x, dtype=np.float32)
    xd = torch.from_numpy(x).cuda()
    taps = [rng.standard_normal(163), rng.standard_normal(150) * 0.01]
    pair = dw.detect._xcorr_device(xd, taps, normalize=False, method="mm")
    sel = np.r_[0:CHECKED, nx - CHECKED:nx]
    for t in range(2):
        ref = np.stack([cs.orc.shift_xcorr(r.astype(np.float64), np.pad(taps[t], (0, ns - len(taps[t])))) for r in x[sel]])
        assert cs.row_err(pair[t][sel].cpu().numpy(), ref).max() < WHITE
        (single,) = dw.detect._xcorr_device(xd, [taps[t]], normalize=False, method="mm")
        assert torch.equal(single, pair[t])


def test_unaligned_rows_short_continuation_and_row_maxima(dw):
    nx, ns, n_next = 600, 8193 + 4096, 50
    x = cs.rows(nx, ns, seed=78, first_kind=1)
    tpls = [cs.template(ns, s, zero_mean=False, seed=s) for s in (136, 156)]
    tt = [cs.taps_and_tail(tp, True) for tp in tpls]
    taps, tails = [a for a, _ in tt], [b for _, b in tt]
    xd = torch.from_numpy(x).cuda()
    stats = dw.detect._row_stats_cached(xd)[:2]
    base = dw.detect._xcorr_device(xd, taps, normalize=True, method="mm", stats=stats, tails=tails)
    # rows that start 4 bytes past a 16-byte boundary, odd length: scalar loads and stores in every chunk
    buf = torch.zeros(nx * ns + 4, dtype=torch.float32, device="cuda")
    xu = buf[1:1 + nx * ns].view(nx, ns)
    xu.copy_(xd)
    assert xu.data_ptr() % 16 == 4
    got = dw.detect._xcorr_device(xu, taps, normalize=True, method="mm", stats=stats, tails=tails)
    assert all(torch.equal(a, b) for a, b in zip(got, base))
    # the rows' maxima out of the epilogue
    rm = []
    ys = dw.detect._xcorr_device(xd, taps, normalize=True, method="mm", stats=stats, tails=tails, row_max=rm)
    for t in range(2):
        assert torch.equal(ys[t], base[t]) and torch.equal(rm[t], base[t].max(dim=1).values)
    # a continuation shorter than the halo: two templates and one template agree bit for bit, and the last lags moved
    rng = np.random.default_rng(5)
    head = torch.from_numpy(np.ascontiguousarray(rng.standard_normal((nx, 64)) * x.std(axis=1, keepdims=True) + x.mean(axis=1, keepdims=True),
                                                 dtype=np.float32)).cuda()
    cont = dw.detect._xcorr_device(xd, taps, normalize=True, method="mm", stats=stats, tails=tails, cont=(head, n_next))
    for t in range(2):
        (one,) = dw.detect._xcorr_device(xd, [taps[t]], normalize=True, method="mm", stats=stats, tails=[tails[t]], cont=(head, n_next))
        assert torch.equal(one, cont[t])
        assert not torch.equal(cont[t][:, -100:], base[t][:, -100:])
    plain = dw.detect._xcorr_device(xd, [cs.taps_and_tail(tp, False)[0] for tp in tpls], normalize=True, method="mm", stats=stats,
                                    cont=(head, n_next))
    sel = np.r_[0:CHECKED, nx - CHECKED:nx]
    kinds = cs.kinds(nx, 1)
    for t in range(2):
        ref = cs.reference(x[sel], tpls[t], False, head=head[sel, :n_next].cpu().numpy())
        assert np.all(cs.row_err(plain[t][sel].cpu().numpy(), ref) < bounds([kinds[r] for r in sel]))
    # a row that holds a NaN: its maximum is NaN, the other rows keep theirs
    xn = xd.clone()
    xn[2, 9000] = float("nan")
    rm = []
    ys = dw.detect._xcorr_device(xn, taps, normalize=True, method="mm", stats=stats, tails=tails, row_max=rm)
    keep = torch.tensor([0, 1, 3, nx - 1], device="cuda")
    for t in range(2):
        assert bool(torch.isnan(rm[t][2])) and torch.equal(rm[t][keep], base[t][keep].max(dim=1).values)


def _checked(nx):
    return np.unique(np.r_[np.arange(min(nx, CHECKED)), np.arange(max(nx - CHECKED, 0), nx)])


@pytest.mark.parametrize("support", [150, 200, 330, 450])
def test_one_template_kernels_of_every_depth_with_tail_and_row_maxima(dw, support):
    """One template of 6, 7, 11 and 15 k-steps -- the 6-, 8-, 12- and 16-step kernels -- without and with the tail, without and
    with the row maxima (the 6-step kernel with both is an instantiation of its own): float64, the same values whether or not
    the maxima are formed, and the maxima of what was stored.  One row more than the grid, one sample into a third chunk."""
    nx, ns = 513, 8193
    x = cs.rows(nx, ns, seed=300 + support)
    kinds, sel = cs.kinds(nx), _checked(nx)
    xd = torch.from_numpy(x).cuda()
    for with_tail in (False, True):
        tpl = cs.template(ns, support, zero_mean=False, seed=support)
        taps, tail = cs.taps_and_tail(tpl, with_tail)
        tails = [tail] if with_tail else None
        (plain,) = dw.detect._xcorr_device(xd, [taps], normalize=True, method="mm", tails=tails)
        e = cs.row_err(plain[sel].cpu().numpy(), cs.reference(x[sel], tpl, with_tail))
        print("support %d tail %s: worst white row %.2e, worst other row %.2e" % (
            support, with_tail, max([v for v, r in zip(e, sel) if kinds[r] == "white"], default=0.0),
            max([v for v, r in zip(e, sel) if kinds[r] != "white"], default=0.0)))
        assert np.all(e < bounds([kinds[r] for r in sel])), (with_tail, e)
        rm = []
        (y,) = dw.detect._xcorr_device(xd, [taps], normalize=True, method="mm", tails=tails, row_max=rm)
        assert torch.equal(y, plain) and torch.equal(rm[0], plain.max(dim=1).values)


@pytest.mark.parametrize("with_tail", [False, True], ids=["tail0", "tail"])
def test_row_maxima_of_the_pairs(dw, with_tail):
    """The two-template kernels of 5 + 6 and of 6 + 6 k-steps with the row maxima, without and with the tail."""
    nx, ns = 513, 8193
    x = cs.rows(nx, ns, seed=98)
    kinds, sel = cs.kinds(nx), _checked(nx)
    xd = torch.from_numpy(x).cuda()
    for sup in cs.SUPPORTS:
        tpls = [cs.template(ns, s, zero_mean=False, seed=s) for s in sup]
        tt = [cs.taps_and_tail(tp, with_tail) for tp in tpls]
        taps, tails = [a for a, _ in tt], ([b for _, b in tt] if with_tail else None)
        plain = dw.detect._xcorr_device(xd, taps, normalize=True, method="mm", tails=tails)
        rm = []
        ys = dw.detect._xcorr_device(xd, taps, normalize=True, method="mm", tails=tails, row_max=rm)
        for t in range(2):
            e = cs.row_err(plain[t][sel].cpu().numpy(), cs.reference(x[sel], tpls[t], with_tail))
            assert np.all(e < bounds([kinds[r] for r in sel])), (sup, t, e)
            assert torch.equal(ys[t], plain[t]) and torch.equal(rm[t], plain[t].max(dim=1).values)
