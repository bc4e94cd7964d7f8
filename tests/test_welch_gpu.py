"""GPU tests of csrc/welch.hip through the Python interface: dsp.welch_psd, tools.spec, tools.energy_TimeDomain and
tools.disp_comprate, against scipy.signal.welch / float64 sums with the cases and tolerances of tests/welch_cases.py
(1e-5 of every row's maximum; energy at rtol 1e-6)."""
import numpy as np
import pytest
import torch

from tests import welch_cases as wc

pytestmark = pytest.mark.gpu
FS = 200.0


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import das4whales_amd as dw_
    from das4whales_amd import _lib
    assert "gfx950" in _lib.version()
    return dw_


@pytest.mark.parametrize("name", sorted(wc.GPU_CASES))
def test_welch_psd_matches_scipy(dw, name):
    nx, ns, chunk, nperseg, noverlap = wc.GPU_CASES[name]
    ref, _ = wc.reference(name, FS)
    x = wc.make_input(name)
    f, p = dw.dsp.welch_psd(x, FS, nperseg=nperseg, noverlap=noverlap, chunk=chunk)
    assert isinstance(p, np.ndarray) and p.dtype == np.float32
    assert np.array_equal(f, np.fft.rfftfreq(nperseg, 1.0 / FS))
    wc.check_rows(p, ref, name)
    if chunk == ns:                                                   # chunk=None: one chunk, the whole record, [nx, nbins]
        f1, p1 = dw.dsp.welch_psd(x, FS, nperseg=nperseg, noverlap=noverlap)
        assert p1.shape == (nx, nperseg // 2 + 1) and np.array_equal(p1, p[:, 0])


def test_welch_psd_containers_and_stream(dw):
    """float64 NumPy in -> float64 out; a device tensor in -> a device tensor out, computed on the current (non-default)
    stream, the same bits both ways; 1-D in -> one row less."""
    name = "odd_sizes"
    nx, ns, chunk, nperseg, noverlap = wc.CASES[name]
    ref, _ = wc.reference(name, FS)
    x32 = wc.make_input(name)
    _, p32 = dw.dsp.welch_psd(x32, FS, nperseg=nperseg, noverlap=noverlap, chunk=chunk)
    _, p64 = dw.dsp.welch_psd(x32.astype(np.float64), FS, nperseg=nperseg, noverlap=noverlap, chunk=chunk)
    assert p64.dtype == np.float64 and np.array_equal(p64, p32.astype(np.float64))
    xt = torch.from_numpy(np.array(x32)).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        f, pt = dw.dsp.welch_psd(xt, FS, nperseg=nperseg, noverlap=noverlap, chunk=chunk)
        e = dw.tools.energy_TimeDomain(xt, chunk=chunk)
    side.synchronize()
    assert isinstance(pt, torch.Tensor) and pt.is_cuda and pt.dtype == torch.float32 and isinstance(f, np.ndarray)
    assert isinstance(e, torch.Tensor) and e.is_cuda and e.shape == (nx, -(-ns // chunk))
    assert np.array_equal(pt.cpu().numpy(), p32)
    wc.check_rows(pt.cpu().numpy(), ref, name + " (tensor, side stream)")
    _, p1 = dw.dsp.welch_psd(x32[1], FS, nperseg=nperseg, noverlap=noverlap, chunk=chunk)
    assert p1.shape == ref.shape[1:] and np.array_equal(p1, p32[1])


@pytest.mark.parametrize("name", ["reference_case", "rows_64x12000"])
def test_spec_is_the_reference_case(dw, name):
    """tools.spec = welch(fs=200, nperseg=1024) over chunks of 3000 samples: against SciPy, bit for bit the general form,
    and its 1-D and 2-D forms agree."""
    nx, ns, chunk, nperseg, _ = wc.GPU_CASES[name]
    assert (chunk, nperseg) == (3000, 1024)
    ref, _ = wc.reference(name, 200.0)
    x = wc.make_input(name)
    s = dw.tools.spec(x)
    assert s.shape == (nx, int(ns / 3000), 513) and s.dtype == np.float32
    wc.check_rows(s, ref, "spec " + name)
    assert np.array_equal(s, dw.dsp.welch_psd(x, fs=200, nperseg=1024, chunk=3000)[1])
    for r in (0, nx - 1):
        s1 = dw.tools.spec(x[r])
        assert s1.shape == (int(ns / 3000), 513) and np.array_equal(s1, s[r])
    s64 = dw.tools.spec(x[:3].astype(np.float64))
    assert s64.dtype == np.float64 and np.array_equal(s64, s[:3].astype(np.float64))


@pytest.mark.parametrize("name", sorted(wc.ENERGY_CASES))
def test_energy_time_domain(dw, name):
    ns, chunk = wc.ENERGY_CASES[name]
    x = wc.energy_input(name)
    ref = wc.energy_reference(name)
    e = dw.tools.energy_TimeDomain(x, chunk=chunk)
    assert e.shape == ref.shape and e.dtype == np.float32
    print("energy %s: max relative error %.3e" % (name, np.max(np.abs(e - ref) / ref)))
    np.testing.assert_allclose(e, ref, rtol=wc.ENERGY_RTOL, atol=0.0)
    e64 = dw.tools.energy_TimeDomain(x.astype(np.float64), 'time', chunk=chunk)
    assert e64.dtype == np.float64 and np.array_equal(e64, e.astype(np.float64))
    e1 = dw.tools.energy_TimeDomain(x[1], chunk=chunk)
    assert e1.shape == ref.shape[1:] and np.array_equal(e1, e[1])


def test_welch_psd_argument_errors(dw):
    x = np.zeros((2, 4000), dtype=np.float32)
    for kw in (dict(nperseg=1023), dict(nperseg=8), dict(nperseg=4098), dict(nperseg=2 * 37), dict(nperseg=1024, noverlap=1024),
               dict(nperseg=1024, chunk=1000), dict(nperseg=1024, chunk=4001)):
        with pytest.raises(ValueError, match="d4w: "):
            dw.dsp.welch_psd(x, FS, **kw)


def test_disp_comprate_designed_mask(dw, capsys):
    """A designed mask is counted on the device: the sizes follow mask.nnz and the dense form is not kept."""
    mask = dw.dsp.hybrid_ninf_filter_design((64, 240), [0, 320, 5], 2.0419, 200.0)
    assert mask._tensor is None
    assert dw.tools.disp_comprate(mask) is None
    assert mask._tensor is None
    out = capsys.readouterr().out
    gib = 1024.0 ** 3
    nnz = mask.nnz
    assert 0 < nnz < 64 * 240
    sparse, dense = nnz * 8 / gib, 64 * 240 * 8 / gib
    assert out == (f'The size of the sparse filter is {sparse:.4f} Gib\n'
                   f'The size of the dense filter is {dense:.2f} Gib\n'
                   f'The compression ratio is {dense / sparse:.2f} ({abs(dense - sparse) * 100 / dense:.1f} %)\n')
    formed = mask.tensor                                              # a mask whose dense form exists keeps it
    dw.tools.disp_comprate(mask)
    assert mask._tensor is formed and capsys.readouterr().out == out
    assert dw.tools.disp_comprate(dw.dsp.DeviceMask(formed)) is None and capsys.readouterr().out == out
