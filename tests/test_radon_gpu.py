"""GPU parity of improcess.compute_radon_transform (csrc/radon.hip) against the fixture recorded from the reference's
call (tests/golden/radon.npz: skimage.transform.radon(x, theta, circle=False)), against the float64 restatement of
tests/test_emu_radon.py at the binned file-image shape, and against known answers."""
import numpy as np
import pytest
import torch

from tests import golden_npz
from tests.test_emu_radon import radon_f64, rel

pytestmark = pytest.mark.gpu
TOL = 1e-5
G = golden_npz.load("radon.npz")
CASES = [str(c) for c in G["cases"]]


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available()
    import das4whales_amd as dw_
    return dw_


@pytest.mark.parametrize("name", CASES)
def test_fixture_parity_and_dtype(dw, name):
    x, th, ref = G[name + "/x"], G[name + "/theta"], G[name + "/y"]
    y = dw.improcess.compute_radon_transform(x, theta=th)
    assert isinstance(y, np.ndarray) and y.shape == ref.shape
    assert y.dtype == np.dtype(str(G[name + "/dtype"])), (x.dtype, y.dtype)
    assert rel(y, ref) < TOL, (name, rel(y, ref))


def test_default_theta(dw):
    x = G["s37x52/x"]
    y = dw.improcess.compute_radon_transform(x)
    assert y.shape == (74, 180) and y.dtype == np.float64
    assert rel(y, G["s37x52/y"]) < TOL


def _file_image(h=1102, w=1200, seed=11):
    """A binned file image: smooth background, a bright line and noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    img = 40.0 + 30.0 * np.sin(xx / w * 5.0) * np.cos(yy / h * 3.0)
    img += 200.0 * (np.abs(yy - 0.7 * xx - 100.0) < 2.0)
    img += 5.0 * rng.standard_normal((h, w))
    return img


def test_file_image_shape_vs_restatement(dw):
    img = _file_image()
    th = np.array([0.0, 1.0, 33.0, 45.0, 47.3, 90.0, 137.3, 200.5])
    y = dw.improcess.compute_radon_transform(img, theta=th)
    ref = radon_f64(img, th)
    assert y.shape == ref.shape == (1698, th.size) and y.dtype == np.float64
    for i in range(th.size):                            # every angle against the sinogram's scale
        assert float(np.max(np.abs(y[:, i] - ref[:, i]))) / float(np.max(np.abs(ref))) < TOL, th[i]


def test_disc_known_answer(dw):
    """A centred disc of radius rho projects to the chord 2 sqrt(rho^2 - s^2) at every angle; each angle's column sum
    is the restatement's (the disc's area, as bilinear rotation keeps the mass of an interior object)."""
    n, rho = 201, 60.0
    yy, xx = np.meshgrid(np.arange(n) - n // 2, np.arange(n) - n // 2, indexing="ij")
    disc = (xx * xx + yy * yy <= rho * rho).astype(np.float64)
    th = np.array([0.0, 10.0, 45.0, 72.5, 90.0, 137.3, 180.0])
    y = dw.improcess.compute_radon_transform(disc, theta=th)
    P = y.shape[0]
    s = np.arange(P) - P // 2
    chord = 2.0 * np.sqrt(np.maximum(rho * rho - s * s, 0.0))
    inner, outer = np.abs(s) <= rho - 2, np.abs(s) >= rho + 2
    for i in range(th.size):
        assert np.max(np.abs(y[inner, i] - chord[inner])) < 2.0, th[i]       # pixelated edge: within a pixel at either end
        assert np.all(y[outer, i] == 0.0), th[i]
    ref = radon_f64(disc, th)
    assert np.allclose(y.sum(0), ref.sum(0), rtol=1e-6, atol=0)
    assert np.allclose(y.sum(0), disc.sum(), rtol=1e-3)


def test_bit_identical_runs(dw):
    x = torch.from_numpy(_file_image(401, 555, seed=3)).to(torch.float32).cuda()
    a = dw.improcess.compute_radon_transform(x)
    b = dw.improcess.compute_radon_transform(x)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_tensor_in_tensor_out(dw):
    img = G["s240x320/x"]
    x = torch.from_numpy(img).to(torch.float64).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        y = dw.improcess.compute_radon_transform(x, theta=torch.arange(0, 180, dtype=torch.float64))
    s.synchronize()
    assert isinstance(y, torch.Tensor) and y.is_cuda and y.device == x.device and y.dtype == torch.float32
    assert tuple(y.shape) == (453, 180) and rel(y.cpu().numpy(), G["s240x320/y"]) < TOL
    # integer and bool tensors follow the NumPy dtype rule (img_as_float), still returned as float32
    u8 = torch.from_numpy(G["u8/x"]).cuda()
    yu = dw.improcess.compute_radon_transform(u8, theta=G["u8/theta"])
    assert yu.dtype == torch.float32 and rel(yu.cpu().numpy(), G["u8/y"]) < TOL
    b = torch.from_numpy(G["bool/x"]).cuda()
    yb = dw.improcess.compute_radon_transform(b, theta=G["bool/theta"])
    assert rel(yb.cpu().numpy(), G["bool/y"]) < TOL


def test_empty_theta_and_bad_input(dw):
    ip = dw.improcess
    y = ip.compute_radon_transform(np.ones((5, 7)), theta=np.array([]))
    assert y.shape == (10, 0) and y.dtype == np.float64
    yt = ip.compute_radon_transform(torch.ones((5, 7), device="cuda"), theta=[])
    assert tuple(yt.shape) == (10, 0) and yt.is_cuda
    with pytest.raises(ValueError):
        ip.compute_radon_transform(np.ones((4, 5, 3)))
    with pytest.raises(ValueError):
        ip.compute_radon_transform(torch.ones((4, 5, 3), device="cuda"))
    with pytest.raises(ValueError):
        ip.compute_radon_transform(np.ones((4, 5)), theta=np.array([0.0, np.nan]))
