"""GPU tests of the local slant-stack semblance through dw.detect.local_semblance, with NumPy and with CUDA tensor input: the
cases of tests/semblance_cases.py (which tests/test_emu_semblance.py runs on the CPU emulator build) against the float64
restatement and the derived tolerance of tests/known_answers_semblance.py, and the exact known answers."""
import ctypes

import numpy as np
import pytest
import torch

from tests import semblance_cases as sc

pytestmark = pytest.mark.gpu
CONTAINERS = ("numpy", "tensor")


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available()
    import das4whales_amd as dw
    return dw


@pytest.fixture(scope="module")
def tile(dw):
    from das4whales_amd._lib import lib, check
    tc, ts = ctypes.c_int(), ctypes.c_int()
    check(lib.d4w_semblance_tile(ctypes.byref(tc), ctypes.byref(ts)))
    return tc.value, ts.value


def runner(dw, container):
    def run(buf, ns, delays, H, w, return_all):
        if container == "tensor":
            data = torch.from_numpy(np.array(buf, dtype=np.float32)).cuda()[:, :ns]          # pitch > ns: a view, read in place
            assert data.stride(0) == buf.shape[1]
            got = dw.detect.local_semblance(data, delays, H, weights=torch.from_numpy(np.array(w)), return_all=return_all)
            assert all(isinstance(g, torch.Tensor) and g.is_cuda for g in got)
            got = [g.cpu().numpy() for g in got]
        else:
            got = dw.detect.local_semblance(np.array(buf[:, :ns]), delays, H, weights=w, return_all=return_all)
            assert all(isinstance(g, np.ndarray) for g in got)
        assert len(got) == (3 if return_all else 2)
        assert got[0].dtype == np.float32 and got[1].dtype == np.uint8 and got[0].shape == got[1].shape == (buf.shape[0], ns)
        return got[0], got[1], (got[2] if return_all else None)
    return run


@pytest.mark.parametrize("container", CONTAINERS)
@pytest.mark.parametrize("case", sc.parity_cases(), ids=sc.case_id)
def test_parity(dw, tile, case, container):
    sc.check_parity(runner(dw, container), case, tile)


@pytest.mark.parametrize("container", CONTAINERS)
def test_plane_wave_is_exactly_one(dw, tile, container):
    sc.check_plane_wave(runner(dw, container), tile)


@pytest.mark.parametrize("container", CONTAINERS)
def test_single_channel(dw, tile, container):
    sc.check_single_channel(runner(dw, container), tile)


@pytest.mark.parametrize("container", CONTAINERS)
def test_zeros(dw, tile, container):
    sc.check_zeros(runner(dw, container), tile)


@pytest.mark.parametrize("container", CONTAINERS)
def test_scaling_and_repeat_are_bit_identical(dw, tile, container):
    sc.check_scaling_and_repeat(runner(dw, container), tile)


def test_default_weights_and_slowness_delays(dw, tile):
    """weights=None is all ones; a table from slowness_delays finds a plane wave's slowness and its sign on either side."""
    x, _, M, H, _ = sc.plane_wave(tile)
    dx, fs = 2.0, 256.0                                     # (dx fs a power of two: the table is exact)
    s = np.array([-2.0, -1.0, 0.0, 1.0, 2.0]) / (dx * fs)                                     # samples per channel / (dx fs)
    d = dw.detect.slowness_delays(s, dx, fs, M)
    coh, idx = dw.detect.local_semblance(x, d, H)
    coh1, idx1 = dw.detect.local_semblance(x, d, H, weights=np.ones(2 * M + 1))
    assert np.array_equal(coh, coh1) and np.array_equal(idx, idx1)
    inner = slice(H + M + 1, x.shape[1] - (H + M + 1))
    assert np.all(s[idx[:, inner]] == 1.0 / (dx * fs)) and np.all(coh[:, inner] == 1)
    cohr, idxr = dw.detect.local_semblance(x[::-1].copy(), d, H)                               # the cable reversed: the other sign
    assert np.all(s[idxr[:, inner]] == -1.0 / (dx * fs)) and np.all(cohr[:, inner] == 1)


def test_float64_numpy_input_keeps_its_dtype(dw, tile):
    x = np.random.default_rng(8).standard_normal((3, 50))
    coh, idx, cube = dw.detect.local_semblance(x, sc.delays_table(6, 1, 0), 2, return_all=True)
    assert coh.dtype == np.float64 and cube.dtype == np.float64 and idx.dtype == np.uint8
    c32 = dw.detect.local_semblance(x.astype(np.float32), sc.delays_table(6, 1, 0), 2)[0]
    assert np.array_equal(coh, c32.astype(np.float64))
