"""Welch's PSD and the row operators share one transform plan per length (csrc/row_fft.h): a plan built by one family
serves the other, through the Python interface on the GPU.  Sequence and bars: tests/row_fft_shared_cases.py."""
import pytest
import torch

from tests import row_fft_shared_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import das4whales_amd as dw_
    return dw_


class PyOps:
    def __init__(self, dw):
        self.dsp = dw.dsp

    def welch(self, x, fs, nperseg):
        return self.dsp.welch_psd(x, fs, nperseg=nperseg)[1]

    def envelope(self, x):
        return self.dsp.envelope(x)

    def fx(self, x, nfft):
        return self.dsp.get_fx(x, nfft)

    def spectrogram(self, row, fs, nfft):
        return self.dsp.get_spectrogram(row, fs, nfft=nfft)[0]


@pytest.mark.parametrize("N,welch_first", [(sc.LENGTHS[0], True), (sc.LENGTHS[1], False)])
def test_welch_and_row_operators_on_one_plan(dw, N, welch_first):
    sc.run_sequence(PyOps(dw), N, welch_first)
