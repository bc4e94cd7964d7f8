"""Welch's PSD and the row operators share one transform plan per length (csrc/row_fft.h): a plan built by one family
serves the other, on the CPU emulator build through the C ABI.  Sequence and bars: tests/row_fft_shared_cases.py."""
import ctypes

import numpy as np
import pytest

from tests import row_fft_shared_cases as sc
from tests.emu_util import load_emu, vp


class EmuOps:
    def __init__(self, lib):
        self.lib = lib

    def ok(self, rc):
        assert rc == 0, self.lib.d4w_last_error()

    def welch(self, x, fs, nperseg):
        nx, ns = x.shape
        p = np.full((nx, self.lib.d4w_welch_bins(nperseg)), np.nan, dtype=np.float32)
        self.ok(self.lib.d4w_welch_f32(vp(x), nx, ns, ns, nperseg, nperseg // 2, ctypes.c_double(fs), vp(p), None))
        return p

    def envelope(self, x):
        y = np.full(x.shape, np.nan, dtype=np.float32)
        self.ok(self.lib.d4w_analytic_f32(vp(x), vp(y), x.shape[0], x.shape[1], 0, None, ctypes.c_double(0.0), None))
        return y

    def fx(self, x, nfft):
        y = np.full((x.shape[0], nfft), np.nan, dtype=np.float32)
        self.ok(self.lib.d4w_fx_f32(vp(x), vp(y), x.shape[0], x.shape[1], nfft, None))
        return y

    def spectrogram(self, row, fs, nfft):
        """dsp.get_spectrogram's two calls: all bins and the row maximum, then 20 log10(S / max)."""
        x = np.ascontiguousarray(row.reshape(1, -1), dtype=np.float32)
        hop = int(np.floor(nfft * (1 - 0.8)))
        S = np.full((1, nfft // 2 + 1, self.lib.d4w_stft_frames(x.shape[1], hop)), np.nan, dtype=np.float32)
        mx = np.empty(1, dtype=np.float32)
        self.ok(self.lib.d4w_stft_mag_f32(vp(x), vp(S), vp(mx), 1, x.shape[1], nfft, hop, 0, nfft // 2, None))
        self.ok(self.lib.d4w_scale_rows_f32(vp(S), 1, ctypes.c_size_t(S[0].size), vp(mx), 1, None))
        return S[0]


@pytest.mark.parametrize("N,welch_first", [(sc.LENGTHS[0], True), (sc.LENGTHS[1], False)])
def test_welch_and_row_operators_on_one_plan(N, welch_first):
    sc.run_sequence(EmuOps(load_emu()), N, welch_first)
