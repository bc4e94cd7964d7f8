"""Welch's PSD and the row operators on ONE transform plan per length (csrc/row_fft.h): the sequence, inputs, float64
references and checks shared by tests/test_row_fft_shared_gpu.py (Python interface) and tests/test_emu_row_fft_shared.py
(CPU emulator, C ABI).

A plan of length N is built by whichever family asks first and then serves both.  For N = 240 (2^4 3 5, fast radices only)
Welch comes first, then the row operators, then Welch again; for N = 224 (2^5 7, the GENERIC stage path) the row operators
come first and Welch last, and both are run once more.  Every repeated result equals the first bit for bit, and every
result meets the bar of its own test: tests/welch_cases.py, tests/analytic_cases.py, tests/test_spectral_gpu.py (imported,
not restated).

`ops` is the adapter of the build under test:
    ops.welch(x, fs, nperseg) -> [nx, nperseg // 2 + 1]     (one chunk, noverlap = nperseg // 2)
    ops.envelope(x)           -> [nx, ns]
    ops.fx(x, nfft)           -> [nx, nfft]
    ops.spectrogram(row, fs, nfft) -> [nfft // 2 + 1, frames]  in dB under the row's maximum (overlap 0.8)"""
import numpy as np
import scipy.signal as sps

from oracle import d4w_oracle as orc
from tests import analytic_cases as ac
from tests import welch_cases as wc
from tests.test_spectral_gpu import TOL, rel

FS = 200.0
NX = 8
LENGTHS = (240, 224)


def welch_block(N):
    """[8, 4 N] float32 in the row kinds of tests/welch_cases.py: noise, noise 1000 x its rms off zero, a tone between bins."""
    rng = np.random.default_rng(N)
    ns = 4 * N
    x = rng.standard_normal((NX, ns))
    t = np.arange(ns)
    for r in range(NX):
        if r % 3 == 1:
            x[r] += 1000.0 * np.sqrt(np.mean(x[r] ** 2))
        elif r % 3 == 2:
            x[r] = np.sin(2.0 * np.pi * (N // 8 + r // 3 + 0.5) / N * t + 0.3 * r) + 1e-3 * x[r]
    return np.ascontiguousarray(x, dtype=np.float32)


def run_welch(ops, N, x):
    p = np.asarray(ops.welch(x, FS, N))
    ref = sps.welch(x.astype(np.float64), fs=FS, nperseg=N, noverlap=N // 2, axis=-1)[1]
    wc.check_rows(p, ref, "nperseg %d" % N)
    return p


def run_row_ops(ops, N, xw):
    """envelope of 8 x 2 N (packed, L = N) and of 8 x (N - 1) (odd), get_fx(nfft = N), get_spectrogram(nfft = N)."""
    out = []
    for ns in (2 * N, N - 1):
        x = ac.tone_block(NX, ns, seed=N + ns)
        y = np.asarray(ops.envelope(x))
        err = ac.check_mode(0, y, *ac.reference(x))
        print("envelope %d x %d: %.3e" % (NX, ns, err))
        out.append(y)
    x = ac.tone_block(NX, 2 * N, seed=N)
    y = np.asarray(ops.fx(x, N))
    err = rel(y, orc.get_fx(x.astype(np.float64), N))
    print("get_fx nfft %d: %.3e" % (N, err))
    assert err < TOL
    out.append(y)
    p = np.asarray(ops.spectrogram(xw[0], FS, N))
    ref = orc.get_spectrogram(xw[0].astype(np.float64), FS, nfft=N)[0]
    assert p.shape == ref.shape
    err = float(np.max(np.abs(10.0 ** (p.astype(np.float64) / 20) - 10.0 ** (ref / 20))))
    print("get_spectrogram nfft %d: %.3e" % (N, err))
    assert err < TOL
    out.append(p)
    return out


def run_sequence(ops, N, welch_first):
    xw = welch_block(N)
    if welch_first:
        p1 = run_welch(ops, N, xw)
        run_row_ops(ops, N, xw)
        assert np.array_equal(run_welch(ops, N, xw), p1), "Welch after the row operators differs from Welch before them"
        return
    r1 = run_row_ops(ops, N, xw)
    p1 = run_welch(ops, N, xw)
    for a, b in zip(r1, run_row_ops(ops, N, xw)):
        assert np.array_equal(a, b), "a row operator after Welch differs from the same call before it"
    assert np.array_equal(run_welch(ops, N, xw), p1)
