"""The spectrogram detector chain (STFT, row median, kernel x spectrogram correlation: csrc/stft.hip, csrc/noise.hip, csrc/spectrocorr.hip, csrc/stft_mm.hip)
on the CPU emulator build: same HIP source, same C ABI, host pointers, against the float64 references of
tests/spectro_cases.py (cases, tolerances and why the long kernels use integer inputs: there)."""
import ctypes

import numpy as np
import pytest

from tests import spectro_cases as sc
from tests.emu_util import load_emu, vp


@pytest.fixture(scope="module")
def emu():
    return load_emu()


def ok(lib, rc):
    assert rc == 0, lib.d4w_last_error()


def median(lib, v):
    v = np.ascontiguousarray(v, dtype=np.float32)
    med = np.full(v.shape[0], np.nan, dtype=np.float32)
    ok(lib, lib.d4w_row_median_f32(vp(v), v.shape[0], ctypes.c_size_t(v[0].size), vp(med), None))
    return med


def corr(lib, S, K, off, nout, zero_ends, med=None):
    """Median of every [nf, nt] spectrogram (unless given), then the correlation; the output sits in front of NaNs that
    must stay."""
    S, K = np.ascontiguousarray(S), np.ascontiguousarray(K)
    nx, nf, nt = S.shape
    if med is None:
        med = median(lib, S.reshape(nx, -1))
    buf = np.full(nx * nout + 64, np.nan, dtype=np.float32)
    out = buf[:nx * nout].reshape(nx, nout)
    ok(lib, lib.d4w_spectrocorr_f32(vp(S), nx, nf, nt, vp(K), K.shape[1], off, nout, vp(med), zero_ends, vp(out), None))
    assert np.all(np.isnan(buf[nx * nout:])), "wrote past the [nx, nout] output"
    return out


@pytest.mark.parametrize("nk", sc.REAL_NK)
def test_correlation_short_kernels(emu, nk):
    """spectro_corr<4,5>: every kernel length class (odd, even, one tap, the longest of the form), 1-13 frequency rows,
    rows shorter than the kernel, one lag, tile boundaries; both modes; medians 1e3 apart."""
    assert sc.form_of(nk) == "<4,5>"
    worst = 0.0
    for nf, nt, mode in sc.real_cases(nk):
        S, K = sc.real_input(nk, nf, nt)
        ref, raw, off, nout, ze = sc.corr_reference(S, K, mode)
        err = sc.corr_error(corr(emu, S, K, off, nout, ze), ref, raw)
        worst = max(worst, err)
        assert err <= sc.TOL, (nk, nf, nt, mode, err)
    print("spectro_corr<4,5> nk=%d: worst error / row maximum %.3e over %d cases" % (nk, worst, len(sc.real_cases(nk))))


@pytest.mark.parametrize("nk", sc.EXACT_NK)
def test_correlation_long_kernels_exact(emu, nk):
    """Every form, above all spectro_corr<2,10> and <1,20>, on integer inputs whose float32 sums are exact: the output is
    the float64 reference rounded to float32, to 1 ulp."""
    worst = 0.0
    for nf in sc.EXACT_NF:
        for nt in sc.EXACT_NT:
            S, K = sc.exact_input(nk, nf, nt)
            for mode in sc.MODES:
                if mode == "valid" and nt - nk + 1 < 1:
                    continue
                ref, off, nout, ze = sc.exact_reference(S, K, mode)
                u = sc.ulp_error(corr(emu, S, K, off, nout, ze), ref)
                worst = max(worst, u)
                assert u <= 1.0, (nk, nf, nt, mode, u)
    print("spectro_corr%s nk=%d: worst distance %.2f ulp" % (sc.form_of(nk), nk, worst))


@pytest.mark.parametrize("form", sorted(sc.IMPULSE_CASES))
@pytest.mark.parametrize("mode", sc.MODES)
def test_correlation_of_an_impulse_is_the_reversed_kernel(emu, form, mode):
    S, K, med = sc.impulse_input(form)
    want = sc.impulse_expected(form, mode)
    nk, nt = K.shape[1], S.shape[2]
    off, nout, ze = (nk // 2, nt, 0) if mode == "same" else (0, nt - nk + 1, 1)
    out = corr(emu, S, K, off, nout, ze, med=med)
    assert np.array_equal(out != 0, want != 0), "taps at the wrong lags"
    assert sc.ulp_error(out, want) <= 1.0


def test_correlation_kernel_too_long(emu):
    S, K = sc.exact_input(sc.NK_MAX, 1, 2100)
    ref, off, nout, ze = sc.exact_reference(S, K, "same")
    assert sc.ulp_error(corr(emu, S, K, off, nout, ze), ref) <= 1.0          # the longest accepted kernel
    K2 = np.ones((1, sc.NK_MAX + 1), dtype=np.float32)
    out = np.zeros((2, 2100), dtype=np.float32)
    med = np.ones(2, dtype=np.float32)
    rc = emu.d4w_spectrocorr_f32(vp(S), 2, 1, 2100, vp(K2), sc.NK_MAX + 1, (sc.NK_MAX + 1) // 2, 2100, vp(med), 0, vp(out), None)
    assert rc == -1 and b"too long" in emu.d4w_last_error() and not out.any()


@pytest.mark.parametrize("mode", sc.MODES)
def test_correlation_nan_poisons_its_window_only(emu, mode):
    S, clean, K, med = sc.nan_input()
    ref, raw, off, nout, ze = sc.corr_reference(clean, K, mode)
    out = corr(emu, S, K, off, nout, ze, med=med)
    lags = sc.nan_lags(mode)
    assert len(lags) == K.shape[1] and np.array_equal(np.flatnonzero(np.isnan(out[0])), lags)
    rest = np.ones(nout, dtype=bool)
    rest[lags] = False
    assert sc.corr_error(out[:, rest], ref[:, rest], raw[:, rest]) <= sc.TOL


@pytest.mark.parametrize("mode", sc.MODES)
def test_correlation_all_zero_row_is_nan(emu, mode):
    S, K = sc.zero_row_input()
    ref, raw, off, nout, ze = sc.corr_reference(S, K, mode)
    out = corr(emu, S, K, off, nout, ze)
    inner = slice(1, -1) if mode == "valid" else slice(None)                 # 'valid' forces its two ends to 0
    assert np.all(np.isnan(out[1, inner])) and np.all(np.isnan(ref[1, inner]))
    if mode == "valid":
        assert out[1, 0] == 0 and out[1, -1] == 0
    assert sc.corr_error(out[[0, 2]], ref[[0, 2]], raw[[0, 2]]) <= sc.TOL


@pytest.mark.parametrize("mode", sc.MODES)
def test_correlation_negative_median(emu, mode):
    """A dB spectrogram: 'same' clips the raw sum and then divides by the negative median (values <= 0, detect.py:599-600),
    'valid' divides and then clips (values >= 0, detect.py:642-645)."""
    S, K = sc.negative_median_input()
    ref, raw, off, nout, ze = sc.corr_reference(S, K, mode)
    out = corr(emu, S, K, off, nout, ze)
    assert (ref.max() <= 0 and ref.min() < 0) if mode == "same" else (ref.min() >= 0 and ref.max() > 0)
    err = sc.corr_error(out, ref, raw)
    print("negative median, %s: output in [%.3f, %.3f], reference in [%.3f, %.3f], error %.3e"
          % (mode, out.min(), out.max(), ref.min(), ref.max(), err))
    assert err <= sc.TOL


def test_median_detector_rows(emu):
    v = sc.detector_rows()
    assert np.array_equal(median(emu, v), sc.median_reference(v))
    vo = np.ascontiguousarray(v[:, :-1])                                     # odd count
    assert np.array_equal(median(emu, vo), sc.median_reference(vo))


@pytest.mark.parametrize("n", sc.MEDIAN_N)
def test_median_row_kinds(emu, n):
    v = sc.median_rows(n)
    med, ref = median(emu, v), sc.median_reference(v)
    assert np.array_equal(med, ref), (n, np.flatnonzero(med != ref), med, ref)


def test_median_many_rows_one_launch(emu):
    v = sc.median_many_rows()
    med, ref = median(emu, v), sc.median_reference(v)
    assert np.array_equal(med, ref), np.flatnonzero(med != ref)


def stft(lib, x, n_fft, hop, lo, hi, want_max):
    nx, ns = x.shape
    nt = lib.d4w_stft_frames(ns, hop)
    S = np.full((nx, hi - lo + 1, nt), np.nan, dtype=np.float32)
    mx = np.full(nx, np.nan, dtype=np.float32) if want_max else None
    ok(lib, lib.d4w_stft_mag_f32(vp(x), vp(S), vp(mx) if want_max else None, nx, ns, n_fft, hop, lo, hi, None))
    return S, mx


@pytest.mark.parametrize("name", sorted(sc.STFT_EMU_CASES))
def test_stft_forms_and_edges(emu, name):
    n_fft, hop, nx, ns, lo, hi, want_max = sc.STFT_CASES[name]
    x = sc.stft_case_input(name)
    mm = (not want_max) and emu.d4w_stft_mm_eligible(n_fft, hop, lo, hi) == 1
    assert mm == name.startswith("mm-"), "the table's matrix-core cases are the eligible ones"
    S, mx = stft(emu, x, n_fft, hop, lo, hi, want_max)
    err = sc.stft_error(S, name)
    print("stft %s (%s): error / full maximum %.3e" % (name, "matrix cores" if mm else "FFT", err))
    assert err <= (sc.MM_TOL if mm else sc.TOL)
    if want_max:
        _, full_max = sc.stft_reference(name)
        assert np.all(np.abs(mx - full_max) <= sc.TOL * full_max)
        lo2, hi2 = sc.stft_slice(name)
        if (lo, hi) == (0, n_fft // 2) and lo2 <= hi2:
            S2, mx2 = stft(emu, x, n_fft, hop, lo2, hi2, True)
            assert np.array_equal(S2, S[:, lo2:hi2 + 1]) and np.array_equal(mx2, mx)
