"""GPU tests of the spectrogram detector chain through the Python interface: dw.detect._spectrocorr_device, xcorr2d, xcorr,
nxcorr2d, dw.dsp._stft_mag and d4w_row_median_f32 as detect.xcorr calls it, against the float64 references of
tests/spectro_cases.py -- every form of the correlation kernel (spectro_corr<4,5>, <2,10>, <1,20>), of the STFT (stft_fat,
stft_mag, Bluestein, the matrix-core form, tile walks) and the radix select on row kinds the detector never feeds it.
Device tensors in, compared on the host; every test prints its worst figure before it asserts."""
import numpy as np
import pytest
import scipy.signal as sps
import torch

from tests import spectro_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import das4whales_amd as dw_
    from das4whales_amd import _lib
    assert "gfx950" in _lib.version()
    return dw_


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def corr(dw, S, K, off, nout, zero_ends, med=None):
    out = dw.detect._spectrocorr_device(cuda(S), K, off, nout, med=None if med is None else cuda(med), zero_ends=bool(zero_ends))
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (S.shape[0], nout)
    return out.cpu().numpy()


def median(dw, v):
    """d4w_row_median_f32 the way detect.xcorr calls it."""
    from das4whales_amd import _device as dev
    from das4whales_amd._lib import check, lib
    t = cuda(np.ascontiguousarray(v, dtype=np.float32))
    med = torch.full((t.shape[0],), float("nan"), dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        check(lib.d4w_row_median_f32(dev.ptr(t), t.shape[0], t[0].numel(), dev.ptr(med), dev.stream_ptr(t)))
    return med.cpu().numpy()


@pytest.mark.parametrize("nk", sc.REAL_NK)
def test_correlation_short_kernels(dw, nk):
    assert sc.form_of(nk) == "<4,5>"
    worst = 0.0
    for nf, nt, mode in sc.real_cases(nk):
        S, K = sc.real_input(nk, nf, nt)
        ref, raw, off, nout, ze = sc.corr_reference(S, K, mode)
        err = sc.corr_error(corr(dw, S, K, off, nout, ze), ref, raw)
        worst = max(worst, err)
        assert err <= sc.TOL, (nk, nf, nt, mode, err)
    print("spectro_corr<4,5> nk=%d: worst error / row maximum %.3e over %d cases" % (nk, worst, len(sc.real_cases(nk))))


@pytest.mark.parametrize("nk", sc.EXACT_NK)
def test_correlation_long_kernels_exact(dw, nk):
    worst = 0.0
    for nf in sc.EXACT_NF:
        for nt in sc.EXACT_NT:
            S, K = sc.exact_input(nk, nf, nt)
            for mode in sc.MODES:
                if mode == "valid" and nt - nk + 1 < 1:
                    continue
                ref, off, nout, ze = sc.exact_reference(S, K, mode)
                u = sc.ulp_error(corr(dw, S, K, off, nout, ze), ref)
                worst = max(worst, u)
                assert u <= 1.0, (nk, nf, nt, mode, u)
    print("spectro_corr%s nk=%d: worst distance %.2f ulp" % (sc.form_of(nk), nk, worst))


@pytest.mark.parametrize("form", sorted(sc.IMPULSE_CASES))
@pytest.mark.parametrize("mode", sc.MODES)
def test_correlation_of_an_impulse_is_the_reversed_kernel(dw, form, mode):
    S, K, med = sc.impulse_input(form)
    want = sc.impulse_expected(form, mode)
    nk, nt = K.shape[1], S.shape[2]
    off, nout, ze = (nk // 2, nt, 0) if mode == "same" else (0, nt - nk + 1, 1)
    out = corr(dw, S, K, off, nout, ze, med=med)
    assert np.array_equal(out != 0, want != 0), "taps at the wrong lags"
    u = sc.ulp_error(out, want)
    print("impulse %s %s: %.2f ulp" % (form, mode, u))
    assert u <= 1.0


def test_correlation_kernel_too_long(dw):
    S = np.ones((1, 1, 2100), dtype=np.float32)
    with pytest.raises(ValueError, match="too long"):
        dw.detect.xcorr2d(cuda(S[0]), np.ones((1, sc.NK_MAX + 1)))


@pytest.mark.parametrize("mode", sc.MODES)
def test_correlation_nan_poisons_its_window_only(dw, mode):
    S, clean, K, med = sc.nan_input()
    ref, raw, off, nout, ze = sc.corr_reference(clean, K, mode)
    out = corr(dw, S, K, off, nout, ze, med=med)
    lags = sc.nan_lags(mode)
    assert len(lags) == K.shape[1] and np.array_equal(np.flatnonzero(np.isnan(out[0])), lags)
    rest = np.ones(nout, dtype=bool)
    rest[lags] = False
    assert sc.corr_error(out[:, rest], ref[:, rest], raw[:, rest]) <= sc.TOL


@pytest.mark.parametrize("mode", sc.MODES)
def test_correlation_all_zero_row_is_nan(dw, mode):
    S, K = sc.zero_row_input()
    ref, raw, off, nout, ze = sc.corr_reference(S, K, mode)
    out = corr(dw, S, K, off, nout, ze)
    inner = slice(1, -1) if mode == "valid" else slice(None)
    assert np.all(np.isnan(out[1, inner])) and np.all(np.isnan(ref[1, inner]))
    if mode == "valid":
        assert out[1, 0] == 0 and out[1, -1] == 0
    assert sc.corr_error(out[[0, 2]], ref[[0, 2]], raw[[0, 2]]) <= sc.TOL


def public_call(dw, S2d, K, mode):
    """detect.xcorr2d / detect.xcorr on one [nf, nt] device spectrogram."""
    nk, nt = K.shape[1], S2d.shape[1]
    if mode == "same":
        out = dw.detect.xcorr2d(cuda(S2d), K)
    else:
        t = np.arange(nt) * 0.04
        ts, out = dw.detect.xcorr(t, np.arange(K.shape[0]), cuda(S2d), np.arange(nk), np.arange(K.shape[0]), K)
        assert np.array_equal(ts, t[int(nk / 2) - 1:-int(np.ceil(nk / 2))])
    assert out.is_cuda and out.dtype == torch.float32
    return out.cpu().numpy()[None]


@pytest.mark.parametrize("mode", sc.MODES)
def test_correlation_negative_median(dw, mode):
    """A dB spectrogram: xcorr2d clips and then divides by the negative median (values <= 0), xcorr divides and then clips
    (values >= 0) -- through the internal entry and through the public functions."""
    S, K = sc.negative_median_input()
    ref, raw, off, nout, ze = sc.corr_reference(S, K, mode)
    assert (ref.max() <= 0 and ref.min() < 0) if mode == "same" else (ref.min() >= 0 and ref.max() > 0)
    out = corr(dw, S, K, off, nout, ze)
    err = sc.corr_error(out, ref, raw)
    print("negative median, %s: output in [%.3f, %.3f], reference in [%.3f, %.3f], error %.3e"
          % (mode, out.min(), out.max(), ref.min(), ref.max(), err))
    assert err <= sc.TOL
    for c in range(S.shape[0]):
        assert np.array_equal(public_call(dw, S[c], K, mode)[0], out[c])


@pytest.mark.parametrize("nk", [126, 766, 2046])
@pytest.mark.parametrize("mode", sc.MODES)
def test_xcorr2d_and_xcorr_public_functions_exact(dw, nk, mode):
    """The longest kernel of each form through detect.xcorr2d / detect.xcorr, on the exact integer inputs."""
    S, K = sc.exact_input(nk, 3, 2100)
    ref, _, _, _ = sc.exact_reference(S, K, mode)
    for c in range(2):
        u = sc.ulp_error(public_call(dw, S[c], K, mode), ref[c:c + 1])
        print("%s nk=%d row %d: %.2f ulp" % ("xcorr2d" if mode == "same" else "xcorr", nk, c, u))
        assert u <= 1.0


def test_nxcorr2d_odd_kernel(dw):
    """detect.nxcorr2d (reference detect.py:544-576: correlate(S, K, 'same') / (std(S) std(K) nt), max over frequency) with an
    odd kernel length, restated in float64 with the direct method."""
    S, K = sc.real_input(21, 5, 513)
    S2, K2 = S[0].astype(np.float64), K[1:4].astype(np.float64)              # 5 x 513 against 3 x 21
    ref = np.max(sps.correlate(S2, K2, mode="same", method="direct") / (np.std(S2) * np.std(K2) * S2.shape[1]), axis=0)
    out = dw.detect.nxcorr2d(cuda(S[0]), K2).cpu().numpy()
    err = float(np.max(np.abs(out - ref)) / np.max(np.abs(ref)))
    print("nxcorr2d 5x513 * 3x21: error %.3e" % err)
    assert out.shape == ref.shape and err <= sc.TOL


def test_median_detector_rows(dw):
    v = sc.detector_rows()
    assert np.array_equal(median(dw, v), sc.median_reference(v))
    vo = np.ascontiguousarray(v[:, :-1])                                     # odd count
    assert np.array_equal(median(dw, vo), sc.median_reference(vo))


@pytest.mark.parametrize("n", sc.MEDIAN_N)
def test_median_row_kinds(dw, n):
    v = sc.median_rows(n)
    med, ref = median(dw, v), sc.median_reference(v)
    assert np.array_equal(med, ref), (n, np.flatnonzero(med != ref), med, ref)


def test_median_many_rows_one_launch(dw):
    v = sc.median_many_rows()
    med, ref = median(dw, v), sc.median_reference(v)
    assert np.array_equal(med, ref), np.flatnonzero(med != ref)


def stft(dw, xt, n_fft, hop, lo, hi, want_max):
    """dsp._stft_mag, and the same call on an output prefilled with NaN: the same bits, and no NaN left."""
    from das4whales_amd import _device as dev
    from das4whales_amd._lib import check, lib
    S, mx = dw.dsp._stft_mag(xt, n_fft, hop, lo, hi, want_max=want_max)
    assert (mx is not None) == want_max and S.is_cuda and S.dtype == torch.float32
    S2 = torch.full_like(S, float("nan"))
    mx2 = torch.full_like(mx, float("nan")) if want_max else None
    with torch.cuda.device(xt.device):
        check(lib.d4w_stft_mag_f32(dev.ptr(xt), dev.ptr(S2), dev.ptr(mx2) if want_max else None, xt.shape[0], xt.shape[1],
                                   n_fft, hop, lo, hi, dev.stream_ptr(xt)))
    S, S2 = S.cpu().numpy(), S2.cpu().numpy()
    assert not np.isnan(S2).any() and np.array_equal(S, S2)
    if want_max:
        mx, mx2 = mx.cpu().numpy(), mx2.cpu().numpy()
        assert np.array_equal(mx, mx2)
    return S, mx


@pytest.mark.parametrize("name", sorted(sc.STFT_CASES))
def test_stft_forms_and_edges(dw, name):
    from das4whales_amd._lib import lib
    n_fft, hop, nx, ns, lo, hi, want_max = sc.STFT_CASES[name]
    xt = cuda(sc.stft_case_input(name))
    mm = (not want_max) and lib.d4w_stft_mm_eligible(n_fft, hop, lo, hi) == 1
    assert mm == name.startswith("mm-"), "the table's matrix-core cases are the eligible ones"
    S, mx = stft(dw, xt, n_fft, hop, lo, hi, want_max)
    err = sc.stft_error(S, name)
    print("stft %s (%s): error / full maximum %.3e" % (name, "matrix cores" if mm else "FFT", err))
    assert err <= (sc.MM_TOL if mm else sc.TOL)
    if want_max:
        _, full_max = sc.stft_reference(name)
        assert np.all(np.abs(mx - full_max) <= sc.TOL * full_max)
        lo2, hi2 = sc.stft_slice(name)
        if (lo, hi) == (0, n_fft // 2) and lo2 <= hi2:
            S2, mx2 = stft(dw, xt, n_fft, hop, lo2, hi2, True)
            assert np.array_equal(S2, S[:, lo2:hi2 + 1]) and np.array_equal(mx2, mx)
