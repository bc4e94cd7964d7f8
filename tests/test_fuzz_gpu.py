"""Seeded random-shape sweep of every row of SURVEY 8(a) on the GPU against SciPy / the oracle:
ragged and odd shapes, prime factors, tiny inputs, rows of zeros / constants.  Complements the
golden-vector and full-size tests with breadth."""
import os

import numpy as np
import pytest
import scipy.signal as sps
import torch

from oracle import d4w_oracle as orc

SEED = int(os.environ.get("D4W_FUZZ_SEED", "0"))      # a different seed offset = a different set of random cases (stress runs)
pytestmark = pytest.mark.gpu
TOL = 1e-5
FS = 200.0


def rel(y, ref):
    d = np.max(np.abs(np.asarray(y, dtype=np.float64) - ref))
    s = np.max(np.abs(ref))
    return float(d / s) if s > 0 else float(d)


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available()
    import das4whales_amd as dw_
    return dw_


def smooth_lengths(rng, n, lo, hi, even=False):
    """Random lengths whose prime factors are <= 31 (what the transforms support)."""
    out = []
    while len(out) < n:
        v = int(rng.integers(lo, hi))
        if even and v % 2:
            v += 1
        m = v
        for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31):
            while m % p == 0:
                m //= p
        if m == 1:
            out.append(v)
    return out


def test_fk_filter_random_shapes(dw):
    rng = np.random.default_rng(101 + SEED)
    for nx, ns in zip(smooth_lengths(rng, 6, 2, 400), smooth_lengths(rng, 6, 4, 3000, even=True)):
        x = rng.standard_normal((nx, ns))
        m = rng.random((nx, ns)) * (rng.random((nx, 1)) > 0.3)          # some all-zero wavenumber rows
        ref = orc.fk_filter_filt(x, m)
        assert rel(dw.dsp.fk_filter_filt(x, m), ref) < TOL, (nx, ns)
        assert rel(dw.dsp.fk_filter_filt(x, m, tapering=True), orc.fk_filter_filt(x, m, tapering=True)) < TOL, (nx, ns)


def test_bandpass_random_shapes(dw):
    rng = np.random.default_rng(102 + SEED)
    for _ in range(5):
        nx, ns = int(rng.integers(1, 300)), int(rng.integers(60, 20000))
        x = rng.standard_normal((nx, ns)) + rng.standard_normal((nx, 1)) * 3
        lo = float(rng.uniform(5, 20))
        hi = lo + float(rng.uniform(5, 40))
        # ground truth = the float64 second-order-section filter with filtfilt's padlen; the reference's
        # 17-coefficient `ba` form (dsp.py:878-879) agrees with it to ~1e-7 for well-conditioned bands
        # (14-30 Hz) but is itself several 1e-5 off for narrow low bands, in float64
        sos = sps.butter(8, [lo / (FS / 2), hi / (FS / 2)], "bp", output="sos")
        truth = sps.sosfiltfilt(sos, x, axis=1, padlen=51)
        assert rel(dw.dsp.bp_filt(x, FS, lo, hi), truth) < TOL, (nx, ns, lo, hi)
        if SEED == 0 and not int(os.environ.get("D4W_SEED_SHIFT", "0")):       # the reference's own `ba` form: fine for the pinned cases, unstable for some random narrow low bands
            assert rel(orc.bp_filt(x, FS, lo, hi), truth) < 2e-4     # (other seeds: 3.7e-4, and 0.2 for a 5-Hz-wide band at 6 Hz)
        sos = dw.dsp.butterworth_filter([int(rng.integers(1, 6)), float(rng.uniform(2, 40)), "hp"], FS)
        assert rel(dw.dsp.sosfiltfilt(sos, x, axis=1), sps.sosfiltfilt(sos, x, axis=1)) < TOL


def test_matched_filter_random_shapes(dw):
    rng = np.random.default_rng(103 + SEED)
    for _ in range(6):
        nx, ns = int(rng.integers(1, 200)), int(rng.integers(200, 30000))
        x = rng.standard_normal((nx, ns)) + 0.2
        if nx > 2:
            x[1] = 0.0                                                   # all-zero row -> zeros (documented)
        L = int(rng.integers(3, min(161, ns // 2)))                       # (np.hanning(2) is all zeros)
        tpl = np.zeros(ns)
        tpl[:L] = rng.standard_normal(L) * np.hanning(L)
        c = dw.detect.compute_cross_correlogram(x, tpl)
        keep = [r for r in range(nx) if np.any(x[r] != 0)]
        ref = orc.compute_cross_correlogram(x[keep], tpl)
        assert rel(c[keep], ref) < TOL, (nx, ns, L)                   # incl. the zero-padded template's DC tail
        if nx > 2:
            assert np.all(c[1] == 0)
        # long second operand: direct form
        y = rng.standard_normal(ns)
        assert rel(dw.detect.shift_xcorr(x[0], y), orc.shift_xcorr(x[0], y)) < TOL
        assert rel(dw.detect.shift_nxcorr(x[0], y), orc.shift_nxcorr(x[0], y)) < TOL


def test_matrix_core_correlator_random_cases(dw):
    """csrc/xcorr_mm.hip over random shapes: supports 1..1100 (fused two-template kernel up to 177, the one-template kernels
    of 6 / 8 / 12 / 16 k-steps up to 497 in one launch, 496-tap sections that accumulate beyond -- VERDICT r04 #3: supports
    242 .. 1024), template pairs in both orders, single templates, rows of any length and alignment (templates longer than the
    row too), rows with a large offset, against a float64 correlation."""
    import torch
    rng = np.random.default_rng(2024 + SEED)
    for it in range(14):
        nx, ns = int(rng.integers(1, 60)), int(rng.integers(30, 20000))
        lmax = min(1100 if it % 2 else 241, ns)
        L0, L1 = int(rng.integers(1, lmax + 1)), int(rng.integers(1, lmax + 1))
        if it == 1:
            L0, L1 = min(450, ns), min(1024, ns)
        x = rng.standard_normal((nx, ns)) * float(10.0 ** rng.integers(-3, 4)) + float(rng.standard_normal()) * 5.0
        taps = [rng.standard_normal(L0) * np.hanning(L0 + 2)[1:-1], rng.standard_normal(L1)]
        if it % 3 == 0:
            taps = taps[:1]
        xd = torch.from_numpy(x.astype(np.float32)).cuda()
        # the library's own row statistics against a float64 de-meaning, as the reference does it (detect.py:157): the row
        # means are float64 and enter the kernels as two-float values, so an offset a thousand times the signal (one float32
        # ulp of such a mean is 1e-5 of the de-meaned row) costs nothing
        ym = dw.detect._xcorr_device(xd, taps, normalize=True, method="mm")
        x64 = xd.double().cpu().numpy()
        xn = (x64 - x64.mean(axis=1, keepdims=True)) / np.abs(x64).max(axis=1, keepdims=True)
        for k, tp in enumerate(taps):
            ref = np.stack([np.correlate(np.concatenate((r, np.zeros(len(tp) - 1))), tp, "valid") for r in xn])
            e = rel(ym[k].cpu().numpy(), ref)
            assert e < 3e-6, (nx, ns, L0, L1, k, e)
        yr = dw.detect._xcorr_device(xd, taps, normalize=False, method="mm")          # per-chunk power-of-two scale
        for k, tp in enumerate(taps):
            ref = np.stack([np.correlate(np.concatenate((r, np.zeros(len(tp) - 1))), tp, "valid") for r in x64])
            assert rel(yr[k].cpu().numpy(), ref) < 3e-6, (nx, ns, L0, L1, k, "raw")
    with pytest.raises(ValueError):
        dw.detect._xcorr_device(xd, [rng.standard_normal(16 * 496 + 1)], normalize=True, method="mm")


def test_detector_stft_random_cases(dw):
    """csrc/stft_mm.hip (the detector's STFT on the matrix cores) over random rows: eligible (n_fft, hop, bins) against the
    float64 restatement of librosa.stft; ineligible parameters keep running the FFT kernels."""
    import torch
    rng = np.random.default_rng(77 + SEED)
    for n_fft, hop in ((160, 8), (128, 8), (160, 16), (96, 24), (64, 32), (160, 8)):
        nx, ns = int(rng.integers(1, 40)), int(rng.integers(n_fft, 15000))
        nb = int(rng.integers(1, 17))
        lo = int(rng.integers(0, n_fft // 2 + 2 - nb))
        hi = lo + nb - 1
        x = rng.standard_normal((nx, ns)) * float(10.0 ** rng.integers(-2, 3))
        xd = torch.from_numpy(x.astype(np.float32)).cuda()
        S, mx = dw.dsp._stft_mag(xd, n_fft, hop, lo, hi, want_max=False)
        assert mx is None
        S = S.cpu().numpy()
        for c in range(0, nx, max(1, nx // 4)):
            ref = np.abs(orc.librosa_stft(xd[c].double().cpu().numpy(), n_fft=n_fft, hop_length=hop))
            assert np.max(np.abs(S[c] - ref[lo:hi + 1])) < 3e-6 * np.abs(ref).max(), (n_fft, hop, lo, hi, ns)


def test_analytic_and_snr_random_shapes(dw):
    rng = np.random.default_rng(104 + SEED)
    for ns in smooth_lengths(rng, 4, 16, 30000, even=True) + smooth_lengths(rng, 2, 15, 15000) + [120000 // 2, 2 * 3 * 5 * 7 * 11 * 13]:
        nx = int(rng.integers(1, 40))
        x = rng.standard_normal((nx, ns))
        z = orc.hilbert(x)
        assert rel(dw.dsp.envelope(x), np.abs(z)) < TOL, ns
        if ns % 2 == 0:
            s = dw.dsp.snr_tr_array(x, env=True)
            lin, ref = 10.0 ** (s / 10), np.abs(z) ** 2 / np.var(x, axis=1, keepdims=True)
            assert np.max(np.abs(lin - ref)) / np.max(ref) < TOL, ns


def test_spectrogram_random_parameters(dw):
    rng = np.random.default_rng(105 + SEED)
    for _ in range(6):
        ns = int(rng.integers(300, 20000))
        nfft = int(rng.choice([32, 64, 100, 128, 160, 256, 500, 512, 1024, 148, 202]))     # 148 = 4 x 37, 202 = 2 x 101: Bluestein frames
        ov = float(rng.choice([0.5, 0.75, 0.8, 0.9, 0.95]))
        x = rng.standard_normal(ns)
        p, tt, ff = dw.dsp.get_spectrogram(x, FS, nfft=nfft, overlap_pct=ov)
        pr, ttr, ffr = orc.get_spectrogram(x, FS, nfft=nfft, overlap_pct=ov)
        assert p.shape == pr.shape and np.allclose(tt, ttr) and np.allclose(ff, ffr)
        assert np.max(np.abs(10.0 ** (p / 20) - 10.0 ** (pr / 20))) < TOL, (ns, nfft, ov)
        nfx = int(rng.choice([64, 300, 512, 1000, 4096]))
        xm = rng.standard_normal((int(rng.integers(1, 50)), int(rng.integers(10, 900))))
        assert rel(dw.dsp.get_fx(xm, nfx), orc.get_fx(xm, nfx)) < TOL


def test_spectrocorr_random_parameters(dw):
    rng = np.random.default_rng(106 + SEED)
    for _ in range(4):
        nx, ns = int(rng.integers(1, 60)), int(rng.integers(3000, 16000))
        x = rng.standard_normal((nx, ns))
        win = float(rng.choice([0.4, 0.64, 0.8]))
        ov = float(rng.choice([0.9, 0.95]))
        ker = {"f0": 27., "f1": 17., "dur": float(rng.choice([0.6, 0.8, 1.0])), "bdwidth": float(rng.choice([3., 4.]))}
        sc = dw.detect.compute_cross_correlogram_spectrocorr(x, FS, [14., 30.], ker, win, ov)
        ref = orc.compute_cross_correlogram_spectrocorr(x, FS, [14., 30.], ker, win, ov)
        assert sc.shape == ref.shape and rel(sc, ref) < TOL, (nx, ns, win, ov)


def test_picks_random_rows(dw):
    rng = np.random.default_rng(107 + SEED)
    for ns in (3, 4, 64, 65, 1000, 16384, 16385, 50001):
        nx = int(rng.integers(1, 30))
        x = rng.standard_normal((nx, ns)).astype(np.float32)
        x[0] = np.round(x[0] * 2) / 2                                    # plateaus
        if nx > 1:
            x[1] = 1.0                                                   # constant row
        if nx > 2:
            x[2] = np.abs(sps.hilbert(x[2].astype(np.float64))).astype(np.float32) if ns > 8 else x[2]
        for thr in (0.0, 0.5, 2.0, 1e9):
            got = dw.detect.pick_times(x, thr)
            for c in range(nx):
                ref = sps.find_peaks(x[c].astype(np.float64), prominence=thr)[0]
                assert np.array_equal(got[c], ref), (ns, thr, c)


def test_channel_counts_with_large_prime_factors(dw):
    """nx with a prime factor > 31 (any channel selection): pass C runs its Bluestein form."""
    rng = np.random.default_rng(108 + SEED)
    for nx, ns in ((4001, 600), (37 * 2, 64), (2 * 3 * 211, 1200), (1009, 256)):
        x = rng.standard_normal((nx, ns))
        m = rng.random((nx, ns))
        assert rel(dw.dsp.fk_filter_filt(x, m), orc.fk_filter_filt(x, m)) < TOL, (nx, ns)
    sel = [0, 4001, 1]
    x = rng.standard_normal((4001, 1200))
    mask = dw.dsp.hybrid_ninf_filter_design((4001, 1200), sel, 2.04, FS, cs_min=1350., cp_min=1450., cp_max=3300, cs_max=3450,
                                            fmin=14., fmax=30.)
    ref = orc.fk_filter_filt(x, orc.hybrid_ninf_filter_design((4001, 1200), sel, 2.04, FS, cs_min=1350., cp_min=1450.,
                                                              cp_max=3300, cs_max=3450, fmin=14., fmax=30.))
    assert rel(dw.dsp.fk_filter_sparsefilt(x, mask), ref) < TOL


def test_row_lengths_with_large_prime_factors(dw):
    """Analytic-signal rows whose transform has a prime factor > 31 (12002 = 2 x 6001): Bluestein row transform."""
    rng = np.random.default_rng(109 + SEED)
    for nx, ns in ((5, 12002), (3, 2 * 1009), (4, 1091)):
        x = rng.standard_normal((nx, ns))
        z = orc.hilbert(x)
        assert rel(dw.dsp.envelope(x), np.abs(z)) < TOL, ns
        assert rel(dw.dsp.hilbert_imag(x), z.imag) < TOL, ns
    c = rng.standard_normal((6, 12002)).astype(np.float32)
    got = dw.detect.pick_times_env(c, 2.5)
    env = np.abs(orc.hilbert(c.astype(np.float64)))
    for r in range(6):
        ref = sps.find_peaks(env[r], prominence=2.5)[0]
        pr = sps.peak_prominences(env[r], np.union1d(ref, got[r]).astype(int))[0] if len(ref) or len(got[r]) else []
        sym = np.setxor1d(ref, got[r])
        assert all(abs(p - 2.5) < 1e-3 for p in sps.peak_prominences(env[r], sym.astype(int))[0]), (r, sym)


def test_spectrogram_windows_with_large_prime_factors(dw):
    """STFT windows with a prime factor > 31 (e.g. a 0.74-s window at 200 Hz = 148 samples): Bluestein frame transform."""
    rng = np.random.default_rng(110 + SEED)
    x = rng.standard_normal(9000)
    for nfft, ov in ((148, 0.9), (202, 0.8), (2 * 67, 0.95)):
        p, tt, ff = dw.dsp.get_spectrogram(x, FS, nfft=nfft, overlap_pct=ov)
        pr, ttr, ffr = orc.get_spectrogram(x, FS, nfft=nfft, overlap_pct=ov)
        assert p.shape == pr.shape
        assert np.max(np.abs(10.0 ** (p / 20) - 10.0 ** (pr / 20))) < TOL, nfft
    xm = rng.standard_normal((7, 6000))
    ker = {"f0": 27., "f1": 17., "dur": 0.8, "bdwidth": 4.}
    sc = dw.detect.compute_cross_correlogram_spectrocorr(xm, FS, [14., 30.], ker, 0.74, 0.95)      # nperseg = 148
    ref = orc.compute_cross_correlogram_spectrocorr(xm, FS, [14., 30.], ker, 0.74, 0.95)
    assert sc.shape == ref.shape and rel(sc, ref) < TOL


def test_any_channel_count(dw):
    """Channel counts whose part with prime factors > 31 exceeds 4096 (the LDS Bluestein tile of pass C): the plan runs the
    global-memory Bluestein form of the channel transform (fk_dist.hip: fkd_bz_*) -- numpy.fft.fft2 (dsp.py:748) takes any
    shape.  Dense, designed and fk_filt masks, taper, in several scratch chunks."""
    rng = np.random.default_rng(111 + SEED)
    for nx, ns in ((4099, 64), (2 * 5003, 240), (10007, 1200)):
        x = rng.standard_normal((nx, ns))
        m = rng.random((nx, ns))
        assert rel(dw.dsp.fk_filter_filt(x, m), orc.fk_filter_filt(x, m)) < TOL, (nx, ns)
    assert rel(dw.dsp.fk_filter_filt(x, m, tapering=True), orc.fk_filter_filt(x, m, tapering=True)) < TOL
    nx, ns = 8209, 1200
    sel = [0, nx, 1]
    x = rng.standard_normal((nx, ns))
    kw = dict(cs_min=1350., cp_min=1450., cp_max=3300, cs_max=3450, fmin=14., fmax=30.)
    mask = dw.dsp.hybrid_ninf_filter_design((nx, ns), sel, 2.04, FS, **kw)
    ref = orc.fk_filter_filt(x, orc.hybrid_ninf_filter_design((nx, ns), sel, 2.04, FS, **kw))
    assert rel(dw.dsp.fk_filter_sparsefilt(x, mask), ref) < TOL
    assert rel(dw.dsp.fk_filt(x, 1, FS, 1, 2.04, 1400., 3500.), orc.fk_filt(x, 1, FS, 1, 2.04, 1400., 3500.)) < TOL


def test_any_record_length(dw):
    """ns / 2 whose part with prime factors > 31 exceeds 2048 (pass B's Bluestein tile), odd record lengths that zero
    interleaving turns into such, and both axes at once: the global-memory Bluestein form of the time transform (fkd_bt_*)."""
    rng = np.random.default_rng(112 + SEED)
    for nx, ns in ((8, 2 * 4099), (300, 12014), (64, 6007), (4099, 2 * 2053)):      # 12014 = 2 x 6007; 6007 odd and prime
        x = rng.standard_normal((nx, ns))
        m = rng.random((nx, ns))
        assert rel(dw.dsp.fk_filter_filt(x, m), orc.fk_filter_filt(x, m)) < TOL, (nx, ns)
    assert rel(dw.dsp.fk_filter_filt(x, m, tapering=True), orc.fk_filter_filt(x, m, tapering=True)) < TOL
    # long analytic rows (beyond one workgroup's LDS) with a prime factor > 31, any row count
    x = rng.standard_normal((37, 2 * 20011))
    z = orc.hilbert(x)
    assert rel(dw.dsp.envelope(x), np.abs(z)) < TOL
    assert rel(dw.dsp.hilbert_imag(x), z.imag) < TOL
    # ... and odd ones (complex rows of their own length): a prime, 60 s + 1 sample (12001 = 11 x 1091), 10 min + 1 sample
    for nx, ns in ((3, 20011), (5, 12001), (2, 120001)):
        x = rng.standard_normal((nx, ns))
        z = orc.hilbert(x)
        assert rel(dw.dsp.envelope(x), np.abs(z)) < TOL, ns
        assert rel(dw.dsp.hilbert_imag(x), z.imag) < TOL, ns
    x = rng.standard_normal((4, 12001)) + 0.3
    ref = 10 * np.log10(np.abs(orc.hilbert(x)) ** 2 / np.var(x, axis=1)[:, None])
    got = dw.dsp.snr_tr_array(x, env=True)
    assert np.max(np.abs(10.0 ** (got / 10) - 10.0 ** (ref / 10))) / np.max(10.0 ** (ref / 10)) < TOL


def test_unsupported_length_is_a_clear_error(dw):
    """What is left without a kernel: get_fx / spectrogram transforms whose Bluestein tile exceeds a workgroup's LDS.
    ValueError, not a wrong answer.  (The f-k filter and the analytic signal take any shape.)"""
    assert dw.dsp.supported_length(4001) == 4000 and dw.dsp.supported_length(97, even=True) == 96
    x = np.random.default_rng(0 + SEED).standard_normal((8, 2 * 37))
    m = np.random.default_rng(1 + SEED).uniform(size=x.shape)
    assert np.max(np.abs(dw.dsp.fk_filter_filt(x, m) - orc.fk_filter_filt(x, m))) < 1e-5 * np.max(np.abs(x))
    with pytest.raises(ValueError):
        dw.dsp.get_fx(np.zeros((2, 400)), 2 * 10007)
