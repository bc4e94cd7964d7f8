"""Cases, inputs and float64 references of the spectrogram detector chain (STFT -> row median -> kernel x spectrogram
correlation, csrc/stft.hip, csrc/noise.hip, csrc/spectrocorr.hip and csrc/stft_mm.hip), shared by tests/test_emu_spectrocorr.py (CPU emulator, C ABI) and
tests/test_spectrocorr_gpu.py (Python interface on the device).

References are written as the reference package writes them, in float64 on inputs rounded to float32 first:
  'same'  (detect.xcorr2d, detect.py:597-600): fftconvolve(S, flip(K, 1), 'same', axes=1).sum(0), clip at 0, / (median * nk);
  'valid' (detect.xcorr, detect.py:632-645):   sum(K * S[:, i:i+nk]), / (median * nk), ends zeroed, clip at 0;
  np.median for the median; oracle.d4w_oracle.librosa_stft for the STFT.

The correlation kernel has three forms, chosen by the host from the kernel's length: spectro_corr<4,5> for nk <= 126,
<2,10> for nk <= 766 and <1,20> for nk <= 2046 (sc_width(nk) = (nk + 517) & ~3 against 640 / 1280 / 2560); nk = 2047 is
refused.  A strip row is read in 16-byte pieces, the last of which is needed only when nk + 2 is a multiple of 4
(nk = 2, 126, 130, 638, 1278, 2046), and the samples a <2,10> chunk cannot hold start at strip index 1280, which a lag
reaches from nk = 770 on: the exact cases carry those lengths.

Tolerances.  Real-valued inputs: the project's 1e-5 of max|ref| per row.  The long forms add up to 13 x 2046 products in
float32, which alone is 1e-5 of the maximum, so they are checked with integer inputs instead (S in 0..3, K in -2..2: every
partial sum is an integer below 13 * 2046 * 6 < 2^24 and float32 accumulation is exact in any order; the median is a small
integer or half-integer, so median * nk is exact too): the output must be the float64 quotient rounded to float32 to within
1 ulp, which a single dropped or shifted product misses by far.  Medians must equal np.median(float64) rounded to float32.
STFT: 1e-5 of the row's full-spectrogram maximum for the FFT forms, 2e-6 of it for the matrix-core form (as
tests/test_emu_spectral.py::test_stft_on_the_matrix_cores: 2e-6 x (max over all bins / max over kept bins) of the kept
maximum)."""
import functools

import numpy as np
import scipy.signal as sps

from oracle import d4w_oracle as orc

TOL = 1e-5
MM_TOL = 2e-6
NK_MAX = 2046                                      # the longest kernel d4w_spectrocorr_f32 accepts


def form_of(nk):
    """The kernel form the host picks for a kernel of nk frames."""
    w = (512 + nk + 5) & ~3
    return "<4,5>" if w <= 640 else "<2,10>" if w <= 1280 else "<1,20>"


def frozen(a):
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------------------------------------------------
# correlation: references
# ---------------------------------------------------------------------------------------------------------------------
def ref_same(S, K, med):
    """detect.xcorr2d on one spectrogram S [nf, nt] (float64): [nt], and the same before the clip."""
    raw = sps.fftconvolve(S, np.flip(K, axis=1), mode="same", axes=1).sum(axis=0)
    c = raw.copy()
    c[c < 0] = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        return c / (med * K.shape[1]), raw / (med * K.shape[1])


def ref_valid(S, K, med):
    """detect.xcorr on one spectrogram: [nt - nk + 1], and the same before the ends are zeroed and the clip."""
    nk = K.shape[1]
    win = np.lib.stride_tricks.sliding_window_view(S, nk, axis=1)          # [nf, nt - nk + 1, nk]
    with np.errstate(divide="ignore", invalid="ignore"):
        raw = np.einsum("fij,fj->i", win, K) / (med * nk)
    c = raw.copy()
    c[0] = 0
    c[-1] = 0
    c[c < 0] = 0
    return c, raw


def corr_reference(S, K, mode):
    """S [nx, nf, nt] float32, K [nf, nk] float32 -> (ref [nx, nout], unclipped ref, off, nout, zero_ends) in float64."""
    S64, K64 = S.astype(np.float64), K.astype(np.float64)
    f = ref_same if mode == "same" else ref_valid
    both = [f(S64[c], K64, np.median(S64[c])) for c in range(S.shape[0])]
    ref, raw = np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    nk, nt = K.shape[1], S.shape[2]
    return (ref, raw, nk // 2, nt, 0) if mode == "same" else (ref, raw, 0, nt - nk + 1, 1)


def corr_error(out, ref, raw):
    """max over rows of max|out - ref| / max|ref|.  A row whose reference is all zero (one or two valid lags, both forced
    to zero; a single clipped lag) is measured against the largest value before the clip instead."""
    out = np.asarray(out, dtype=np.float64)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    worst = 0.0
    for c in range(ref.shape[0]):
        den = np.max(np.abs(ref[c]))
        if den == 0:
            den = np.max(np.abs(raw[c]))
        assert np.all(np.isfinite(out[c])), c
        worst = max(worst, float(np.max(np.abs(out[c] - ref[c])) / den))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# correlation: real-valued cases (the <4,5> form and its upper boundary)
# ---------------------------------------------------------------------------------------------------------------------
REAL_NK = (1, 2, 3, 4, 5, 7, 20, 21, 125, 126)
REAL_NF = (1, 3, 4, 5, 13)                         # below, at and across the chunk of 4 strip rows, ragged last chunk
ROW_SCALES = (1.0, 1e3, 1e-3)                      # nx = 3: medians 1e3 apart
MODES = ("same", "valid")


def real_nt(nk):
    return sorted({1, nk - 1, nk, 511, 512, 513, 1025, 1537} - {0})


def real_cases(nk):
    """(nf, nt, mode) of one kernel length; 'valid' needs a lag."""
    return [(nf, nt, mode) for nf in REAL_NF for nt in real_nt(nk) for mode in MODES if mode == "same" or nt - nk + 1 >= 1]


@functools.lru_cache(maxsize=None)
def real_input(nk, nf, nt):
    rng = np.random.default_rng(100000 * nk + 10000 * nf + nt)
    S = (np.abs(rng.standard_normal((3, nf, nt))) + 0.1) * np.asarray(ROW_SCALES)[:, None, None]
    # Gaussian bumps whose centre drifts with frequency, all positive: no sum cancels, so 1e-5 of the row maximum is a bound
    # float32 can meet at every shape, a single lag included (signed kernels: the exact and the negative-median cases)
    j = np.arange(nk)[None, :]
    centre = rng.uniform(0, nk, nf)[:, None]
    K = rng.uniform(0.5, 1.5, nf)[:, None] * np.exp(-0.5 * ((j - centre) / (0.15 * nk + 0.5)) ** 2)
    return frozen(np.ascontiguousarray(S, dtype=np.float32)), frozen(np.ascontiguousarray(K, dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# correlation: exact integer cases (the long forms, every threshold and every last-piece length)
# ---------------------------------------------------------------------------------------------------------------------
# 2, 6, 126: <4,5> with a last piece of one needed sample, 126 its longest kernel; 127: first of <2,10>; 766 / 767: last of
# <2,10>, first of <1,20>; 2046: the longest; 130, 638, 1278, 2046: nk + 2 a multiple of 4 (the last 16-byte piece holds one
# needed sample); 770, 890: lags that reach strip index 1280 and beyond
EXACT_NK = (2, 6, 126, 127, 130, 637, 638, 639, 640, 765, 766, 767, 770, 890, 1277, 1278, 1279, 1500, 2044, 2045, 2046)
EXACT_NF = (1, 2, 3, 13)
EXACT_NT = (513, 2100)


@functools.lru_cache(maxsize=4)
def exact_input(nk, nf, nt):
    """S [2, nf, nt] integers 0..3 (row 1 with median 1.5 when the count is even), K [nf, nk] integers -2..2."""
    rng = np.random.default_rng(7 * nk + 1000003 * nf + nt)
    n = nf * nt
    S = rng.integers(0, 4, (2, n))
    if n % 2 == 0:
        lo, hi = rng.integers(0, 2, n // 2), rng.integers(2, 4, n // 2)
        lo[0], hi[0] = 1, 2                        # the two middle values: 1 and 2
        S[1] = rng.permutation(np.concatenate((lo, hi)))
    K = rng.integers(-2, 3, (nf, nk))
    return frozen(S.reshape(2, nf, nt).astype(np.float32)), frozen(K.astype(np.float32))


def exact_reference(S, K, mode, med=None):
    """The integer sums through a float64 FFT convolution (rounded back to the integers they are), then the reference's
    clip / divide order in float64.  Returns (ref float64 [nx, nout], off, nout, zero_ends)."""
    S64, K64 = S.astype(np.float64), K.astype(np.float64)
    nx, _, nt = S.shape
    nk = K.shape[1]
    out = []
    for c in range(nx):
        full = sps.fftconvolve(S64[c], np.flip(K64, axis=1), mode="full", axes=1).sum(axis=0)
        assert np.max(np.abs(full - np.rint(full))) < 1e-6
        full = np.rint(full)                       # full[m] = sum_f sum_j S[f][m - (nk - 1) + j] K[f][j]
        m = np.median(S64[c]) if med is None else float(med[c])
        assert m * 2 == np.rint(m * 2) or med is not None
        if mode == "same":
            r = full[(nk - 1) // 2:(nk - 1) // 2 + nt].copy()
            r[r < 0] = 0
            r /= m * nk
        else:
            r = full[nk - 1:nt].copy()
            r /= m * nk
            r[0] = 0
            r[-1] = 0
            r[r < 0] = 0
        out.append(r)
    ref = np.stack(out)
    return (ref, nk // 2, nt, 0) if mode == "same" else (ref, 0, nt - nk + 1, 1)


def ulp_error(out, ref):
    """Largest distance of the float32 output from the float64 reference rounded to float32, in units of its last place."""
    want = ref.astype(np.float32)
    out = np.asarray(out)
    assert out.dtype == np.float32 and out.shape == want.shape, (out.dtype, out.shape, want.shape)
    assert np.all(np.isfinite(out))
    return float(np.max(np.abs(out.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)))


# one impulse per form: S is a single 1 at (f, t0) with t0 next to a tile boundary of 512 lags, K a ramp of distinct
# positive integers, the divisor given as 1 (the median of such an S is 0): the output is K[f] reversed, / nk
IMPULSE_CASES = {"<4,5>": (21, 3, 1600, 1, 1030), "<2,10>": (300, 3, 1600, 2, 1100), "<1,20>": (1000, 3, 1600, 0, 1400)}


def impulse_input(form):
    nk, nf, nt, f, t0 = IMPULSE_CASES[form]
    assert form_of(nk) == form
    S = np.zeros((1, nf, nt), dtype=np.float32)
    S[0, f, t0] = 1.0
    K = (1.0 + np.arange(nf * nk, dtype=np.float32)).reshape(nf, nk)
    return S, K, np.ones(1, dtype=np.float32)


def impulse_expected(form, mode):
    """out[t] = K[f][t0 - t + off] / nk where that tap exists, else 0 (ends zeroed in 'valid')."""
    nk, nf, nt, f, t0 = IMPULSE_CASES[form]
    _, K, _ = impulse_input(form)
    off, nout = (nk // 2, nt) if mode == "same" else (0, nt - nk + 1)
    want = np.zeros(nout)
    for t in range(nout):
        j = t0 - t + off
        if 0 <= j < nk:
            want[t] = K[f, j] / nk
    if mode == "valid":
        want[0] = want[-1] = 0
    return want[None]


# ---------------------------------------------------------------------------------------------------------------------
# correlation: edge cases
# ---------------------------------------------------------------------------------------------------------------------
NAN_CASE = (21, 5, 2000, 2, 1000)                  # nk, nf, nt, (f, t) of the NaN


def nan_input():
    nk, nf, nt, f, t = NAN_CASE
    S, K = real_input(nk, nf, nt)
    S = S[:1].copy()
    clean = S.copy()
    S[0, f, t] = np.nan
    clean[0, f, t] = 0.0                           # no lag outside the window sees this sample
    return S, clean, K, np.asarray([np.median(clean[0].astype(np.float64))], dtype=np.float32)


def nan_lags(mode):
    """The nk lags whose window holds sample t."""
    nk, _, _, _, t = NAN_CASE
    off = nk // 2 if mode == "same" else 0
    return np.arange(t + off - nk + 1, t + off + 1)


def zero_row_input():
    """Row 1 of three is all zero: its median is 0 and every lag 0 / 0."""
    S, K = real_input(21, 5, 513)
    S = S.copy()
    S[1] = 0.0
    return S, K


def negative_median_input():
    """A spectrogram in dB below its maximum, as dsp.get_spectrogram returns it: every value and the median negative."""
    rng = np.random.default_rng(4242)
    S = 20.0 * np.log10((np.abs(rng.standard_normal((3, 5, 700))) + 1e-3) / 6.0)
    assert S.max() < 0
    K = rng.standard_normal((5, 21))
    return np.ascontiguousarray(S, dtype=np.float32), np.ascontiguousarray(K, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# median
# ---------------------------------------------------------------------------------------------------------------------
def detector_rows(n=19514, seed=99):
    """The seven row kinds of tests/test_emu_spectral.py::test_row_median_even_counts_and_narrow_rows, n even."""
    rng = np.random.default_rng(seed)
    rows = [np.abs(rng.standard_normal(n)) * rng.uniform(0.5, 2.0, n),      # spread over octaves
            1.0 + 0.05 * rng.random(n),                                      # one quarter-octave bin holds the whole row
            np.concatenate((np.full(n // 2, 1.0), np.full(n // 2, 1.5))),    # lower middle the last 1.0, upper middle 1.5
            np.concatenate((np.full(n // 2, 1.0), 1e6 + rng.random(n // 2))),   # upper middle many bins above
            np.full(n, -3.25),
            -np.abs(rng.standard_normal(n)),
            np.concatenate((rng.random(n // 2 - 1) * 0.5, [0.75], 4.0 + rng.random(n // 2)))]   # lower middle alone in its bin
    return frozen(np.stack([rng.permutation(r) for r in rows]).astype(np.float32))


MEDIAN_N = (1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4096)      # 2048 = one sweep step of 8 loads x 256 threads
NEG_NAN_DIGIT0, NEG_NAN_DIGIT1 = 0xFFFFFFFF, 0xFFC00000          # keys 0x00000000 and 0x003FFFFF: top digits 0 and 1


def _bits(u):
    return np.asarray([u], dtype=np.uint32).view(np.float32)[0]


def row_kinds(n, rng):
    """Every row kind that exists at length n, as float32 rows.

    The kernel keeps a private histogram of the four top-digit bins from (first value's bin - 1) on.  The bin is 0 or 1
    -- so that the -1 wraps or lands on bin 0 -- only for a first value that is a negative NaN: -inf has top digit 3 and
    -FLT_MAX 4.  The kernel is an order statistic of the keys, under which a negative NaN sorts below -inf; rows that
    start with one are therefore expected to give the median of the row with -inf in its place (median_reference).  They
    exist from n = 3 on, where the middle is not the NaN itself."""
    a, b = n // 2, n - n // 2
    g = rng.standard_normal
    rows = [g(n),
            np.abs(g(n)) * rng.uniform(0.5, 2.0, n),
            1.0 + 0.05 * rng.random(n),
            rng.permutation(np.concatenate((np.full(a, 1.0), np.full(b, 1.5)))),
            rng.permutation(np.concatenate((np.full(a, 1.0), 1e6 + rng.random(b)))),
            np.full(n, -3.25),
            -np.abs(g(n)),
            np.round(g(n) * 2) / 2,                                          # many duplicates
            rng.choice(np.asarray([-1.5, -0.0, 0.0, 2.0, -1e-3, 1e-3, -0.0, 0.0]), n),   # both zeros among both signs
            (rng.integers(1, 1 << 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)).view(np.float32)]  # denormals
    lo, hi = g(n), g(n)
    i, j = int(np.argmin(lo)), int(np.argmax(hi))
    lo[[0, i]] = lo[[i, 0]]                                                  # the first value's bin is the lowest ...
    hi[[0, j]] = hi[[j, 0]]                                                  # ... and the highest occupied one
    rows += [lo, hi]
    if n >= 8:
        v = g(n)
        v[rng.permutation(n)[:n // 4]] = np.inf                              # away from the middle: the median is finite
        v[rng.permutation(n)[:n // 4]] = -np.inf
        rows.append(v)
    if n >= 3:
        for first in (-np.inf, -np.finfo(np.float32).max, _bits(NEG_NAN_DIGIT1), _bits(NEG_NAN_DIGIT0)):
            v = g(n).astype(np.float32)
            v[0] = first
            rows.append(v)
    return np.stack([np.asarray(r, dtype=np.float32) for r in rows])


@functools.lru_cache(maxsize=None)
def median_rows(n):
    return frozen(row_kinds(n, np.random.default_rng(5000 + n)))


@functools.lru_cache(maxsize=None)
def median_many_rows(nx=300, n=2050):
    """nx rows of different kinds and scales (powers of two) for one launch."""
    rng = np.random.default_rng(300)
    rows = []
    with np.errstate(over="ignore"):               # -FLT_MAX times a power of two is -inf: another row that starts at the lowest bin
        while len(rows) < nx:
            for r in row_kinds(n, rng):
                rows.append(r * np.float32(2.0 ** int(rng.integers(-8, 9))))
    return frozen(np.stack(rows[:nx]))


def median_reference(v):
    """np.median(float64) per row rounded to float32; a leading negative NaN counts as below -inf (row_kinds)."""
    v64 = v.astype(np.float64)
    v64[np.isnan(v64)] = -np.inf
    return np.median(v64, axis=1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# STFT: one row of the table per dispatch form and edge
# ---------------------------------------------------------------------------------------------------------------------
FAT = (128, 160, 256, 512)                         # stft_fat<RA,16>


def _stft_table():
    T = {}

    def add(tag, n_fft, hop, ns, lo=0, hi=None, want_max=True, nx=3):
        hi = n_fft // 2 if hi is None else hi
        name = "%s-%d_%d-ns%d-bins%d_%d-%s" % (tag, n_fft, hop, ns, lo, hi, "max" if want_max else "nomax")
        assert name not in T
        T[name] = (n_fft, hop, nx, ns, lo, hi, want_max)

    # every frame length class at hop 8: 64 radix-2 only, 100 generic radices, 148 = 4 x 37 and 202 = 2 x 101 Bluestein.
    # ns = 1, 7: one frame, nb clamped by the frame count; ns < n_fft / 2: every frame hangs over both row ends
    for n_fft in FAT + (64, 100, 148, 202):
        for ns in (1, 7, n_fft // 2 - 1, 3 * n_fft + 5):
            add("all", n_fft, 8, ns)
            if n_fft in FAT:
                add("kept", n_fft, 8, ns, 0, n_fft // 2, want_max=False)                     # every bin, no row maximum
                add("kept", n_fft, 8, ns, n_fft // 2 - 20, n_fft // 2, want_max=False)       # 21 bins up to Nyquist
    # the matrix-core form: no row maximum, <= 16 kept bins, with DC and with Nyquist
    for ns in (1, 7, 79, 485, 3001):
        add("mm", 160, 8, ns, 0, 15, want_max=False)
        add("mm", 160, 8, ns, 68, 80, want_max=False)
        add("mm", 128, 16, ns, 49, 64, want_max=False)
        add("mm", 128, 16, ns, 0, 0, want_max=False)
    # large hops: the segment of a tile is longer than the 4 x 256 samples that travel in registers
    for n_fft in (160, 256):
        add("hop40", n_fft, 40, 3000)                                                      # seg_len 31 * 40 + n_fft > 1024
        add("hop40", n_fft, 40, 3000, 3, 30, want_max=False)
    add("hop_gt_frame", 128, 128 + 37, 3000)                                               # samples no frame covers
    add("hop_gt_frame", 160, 160 + 37, 3000, 0, 20, want_max=False)
    add("hop_gt_frame", 100, 100 + 37, 3000)
    add("hop700", 512, 700, 3000)
    add("hop700", 160, 700, 3000, 60, 80, want_max=False)
    add("hop700", 202, 700, 3000)
    add("hop4000", 160, 4000, 30000)
    add("hop4000", 100, 4000, 30000)
    add("hop4000", 148, 4000, 30000)
    # more rows than workgroups per row allow: 4100 rows -> one workgroup walks the three tiles of its row with the next
    # tile's samples in registers; 2049 rows -> three workgroups for four tiles
    add("tile_walk", 160, 8, 600, 0, 16, nx=4100)
    add("tile_walk", 160, 8, 600, 0, 16, want_max=False, nx=4100)
    add("tile_walk", 256, 12, 1500, 120, 128, nx=2049)
    add("tile_walk", 256, 12, 1500, 120, 128, want_max=False, nx=2049)
    return T


STFT_CASES = _stft_table()
# a tile walk needs more than 4096 rows, and the emulator, which sets up 256 fibers per workgroup and runs one workgroup at
# a time, needs 9-18 s for any such launch whatever the row length: the walks run on the device only
STFT_EMU_CASES = {k: v for k, v in STFT_CASES.items() if not k.startswith("tile_walk")}


@functools.lru_cache(maxsize=8)
def stft_input(nx, ns, seed):
    """Gaussian rows with scales 1, 300 and 1e-3 and one DC offset, as test_stft_on_the_matrix_cores."""
    rng = np.random.default_rng(seed)
    scale = np.asarray([1.0, 300.0, 1e-3])[np.arange(nx) % 3]
    offset = np.asarray([0.0, 50.0, 0.0])[np.arange(nx) % 3]
    return frozen(np.ascontiguousarray(rng.standard_normal((nx, ns)) * scale[:, None] + offset[:, None], dtype=np.float32))


def stft_case_input(name):
    n_fft, hop, nx, ns, _, _, _ = STFT_CASES[name]
    return stft_input(nx, ns, 1000 * n_fft + hop)


def _stft_rows(x, n_fft, hop):
    """oracle.d4w_oracle.librosa_stft (periodic Hann, center=True with zero padding, 1 + ns // hop frames) of every row of x
    at once: the same arithmetic in float64, checked against the oracle itself on the first row."""
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    xp = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)))
    idx = np.arange(n_fft)[:, None] + hop * np.arange(1 + x.shape[1] // hop)[None, :]
    return np.abs(np.fft.rfft(xp[:, idx] * win[None, :, None], axis=1))


@functools.lru_cache(maxsize=8)
def _stft_reference(n_fft, hop, nx, ns, lo, hi):
    x = stft_input(nx, ns, 1000 * n_fft + hop).astype(np.float64)
    kept = np.empty((nx, hi - lo + 1, 1 + ns // hop))
    full_max = np.empty(nx)
    for a in range(0, nx, 128):
        m = _stft_rows(x[a:a + 128], n_fft, hop)
        if a == 0:
            assert np.array_equal(m[0], np.abs(orc.librosa_stft(x[0], n_fft=n_fft, hop_length=hop)))
        kept[a:a + 128] = m[:, lo:hi + 1]
        full_max[a:a + 128] = m.reshape(m.shape[0], -1).max(axis=1)
    return frozen(kept), frozen(full_max)


def stft_reference(name):
    """(|librosa.stft| of the kept bins [nx, nkeep, nt], the maximum over all bins and frames [nx]) in float64."""
    n_fft, hop, nx, ns, lo, hi, _ = STFT_CASES[name]
    return _stft_reference(n_fft, hop, nx, ns, lo, hi)


def stft_error(S, name):
    """max over rows of max|S - ref| / (the row's maximum over ALL bins and frames); no NaN may be left."""
    kept, full_max = stft_reference(name)
    S = np.asarray(S, dtype=np.float64)
    assert S.shape == kept.shape, (name, S.shape, kept.shape)
    assert not np.isnan(S).any(), "%s: output values never written" % name
    nx = S.shape[0]
    return float(np.max(np.abs(S - kept).reshape(nx, -1).max(axis=1) / full_max))


def stft_slice(name):
    """A bin range without DC (where the offset row has its maximum) and without Nyquist for the 'all bins' cases."""
    n_fft = STFT_CASES[name][0]
    return 3, n_fft // 2 - 2
