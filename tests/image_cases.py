"""Inputs, shapes and checks of the Gabor image kernels (image.hip, filter2d_mm.hip) shared by the GPU parity tests
(tests/test_image_gpu.py) and their CPU-emulator twins (tests/test_emu_image.py).  Every reference is the float64 oracle
applied to the float32-rounded input; `run(img32, ker32)` is whatever executes filter2d in the calling file."""
import numpy as np

from oracle import d4w_oracle as orc

TOL = 1e-5
TOL_SPLIT = 3e-6          # split-binary16 products of exactly representable operands (tests/test_fuzz_gpu.py)


def rel(y, ref):
    return float(np.max(np.abs(np.asarray(y, dtype=np.float64) - ref)) / max(np.max(np.abs(ref)), 1e-300))


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def file_image(h, w, seed):
    """A 0-255 image like trace2image's: an offset of about 90 plus noise, clipped."""
    rng = np.random.default_rng(seed)
    return f32(np.clip(90.0 + 35.0 * rng.standard_normal((h, w)), 0.0, 255.0))


def noise_case(h, w, kh, kw):
    rng = np.random.default_rng(1000 * kh + kw + h + w)
    return f32(rng.standard_normal((h, w))), f32(rng.standard_normal((kh, kw)))


def filter2d_rel(run, img, ker):
    img, ker = f32(img), f32(ker)
    return rel(run(img, ker), orc.filter2d(img.astype(np.float64), ker.astype(np.float64)))


# ---- direct form (filter2d_tile): kernels of >= 114 columns.  (h, w, kh, kw)
DIRECT = [(10, 70, 3, 114),          # the smallest kernel without a matrix-core form, one tile
          (40, 150, 101, 115),       # 96 832-byte patch: above 64 KiB, the dynamic-LDS opt-in; 2 row tiles x 3 ragged column tiles
          (37, 130, 121, 121),       # Gabor ksize 120 on a 0-255 image; reflections wrap more than once
          (8, 40, 145, 145),         # 146 432 bytes of LDS, just under the 160 KiB limit
          (33, 65, 2, 120)]          # even kh, one row and one column past a tile edge
REFUSED = [(201, 201), (3, 1200)]    # need 244 992 and 202 080 bytes of LDS


def direct_case(h, w, kh, kw, gabor=orc.get_gabor_kernel):
    if (kh, kw) == (121, 121):
        return file_image(h, w, 121), f32(gabor((120, 120), 4, np.pi / 2 + np.deg2rad(42.56), 20, 0.15, 0))
    return noise_case(h, w, kh, kw)


# ---- matrix-core form (filter2d_mm_rows)
WIDE = [(6, 2305, 5, 101),           # two workgroups per row block, the second one 257 columns
        (5, 4200, 3, 33),            # three workgroups per row block
        (9, 2049, 2, 113)]           # one column past the first workgroup
TILE_EDGES = [(5, w, 4, 16) for w in (255, 256, 257, 511, 513)]
RING_EDGES = [(7, 300, kh, 7) for kh in (1, 2, 3, 4, 5, 8, 9)]       # kh around the prefetch ring (4) and the row ring (4 + 1)
SHORT_IMAGES = [(h, 300, 9, 7) for h in (1, 2, 3, 5)]                # vertical reflection wraps; ragged last row group


def check_values(run):
    """Value ranges the detector feeds filter2d, on a 9 x 300 image with a 7 x 9 kernel (4 x 16 for the binary image).
    Returns {case: measured figure} after asserting each."""
    rng = np.random.default_rng(79)
    ker = f32(rng.standard_normal((7, 9)))
    k64 = ker.astype(np.float64)
    got = {}
    # constant image: sum(K) everywhere, whatever the border does
    out = np.asarray(run(np.full((9, 300), 37.25, dtype=np.float32), ker), dtype=np.float64)
    got["constant"] = float(np.max(np.abs(out - 37.25 * k64.sum())) / (37.25 * np.abs(k64).sum()))
    assert got["constant"] <= 1e-5, got
    # the m == 0 branch of both power-of-two scales: exact zeros
    noise = f32(rng.standard_normal((9, 300)))
    z = np.asarray(run(np.zeros((9, 300), dtype=np.float32), ker))
    assert z.shape == (9, 300) and np.array_equal(z, np.zeros_like(z))
    z = np.asarray(run(noise, np.zeros((7, 9), dtype=np.float32)))
    assert z.shape == (9, 300) and np.array_equal(z, np.zeros_like(z))
    got["offset 1e4"] = filter2d_rel(run, 1e4 + noise, ker)
    got["0-255"] = filter2d_rel(run, file_image(9, 300, 5), ker)
    # independent scales of image and kernel
    got["1e-30 x 1e20"] = filter2d_rel(run, noise * np.float32(1e-30), ker * np.float32(1e20))
    assert max(got["offset 1e4"], got["0-255"], got["1e-30 x 1e20"]) < TOL, got
    binary = f32(rng.random((9, 300)) < 0.1)
    got["binary"] = filter2d_rel(run, binary, f32(rng.standard_normal((4, 16))))
    assert got["binary"] < TOL_SPLIT, got
    return got


# ---- one non-finite pixel
NONFINITE = [(5, 9), (3, 115)]       # (kh, kw): matrix cores, direct form


def check_nonfinite(run, kh, kw, bad):
    """20 x 400 noise with img[10, 200] = bad (NaN or inf).  The call returns; every output whose kh x kw window holds the
    pixel is non-finite; every output that is finite equals the oracle of the image with that pixel at 0; at most a quarter
    of the outputs are non-finite.  Where the non-finite region ends is not asserted.  Returns (non-finite count, rel)."""
    img, ker = noise_case(20, 400, kh, kw)
    clean = img.copy()
    clean[10, 200] = 0.0
    ref = orc.filter2d(clean.astype(np.float64), ker.astype(np.float64))
    img[10, 200] = bad
    out = np.asarray(run(img, ker), dtype=np.float64)
    assert out.shape == ref.shape
    nonfin = ~np.isfinite(out)
    # out[y, x] reads img[y + ky - kh // 2, x + kx - kw // 2]  (no reflection reaches [10, 200] in this image)
    ys = slice(10 + kh // 2 - (kh - 1), 10 + kh // 2 + 1)
    xs = slice(200 + kw // 2 - (kw - 1), 200 + kw // 2 + 1)
    assert nonfin[ys, xs].all(), "a window that holds the non-finite pixel gave a finite output"
    n = int(nonfin.sum())
    assert n <= out.size // 4, n
    err = float(np.max(np.abs(out[~nonfin] - ref[~nonfin])) / np.max(np.abs(ref)))
    assert err < TOL, err
    return n, err


# ---- resize_rows: a workgroup of 256 outputs stages its input span in LDS when that is <= 4096 samples
RS_SPAN = 4096
RESIZE = [(3, 6000, 3, 300),         # first workgroup unstaged, second staged
          (2, 9000, 2, 100),         # scale 90: 181 taps
          (3, 4500, 3, 257),         # two workgroups, the second holds one output
          (3, 4791, 3, 300),         # first workgroup's span is exactly 4096: staged
          (3, 4792, 3, 300),         # ... 4097: unstaged
          (5, 30, 50, 6000)]         # upsampling: the horizontal pass writes more than 4096 columns
RESIZE_SPANS = {(6000, 300): lambda s: s[0] > RS_SPAN >= s[1], (9000, 100): lambda s: s == [9000],
                (4500, 257): lambda s: s[0] > RS_SPAN and len(s) == 2, (4791, 300): lambda s: s[0] == RS_SPAN,
                (4792, 300): lambda s: s[0] == RS_SPAN + 1, (30, 6000): lambda s: len(s) == 24 and max(s) <= RS_SPAN}


def workgroup_spans(w, ow):
    """Input samples spanned by each workgroup of 256 outputs of the horizontal pass, from the oracle's weight table."""
    rows = orc._aa_weights(w, ow)
    spans = []
    for ox0 in range(0, ow, 256):
        oxl = min(ox0 + 256, ow) - 1
        spans.append(rows[oxl][0] + len(rows[oxl][1]) - rows[ox0][0])
    return spans


def check_resize_side(w, ow):
    spans = workgroup_spans(w, ow)
    assert RESIZE_SPANS[(w, ow)](spans), (w, ow, spans)
    return spans


def bin_factors(h, w, oh, ow):
    """(ft, fx) with int(h * fx) == oh and int(w * ft) == ow, as improcess.binning and the oracle compute the output size."""
    ft, fx = (ow + 0.5) / w, (oh + 0.5) / h
    assert int(h * fx) == oh and int(w * ft) == ow
    return ft, fx


# ---- d4w_minmax_f32: one workgroup up to 65 536 values, three launches above
MINMAX_N = [1, 5, 65536, 65537, 300000]


def minmax_cases(n):
    """(name, float32 array) pairs; the expected result is np.min / np.max of the array (NaN propagates)."""
    rng = np.random.default_rng(n)
    plain = f32(rng.standard_normal(n) * 7 - 2)
    cases = [("plain", plain)]
    for name, idx in (("nan first", 0), ("nan last", n - 1), ("nan middle", n // 3)):
        x = plain.copy()
        x[idx] = np.nan
        cases.append((name, x))
    x = plain.copy()
    x[n // 2] = np.inf
    x[n - 1 if n // 2 != n - 1 else 0] = -np.inf          # (n == 1 holds -inf alone)
    cases.append(("infs", x))
    cases.append(("negative", f32(-1.0 - np.abs(plain))))
    x = f32(1.0 + np.abs(plain))
    x[n // 2] = -0.0
    cases.append(("minus zero", x))
    return cases


def check_minmax(name, x, mm):
    lo, hi = np.min(x), np.max(x)
    if np.isnan(lo):
        assert np.isnan(mm[0]) and np.isnan(mm[1]), (name, x.size, mm)
    else:
        assert mm[0] == lo and mm[1] == hi, (name, x.size, mm, lo, hi)     # (-0.0 == 0.0: the value, not the sign)


def threshold_inputs(thr=0.1):
    """float32 values around a float64 threshold: the decision is float64(x) > thr."""
    up = np.float32(thr)
    if float(up) <= thr:
        up = np.nextafter(up, np.float32(np.inf))
    down = np.nextafter(up, np.float32(-np.inf))             # thr rounded down
    assert float(down) <= thr < float(up)
    x = f32([np.float32(thr), up, down, np.nextafter(down, np.float32(-np.inf)), np.nextafter(up, np.float32(np.inf)),
             -thr, 0.0, 1.0])
    return x, x.astype(np.float64) > thr


# ---- gabor_mask on a file-shaped block
def chirp_block(nx=1050, ns=2570, fs=200.0, dx=2.04, step=4, c0=1500.0, seed=31):
    """Band-limited noise plus four 15-25 Hz chirps along lines of slope near c0 (both directions) in the [channel x time]
    grid, float32.  Binned by 10 it is 105 x 257: 4 * 26 + 1 rows, one column past a 256-column tile, larger than the
    101 x 101 kernel in both axes."""
    rng = np.random.default_rng(seed)
    spec = np.fft.rfft(rng.standard_normal((nx, ns)), axis=1)
    f = np.fft.rfftfreq(ns, 1 / fs)
    spec *= ((f > 10) & (f < 40))[None, :]
    x = np.fft.irfft(spec, n=ns, axis=1)
    x /= x.std()
    t = np.arange(ns)[None, :] / fs
    ch = np.arange(nx)[:, None]
    for t0, ch0, sign, c, amp in ((2.0, 100, 1, 1500.0, 3.0), (9.0, 900, -1, 1480.0, 2.5), (4.0, 500, 1, 1530.0, 2.0),
                                  (11.0, 300, -1, 1500.0, 3.5)):
        tau = t - (t0 + sign * (ch - ch0) * step * dx / c)            # time since the arrival on every channel
        on = (tau >= 0) & (tau < 0.7)
        x += amp * on * np.sin(np.pi * tau / 0.7) ** 2 * np.cos(2 * np.pi * (25.0 * tau - 10.0 / (2 * 0.7) * tau ** 2))
    return f32(x), fs, dx, [0, nx * step, step], c0


def gabor_reference(x32, fs, dx, sel, c0):
    """orc.gabor_mask_pipeline on the float32-rounded block with both thresholds at the 90th percentile of the array
    they apply to; the oracle's binary image and mask must hold both classes.  Returns (result dict, thr, thr2)."""
    thr = {}

    def p90(key):
        def pick(a):
            thr[key] = float(np.percentile(a, 90))
            return thr[key]
        return pick
    ref = orc.gabor_mask_pipeline(x32.astype(np.float64), fs, dx, sel, c0, p90("threshold"), p90("threshold2"))
    for key in ("binary", "mask"):
        assert 0.02 <= ref[key].mean() <= 0.98, (key, ref[key].mean())
    return ref, thr["threshold"], thr["threshold2"]


def near(img, thr, tol):
    return np.abs(img - thr) <= tol * np.max(np.abs(img))


def check_gabor(r, ref, thr, thr2, x32, say=print):
    """The structure of test_golden_pipeline_one_call: floats at TOL, binary decisions identical except within TOL max|.|
    of the threshold, and the exact comparisons downstream whenever nothing flipped.  Returns the measured figures."""
    got = {k: rel(r[k], ref[k]) for k in ("image", "imagebin", "fimage")}
    assert max(got.values()) < TOL, got
    flips1 = (ref["fimage"] > thr) != (np.asarray(r["fimage"], dtype=np.float64) > thr)
    assert not np.any(flips1 & ~near(ref["fimage"], thr, TOL))
    got["flips binary"] = int(flips1.sum())
    if not flips1.any():
        got["score"] = rel(r["score"], ref["score"])
        assert got["score"] < TOL, got
        flips2 = r["mask"] != ref["mask"]
        assert not np.any(flips2 & ~near(ref["score"], thr2, TOL))
        got["flips mask"] = int(flips2.sum())
        if not flips2.any():
            assert np.array_equal(r["mask_sparse"], ref["mask_sparse"])
            assert np.array_equal(r["masked_tr"], x32.astype(np.float64) * ref["mask_sparse"])
    say("gabor_mask %s: %s" % (x32.shape, got))
    return got
