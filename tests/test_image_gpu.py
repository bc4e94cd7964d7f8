"""GPU parity of the Gabor image pipeline against the
fixture generated from the reference's improcess code and against the oracle on larger blocks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import d4w_oracle as orc
from tests import golden_npz
from tests import image_cases as ic

pytestmark = pytest.mark.gpu
TOL = 1e-5
G = golden_npz.load("image_240x1600.npz")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(y, ref):
    return float(np.max(np.abs(np.asarray(y, dtype=np.float64) - ref)) / max(np.max(np.abs(ref)), 1e-300))


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available()
    import das4whales_amd as dw_
    return dw_


def test_golden_stages(dw):
    ip = dw.improcess
    trf = G["trf_fk"].astype(np.float64)
    image = ip.trace2image(trf)
    assert image.dtype == np.float64 and rel(image, G["image"]) < TOL
    assert rel(ip.scale_pixels(trf[:4]), G["scale_pixels"]) < TOL
    assert abs(ip.angle_fromspeed(1500., float(G["fs"]), float(G["dx"]), G["sel"]) - float(G["theta_c0"])) < 1e-12
    up, down = ip.gabor_filt_design(float(G["theta_c0"]))
    assert rel(up, G["gab_up"]) < 1e-12 and rel(down, G["gab_down"]) < 1e-12
    imagebin = ip.binning(G["image"].astype(np.float64), 1 / 10, 1 / 10)
    assert imagebin.shape == (24, 160) and rel(imagebin, G["imagebin"]) < TOL
    fimage = ip.filter2d(G["imagebin"], up) + ip.filter2d(G["imagebin"], down)
    assert rel(fimage, G["fimage"]) < TOL
    binary = G["fimage"] > float(G["threshold"])
    score = ip.filter2d(binary, up) + ip.filter2d(binary, down)
    assert rel(score, G["score"]) < TOL
    up_mask = ip.binning(G["mask"], 10, 10)
    assert up_mask.dtype == bool and np.array_equal(up_mask, G["mask_sparse"])
    assert np.array_equal(ip.apply_smooth_mask(trf, G["mask_sparse"]), trf.astype(np.float32).astype(np.float64) * G["mask_sparse"])
    assert rel(ip.apply_smooth_mask(G["imagebin"], G["mask"]), G["smoothed_image"]) < TOL


def _near(img, thr, tol):
    return np.abs(img - thr) <= tol * np.max(np.abs(img))


def test_golden_pipeline_one_call(dw):
    trf = G["trf_fk"].astype(np.float64)
    r = dw.improcess.gabor_mask(trf, float(G["fs"]), float(G["dx"]), G["sel"], float(G["c0"]), float(G["threshold"]),
                                float(G["threshold2"]))
    assert rel(r["image"], G["image"]) < TOL and rel(r["imagebin"], G["imagebin"]) < TOL
    assert rel(r["fimage"], G["fimage"]) < TOL
    # binary decisions: identical except pixels whose score is within the float32 budget of the threshold
    flips1 = (G["fimage"] > float(G["threshold"])) != (r["fimage"] > float(G["threshold"]))
    assert not np.any(flips1 & ~_near(G["fimage"], float(G["threshold"]), TOL))
    if not flips1.any():
        assert rel(r["score"], G["score"]) < TOL
        flips2 = r["mask"] != G["mask"]
        assert not np.any(flips2 & ~_near(G["score"], float(G["threshold2"]), TOL))
        if not flips2.any():
            assert np.array_equal(r["mask_sparse"], G["mask_sparse"])
            assert np.array_equal(r["masked_tr"], trf.astype(np.float32).astype(np.float64) * G["mask_sparse"])
    # CUDA tensors in -> CUDA tensors out
    rt = dw.improcess.gabor_mask(torch.from_numpy(G["trf_fk"]).cuda(), float(G["fs"]), float(G["dx"]), G["sel"],
                                 float(G["c0"]), float(G["threshold"]), float(G["threshold2"]))
    assert rt["masked_tr"].is_cuda and rt["mask"].dtype == torch.bool
    assert np.array_equal(rt["mask"].cpu().numpy(), r["mask"])


@pytest.mark.parametrize("h,w,kh,kw", [(400, 1200, 101, 101), (77, 333, 9, 31), (30, 20, 101, 101), (5, 5, 3, 3)])
def test_filter2d_random(dw, h, w, kh, kw):
    rng = np.random.default_rng(h + kw)
    img, ker = rng.standard_normal((h, w)), rng.standard_normal((kh, kw))
    assert rel(dw.improcess.filter2d(img, ker), orc.filter2d(img, ker)) < TOL


@pytest.mark.parametrize("h,w,ft,fx", [(4000, 1200, 0.1, 0.1), (1102, 1200, 0.1, 0.1), (123, 457, 0.37, 0.21), (40, 120, 10, 10),
                                       (31, 77, 2.5, 3.0)])
def test_binning_random(dw, h, w, ft, fx):
    rng = np.random.default_rng(h)
    img = rng.standard_normal((h, w))
    ref = orc.binning(img, ft, fx)
    got = dw.improcess.binning(img, ft, fx)
    assert got.shape == ref.shape and rel(got, ref) < TOL
    m = rng.random((h, w)) > 0.97
    assert np.array_equal(dw.improcess.binning(m, ft, fx), orc.binning(m, ft, fx))


def test_trace2image_block_and_long_rows(dw):
    rng = np.random.default_rng(9)
    x = rng.standard_normal((300, 12000)) * rng.uniform(0.5, 2, (300, 1))
    assert rel(dw.improcess.trace2image(x), orc.trace2image(x)) < TOL
    xl = rng.standard_normal((6, 120000))                                  # long-row analytic path
    assert rel(dw.improcess.trace2image(xl), orc.trace2image(xl)) < TOL


def test_errors(dw):
    with pytest.raises(ValueError):
        dw.improcess.trace2image(np.zeros(10))
    with pytest.raises(ValueError):
        dw.improcess.apply_smooth_mask(np.zeros((4, 4)), np.zeros((4, 5), dtype=bool))
    with pytest.raises(ValueError):                                        # int(1101.99..) * 10 != 11020-like mismatch
        dw.improcess.gabor_mask(np.random.default_rng(0).standard_normal((25, 95)), 200., 2.04, [0, 100, 4])


def test_cv2_stand_ins_against_the_documented_definitions(dw):
    """The product's filter2d (HIP) and get_gabor_kernel against OpenCV's documented definitions written as loops
    (tests/known_answers.py) -- not against the restatement."""
    from tests import known_answers as ka
    ka.check_filter2d(dw.improcess.filter2d, 2e-6)
    ka.check_gabor_kernel(dw.improcess.get_gabor_kernel, 1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# Kernels and branches the cases above never reach (shapes, inputs and checks: tests/image_cases.py, shared with the
# emulator twins in tests/test_emu_image.py).  References: the float64 oracle on the float32-rounded input.
# ---------------------------------------------------------------------------------------------------------------------
def _lib():
    from das4whales_amd._lib import lib
    return lib


@pytest.mark.parametrize("h,w,kh,kw", ic.DIRECT)
def test_filter2d_direct_form(dw, h, w, kh, kw):
    """filter2d_tile (kernels of >= 114 columns): one tile, the dynamic-LDS opt-in above 64 KiB, 146 432 bytes of LDS,
    ragged tiles, an even kernel height, a Gabor kernel of ksize 120 on a 0-255 image."""
    assert _lib().d4w_filter2d_mm_eligible(kh, kw) == 0
    e = ic.filter2d_rel(dw.improcess.filter2d, *ic.direct_case(h, w, kh, kw, dw.improcess.get_gabor_kernel))
    print("direct %s rel %.2e" % ((h, w, kh, kw), e))
    assert e < TOL


def test_filter2d_direct_form_accumulates(dw):
    """filter2d_tile<true>: the second kernel of a list adds to the first one's output."""
    assert _lib().d4w_filter2d_mm_eligible(3, 114) == 0
    img, k1 = ic.noise_case(10, 70, 3, 114)
    k2 = ic.noise_case(11, 70, 3, 114)[1]
    got = dw.improcess._filter2d_device(torch.from_numpy(img).cuda(), [k1, k2]).cpu().numpy()
    i64 = img.astype(np.float64)
    e = rel(got, orc.filter2d(i64, k1.astype(np.float64)) + orc.filter2d(i64, k2.astype(np.float64)))
    print("direct, two kernels accumulated: rel %.2e" % e)
    assert e < TOL


def test_filter2d_refuses_kernels_beyond_the_lds_before_any_launch(dw):
    """Kernels whose patch exceeds 160 KiB of LDS raise the library's error naming the need, nothing having run (the
    output and the workspace keep their fill), and leave no sticky error: the next call is right."""
    lib = _lib()
    img = torch.from_numpy(ic.noise_case(8, 40, 3, 3)[0]).cuda()
    for kh, kw in ic.REFUSED:
        with pytest.raises(ValueError, match="bytes of LDS"):
            dw.improcess.filter2d(img.cpu().numpy(), np.ones((kh, kw)))
        ker = torch.ones((kh, kw), dtype=torch.float32, device="cuda")
        out = torch.full_like(img, 7.0)
        ws = torch.full((int(lib.d4w_filter2d_ws_bytes(kh, kw)),), 0x5a, dtype=torch.uint8, device="cuda")
        rc = lib.d4w_filter2d_f32(img.data_ptr(), 8, 40, ker.data_ptr(), kh, kw, out.data_ptr(), 0, ws.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
        assert rc == -1 and b"bytes of LDS" in lib.d4w_last_error()
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((ws == 0x5a).all())
    assert ic.filter2d_rel(dw.improcess.filter2d, *ic.noise_case(8, 40, 3, 114)) < TOL
    torch.cuda.synchronize()


@pytest.mark.parametrize("h,w,kh,kw", ic.WIDE + ic.TILE_EDGES + ic.RING_EDGES + ic.SHORT_IMAGES)
def test_filter2d_matrix_core_edges(dw, h, w, kh, kw):
    """filter2d_mm_rows: two and three workgroups per row block (blockIdx.x > 0 with the prefetch ring in its steady
    state), images that end before, on and after a 256-column tile, kernel heights around the prefetch ring (4) and the
    row ring (4 + 1), images shorter than the kernel and than a row group."""
    assert _lib().d4w_filter2d_mm_eligible(kh, kw) == 1
    e = ic.filter2d_rel(dw.improcess.filter2d, *ic.noise_case(h, w, kh, kw))
    print("matrix cores %s rel %.2e" % ((h, w, kh, kw), e))
    assert e < TOL


def test_filter2d_value_ranges(dw):
    """What the detector feeds the matrix-core form: a constant, zeros (exact), a large offset, a 0-255 image, a 0 / 1
    image (3e-6), and image and kernel scaled apart by 1e-30 and 1e20."""
    assert _lib().d4w_filter2d_mm_eligible(7, 9) == 1 and _lib().d4w_filter2d_mm_eligible(4, 16) == 1
    print("value ranges:", ic.check_values(dw.improcess.filter2d))


@pytest.mark.parametrize("kh,kw", ic.NONFINITE)
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_filter2d_one_nonfinite_pixel(dw, kh, kw, bad):
    """One NaN or inf pixel makes more outputs non-finite than its kh x kw window, in both forms: pinned
    here are that the call returns, that the window is non-finite, that every finite output is right and that at most a
    quarter of the outputs are lost."""
    n, e = ic.check_nonfinite(dw.improcess.filter2d, kh, kw, bad)
    torch.cuda.synchronize()
    print("%s pixel, kernel %d x %d: %d of 8000 outputs non-finite, finite ones rel %.2e" % (bad, kh, kw, n, e))


@pytest.fixture(scope="module")
def chirps():
    """The file-shaped block and its oracle result, computed once (four 105 x 257 x 101^2 correlations)."""
    x32, fs, dx, sel, c0 = ic.chirp_block()
    ref, thr, thr2 = ic.gabor_reference(x32, fs, dx, sel, c0)
    return {"x32": x32, "fs": fs, "dx": dx, "sel": sel, "c0": c0, "ref": ref, "thr": thr, "thr2": thr2}


def test_gabor_mask_file_shape(dw, chirps):
    """gabor_mask as scripts/main_gabordetect.py shapes it: 1050 x 2570 -> 105 x 257 binned (larger than the 101 x 101
    kernel, two 256-column tiles, 4 * 26 + 1 rows), thresholds at the oracle's 90th percentiles."""
    c = chirps
    x64 = c["x32"].astype(np.float64)
    r = dw.improcess.gabor_mask(x64, c["fs"], c["dx"], c["sel"], c["c0"], c["thr"], c["thr2"])
    assert r["imagebin"].shape == (105, 257)
    ic.check_gabor(r, c["ref"], c["thr"], c["thr2"], c["x32"])
    rt = dw.improcess.gabor_mask(torch.from_numpy(c["x32"]).cuda(), c["fs"], c["dx"], c["sel"], c["c0"], c["thr"], c["thr2"])
    assert rt["masked_tr"].is_cuda and rt["mask"].dtype == torch.bool
    assert np.array_equal(rt["mask"].cpu().numpy(), r["mask"])


CHILD = """
import json, sys
import numpy as np
import das4whales_amd as dw
from das4whales_amd._lib import lib
from oracle import d4w_oracle as orc
from tests import image_cases as ic
assert lib.d4w_filter2d_mm_eligible(101, 101) == 0
ref = dict(np.load(sys.argv[1]))
img = ic.file_image(60, 300, 60)
up = ic.f32(dw.improcess.gabor_filt_design(42.56)[0])
out = {"filter2d": ic.filter2d_rel(dw.improcess.filter2d, img, up)}
x32, fs, dx, sel, c0 = ic.chirp_block()
thr, thr2 = float(ref["thr"]), float(ref["thr2"])
r = dw.improcess.gabor_mask(x32.astype(np.float64), fs, dx, sel, c0, thr, thr2)
out.update(ic.check_gabor(r, ref, thr, thr2, x32, say=lambda s: None))
print("RESULT " + json.dumps(out))
"""


def test_direct_form_forced_for_the_detector_kernels(dw, chirps, tmp_path):
    """D4W_F2D_MM=0 sends the 101 x 101 Gabor kernels through filter2d_tile: filter2d on a 60 x 300 0-255 image and the
    gabor_mask above, to the same bars.  The library reads the switch once per process, so it runs in a fresh child."""
    src = str(tmp_path / "ref.npz")
    np.savez(src, thr=chirps["thr"], thr2=chirps["thr2"], **chirps["ref"])
    env = dict(os.environ)
    env["D4W_F2D_MM"] = "0"
    env["PYTHONPATH"] = ROOT + os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else ROOT
    p = subprocess.run([sys.executable, "-c", CHILD, src], cwd=ROOT, env=env, timeout=120, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print("D4W_F2D_MM=0:", got)
    assert got["filter2d"] < TOL and max(got[k] for k in ("image", "imagebin", "fimage")) < TOL


@pytest.mark.parametrize("h,w,oh,ow", ic.RESIZE)
def test_binning_unstaged_branch_and_neighbours(dw, h, w, oh, ow):
    """resize_rows reads global memory directly when a workgroup's 256 outputs span more than 4096 inputs (binning a
    12 000-sample file by 1 / 20 does); the span of every case comes from the oracle's weight table."""
    spans = ic.check_resize_side(w, ow)
    ft, fx = ic.bin_factors(h, w, oh, ow)
    rng = np.random.default_rng(w + ow)
    x = ic.f32(rng.standard_normal((h, w))).astype(np.float64)
    ref = orc.binning(x, ft, fx)
    got = dw.improcess.binning(x, ft, fx)
    assert got.shape == ref.shape == (oh, ow)
    e = rel(got, ref)
    print("binning %s spans %s rel %.2e" % ((h, w, oh, ow), spans[:3], e))
    assert e < TOL
    m = rng.random((h, w)) > 0.97
    assert np.array_equal(dw.improcess.binning(m, ft, fx), orc.binning(m, ft, fx))


@pytest.mark.parametrize("n", ic.MINMAX_N)
def test_minmax_forms_and_nonfinite_values(dw, n):
    """d4w_minmax_f32 on hardware (its wave vote and its two integer atomics): one workgroup up to 65 536 values, three
    launches above; NaN anywhere (first, last, middle) makes both results NaN, infinities come back, -0.0 counts as 0."""
    for name, x in ic.minmax_cases(n):
        mm = dw.improcess._minmax(torch.from_numpy(x).cuda()).cpu().numpy()
        ic.check_minmax(name, x, mm)


def test_scale_constant_image_and_threshold_in_float64(dw):
    """scale_pixels of a constant image is 0 / 0 = NaN in the reference: NaN here too, never a finite number.
    d4w_threshold_f32 decides float64(x) > thr, so float32 neighbours of 0.1 fall on the side float64 puts them."""
    x = np.full((7, 100), 3.5)
    with np.errstate(invalid="ignore"):
        ref = orc.scale_pixels(x)
    got = dw.improcess.scale_pixels(x)
    assert np.isnan(ref).all() and np.array_equal(np.isnan(got), np.isnan(ref))
    xs, want = ic.threshold_inputs(0.1)
    xt = torch.from_numpy(xs).cuda()
    y = torch.empty_like(xt)
    assert _lib().d4w_threshold_f32(xt.data_ptr(), y.data_ptr(), xs.size, 0.1, torch.cuda.current_stream().cuda_stream) == 0
    assert np.array_equal(y.cpu().numpy() != 0, want)
