"""Every mode of the analytic-signal operator (d4w_analytic_f32 / d4w_analytic_long_f32: 0 |z|, 1 H[x], 2 SNR in dB,
3 instantaneous frequency, 4 |z| / std) on every row path, against float64.

The reference is scipy.signal.hilbert in float64 on the float32 samples the kernel saw (oracle hilbert); modes 2 and 4
use np.var in float64 of those samples.  Bars (tests/analytic_cases.py): modes 0, 1, 4 max|y - ref| <= 1e-5 max|ref|;
mode 2 the same on the linear power ratios; mode 3 (modulo fs) d w < 1e-5 fs / 2 on every sample of every row with
w = min(|z_i|, |z_i+1|) / max|z|, d < 5e-5 fs / 2 where w >= 0.2 on the tone rows (at least 90 % of each, asserted from the
reference) and row medians within 0.1 Hz."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import d4w_oracle as orc
from tests import analytic_cases as ac

pytestmark = pytest.mark.gpu
TOL = ac.TOL
FS = ac.FS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX = 5

# row length -> (fits one workgroup's LDS, path).  Each is the smallest shape that reaches its path; nx * ns stays under
# 2^24, so nothing is compiled on the way.  The single-workgroup limit is L + 64 + ceil(L / 64) <= 19200 complex values
# (L = ns / 2 for even rows, ns for odd ones, the Bluestein tile for lengths with a prime factor > 31): even rows up to
# 37 676 samples, so 38400 and 19683 lie beyond it as they stand.
ROW_PATHS = {
    480: (1, "LDS, packed, 256 threads"),
    4200: (1, "LDS, packed, 512 threads, read-ahead tails (L = 2100)"),
    4095: (1, "LDS, odd (3^2 5 7 13)"),
    2018: (1, "LDS, packed, Bluestein (2 x 1009)"),
    4001: (1, "LDS, odd, Bluestein (prime)"),
    38400: (0, "long, even, generic kernels (L = 19200)"),
    19683: (0, "long, odd (3^9): analytic_combine_z"),
    40022: (0, "long, even, global-memory Bluestein (2 x 20011)"),
    20011: (0, "long, odd, Bluestein (prime)"),
}


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import das4whales_amd as dw_
    return dw_


_cases = {}


def case(ns):
    """(x float32 [5, ns]: four tones + a noise row, z, var) -- computed once per length; no test writes to it."""
    if ns not in _cases:
        x = ac.tone_block(NX, ns, seed=ns)
        _cases[ns] = (x,) + ac.reference(x)
    return _cases[ns]


def on_path(dw, ns):
    from das4whales_amd._lib import lib
    fits, path = ROW_PATHS[ns]
    assert lib.d4w_analytic_row_fits_lds(ns) == fits, "%d-sample rows have left the path '%s'" % (ns, path)
    assert NX * ns < (1 << 24)
    return lib


def row_var(lib, xt):
    from das4whales_amd import _device as dev
    from das4whales_amd._lib import check
    var = torch.full((xt.shape[0],), float("nan"), dtype=torch.float32, device=xt.device)
    with torch.cuda.device(xt.device):
        check(lib.d4w_row_var_f32(dev.ptr(xt), xt.shape[0], xt.shape[1], dev.ptr(var), dev.stream_ptr(xt)))
    return var


# ---------------------------------------------------------------------------------------------
# 1. modes x row paths through the public functions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2, 4])
@pytest.mark.parametrize("ns", sorted(ROW_PATHS))
def test_mode_on_row_path(dw, ns, mode):
    """dsp.envelope (0), dsp.hilbert_imag (1), dsp.snr_tr_array(env=True) (2) and the call of improcess.trace2image
    (d4w_row_var_f32 + mode 4) on four tone rows and a noise row."""
    lib = on_path(dw, ns)
    x, z, var = case(ns)
    if mode == 0:
        y = dw.dsp.envelope(x)
    elif mode == 1:
        y = dw.dsp.hilbert_imag(x)
    elif mode == 2:
        y = dw.dsp.snr_tr_array(x, env=True)
    else:
        xt = torch.from_numpy(x).cuda()
        y = dw.dsp._analytic(xt, 4, var=row_var(lib, xt)).cpu().numpy()
    assert isinstance(y, np.ndarray) and y.shape == x.shape
    err = ac.check_mode(mode, y, z, var)
    print("ns %5d mode %d (%s): err %.3e, bar %.0e" % (ns, mode, ROW_PATHS[ns][1], err, TOL))


@pytest.mark.parametrize("ns", sorted(ROW_PATHS))
def test_instant_freq_on_row_path(dw, ns):
    """dsp.instant_freq on the whole 2-D block: [nx, ns - 1] outputs, every row its own carrier (12, 21, 30, 39 Hz), the
    last row noise."""
    on_path(dw, ns)
    x, z, _ = case(ns)
    y = dw.dsp.instant_freq(x, FS)
    assert isinstance(y, np.ndarray) and y.shape == (NX, ns - 1)
    dwm, dmax, dmed, share = ac.check_ifreq(y, z, FS, range(NX - 1))
    print("ns %5d mode 3 (%s): max d w %.3e Hz, bar %.1e; max d on w >= 0.2 %.3e Hz, bar %.1e; medians within %.2e Hz, bar 0.1; "
          "w >= 0.2 on %.1f %% of a tone row" % (ns, ROW_PATHS[ns][1], dwm, TOL * FS / 2, dmax, 5 * TOL * FS / 2, dmed, 100 * share))


@pytest.mark.parametrize("ns", [4200, 19683])
def test_routing_and_types(dw, ns):
    """A CUDA float32 tensor comes back as a CUDA float32 tensor, a NumPy float64 array as NumPy float64, with the same
    values (the float64 array holds the float32 samples exactly)."""
    on_path(dw, ns)
    x, z, var = case(ns)
    xt = torch.from_numpy(x).cuda()
    x64 = x.astype(np.float64)
    for mode, fn in ((0, dw.dsp.envelope), (1, dw.dsp.hilbert_imag), (2, lambda a: dw.dsp.snr_tr_array(a, env=True)),
                     (3, lambda a: dw.dsp.instant_freq(a, FS))):
        yt, y64 = fn(xt), fn(x64)
        assert torch.is_tensor(yt) and yt.is_cuda and yt.dtype == torch.float32 and yt.device == xt.device
        assert isinstance(y64, np.ndarray) and y64.dtype == np.float64
        assert tuple(yt.shape) == y64.shape == (NX, ns - 1 if mode == 3 else ns)
        for y in (yt.cpu().numpy(), y64):
            if mode == 3:
                ac.check_ifreq(y, z, FS, range(NX - 1))
            else:
                ac.check_mode(mode, y, z, var)
    assert torch.equal(xt.cpu(), torch.from_numpy(x))                  # the input is left alone


# ---------------------------------------------------------------------------------------------
# 2. the specialised long-row path at the built-in test shapes
# ---------------------------------------------------------------------------------------------
SPECIALISED = [(8, 480), (100, 600), (154, 48), (1102, 48), (18, 48)]
_long = {}


def long_case(nx, ns):
    """(noise + 0.2 for modes 0, 1, 2, 4; tone rows with carriers 10 .. 60 Hz by r % 6 for mode 3; their references)."""
    if (nx, ns) not in _long:
        xn = (np.random.default_rng(1000 * nx + ns).standard_normal((nx, ns)) + 0.2).astype(np.float32)
        xt = ac.spread_tones(nx, ns)
        _long[(nx, ns)] = (xn, xt, ac.reference(xn), ac.reference(xt))
    return _long[(nx, ns)]


def check_long(tag, nx, ns, ys):
    xn, xt, (zn, varn), (zt, _) = long_case(nx, ns)
    figs = []
    for mode in range(5):
        if mode == 3:
            # rows this short are mostly edge: the conditioned bar on every row, the plain one where w >= 0.2
            figs.append(ac.check_ifreq(ys[3], zt, FS, range(nx), need_share=None)[0])
        else:
            figs.append(ac.check_mode(mode, ys[mode], zn, varn))
    print("%s %d x %d: modes 0, 1, 2, 4 err %.3e %.3e %.3e %.3e (bar %.0e); mode 3 max d w %.3e Hz (bar %.1e)"
          % (tag, nx, ns, figs[0], figs[1], figs[2], figs[4], TOL, figs[3], TOL * FS / 2))


@pytest.mark.parametrize("nx,ns", SPECIALISED)
def test_specialised_long_row_path(dw, nx, ns):
    """d4w_analytic_long_f32 called the way dsp._analytic calls it, on shapes that carry built-in specialised kernels
    (dsp._analytic never routes them there: the rows fit LDS): the inverse pass straight into y (mode 1), the fused
    epilogue (modes 0, 2, 4) and the inverse pass + analytic_combine (mode 3)."""
    from das4whales_amd import _device as dev
    from das4whales_amd._lib import lib
    assert lib.d4w_fk_shape_is_specialised(nx, ns) == 1
    assert os.environ.get("D4W_LONG_FAST", "1") != "0" and os.environ.get("D4W_LONG_FUSE", "1") != "0"
    xn, xt, _, _ = long_case(nx, ns)
    check_long("specialised", nx, ns, ac.run_long_modes(torch, lib, dev, xn, xt))


CHILD = """
import os, sys
import numpy as np
import torch
from das4whales_amd import _device as dev
from das4whales_amd._lib import lib
from tests import analytic_cases as ac
src, dst = sys.argv[1], sys.argv[2]
assert os.environ[sys.argv[3]] == "0"
d = np.load(src)
out = {}
for key in d["shapes"]:
    nx, ns = (int(v) for v in key.split("x"))
    assert lib.d4w_fk_shape_is_specialised(nx, ns) == 1
    ys = ac.run_long_modes(torch, lib, dev, d["noise_" + key], d["tones_" + key])
    for mode in range(5):
        out["y%d_%s" % (mode, key)] = ys[mode]
torch.cuda.synchronize()
np.savez(dst, **out)
"""


@pytest.mark.parametrize("switch,shapes", [("D4W_LONG_FAST", [(8, 480)]), ("D4W_LONG_FAST", [(100, 600)]),
                                           ("D4W_LONG_FUSE", [(8, 480), (100, 600)])])
def test_specialised_shapes_with_a_switch_off(dw, tmp_path, switch, shapes):
    """The same five modes with D4W_LONG_FAST=0 (the generic long-row kernels on these shapes) and with D4W_LONG_FUSE=0
    (the specialised plan with analytic_combine serving modes 0, 2 and 4), to the same bars.  The library reads either
    switch once per process, so each setting runs in a fresh child process."""
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    keys = ["%dx%d" % s for s in shapes]
    data = {"shapes": np.asarray(keys)}
    for key, (nx, ns) in zip(keys, shapes):
        data["noise_" + key], data["tones_" + key] = long_case(nx, ns)[:2]
    np.savez(src, **data)
    env = dict(os.environ)
    env.pop("D4W_LONG_FAST", None)
    env.pop("D4W_LONG_FUSE", None)
    env[switch] = "0"
    env["PYTHONPATH"] = ROOT + os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else ROOT
    p = subprocess.run([sys.executable, "-c", CHILD, src, dst, switch], cwd=ROOT, env=env, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    got = np.load(dst)
    for key, (nx, ns) in zip(keys, shapes):
        check_long("%s=0" % switch, nx, ns, [got["y%d_%s" % (mode, key)] for mode in range(5)])


# ---------------------------------------------------------------------------------------------
# 3. the row variance (the normaliser of modes 2 and 4) on rows that are mostly offset
# ---------------------------------------------------------------------------------------------
ULP = 6e-8                  # what storing a float64 variance as float32 allows, relative
_offset = {}


def offset_case(ns, ratio):
    """x = noise s + offset with offset / s = ratio, rows of s = 1, 3e-3, 40 and of either sign of the offset; float32."""
    if (ns, ratio) not in _offset:
        rng = np.random.default_rng(ns + int(ratio))
        s = np.array([[1.0], [3e-3], [40.0], [1.0]])
        x = (rng.standard_normal((4, ns)) * s + ratio * s * np.array([[1.0], [1.0], [1.0], [-1.0]])).astype(np.float32)
        _offset[(ns, ratio)] = x
    return _offset[(ns, ratio)]


@pytest.mark.parametrize("ratio", [1e3, 1e5])
@pytest.mark.parametrize("ns", [4000, 4001, 4002, 38400])
def test_row_variance_of_offset_rows(dw, ns, ratio):
    """d4w_row_var_f32 (16-byte loads when ns % 4 == 0, scalar loads otherwise) against np.var in float64 of the float32
    samples.  Storing the float64 variance as float32 allows one ulp (6e-8 relative); the bar is 4 ulp, the margin for
    the merge arithmetic.  Largest |var - ref| / (ulp ref) observed on an MI355X: 0.83 (ns = 4002,
    offset / s = 1e3; 0.76 at ns = 38400) -- the float32 rounding of the result and nothing else: the kernel's "no cancellation"
    holds on these rows."""
    from das4whales_amd._lib import lib
    x = offset_case(ns, ratio)
    var = row_var(lib, torch.from_numpy(x).cuda()).cpu().numpy().astype(np.float64)
    ref = np.var(x.astype(np.float64), axis=1)
    ratio_ulp = np.abs(var - ref) / (ULP * ref)
    print("row_var ns %d offset / s %.0e: |var - ref| / (ulp ref) = %s, bar 4" % (ns, ratio, np.array2string(ratio_ulp, precision=3)))
    assert np.all(ratio_ulp <= 4.0), ratio_ulp


@pytest.mark.parametrize("ratio", [1e3, 1e5])
@pytest.mark.parametrize("ns,env", [(4000, False), (4001, False), (4002, False), (4000, True), (4001, True), (4002, True), (38400, True)])
def test_snr_of_offset_rows(dw, ns, env, ratio):
    """dsp.snr_tr_array on rows that are mostly offset, on the linear power ratios as test_snr_fx_ifreq_golden compares
    them, the oracle given the float32 samples."""
    x = offset_case(ns, ratio)
    y = dw.dsp.snr_tr_array(x, env=env)
    assert y.shape == x.shape
    ref = orc.snr_tr_array(x.astype(np.float64), env=env)
    lin, lref = 10.0 ** (y.astype(np.float64) / 10), 10.0 ** (ref / 10)
    err = float(np.max(np.abs(lin - lref)) / np.max(lref))
    print("snr env=%s ns %d offset / s %.0e: err %.3e, bar %.0e" % (env, ns, ratio, err, TOL))
    assert err < TOL
    top = ref > -40
    assert np.max(np.abs(y[top] - ref[top])) < 1e-3


@pytest.mark.parametrize("ratio", [1e3, 1e5])
@pytest.mark.parametrize("ns", [4000, 4001, 4002])
def test_trace2image_of_offset_rows(dw, ns, ratio):
    """improcess.trace2image on rows that are mostly offset at the bar of test_image_gpu.py, the oracle given the float32
    samples."""
    x = offset_case(ns, ratio)
    y = dw.improcess.trace2image(x)
    ref = orc.trace2image(x.astype(np.float64))
    err = float(np.max(np.abs(y - ref)) / np.max(np.abs(ref)))
    print("trace2image ns %d offset / s %.0e: err %.3e, bar %.0e" % (ns, ratio, err, TOL))
    assert err < TOL
