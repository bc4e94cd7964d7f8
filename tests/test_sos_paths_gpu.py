"""Every run-time fork of the zero-phase second-order-section filter (dsp.bp_filt / dsp.sosfiltfilt) on hardware: the table
of tests/sos_cases.py (1 - 10 sections, float and double states, all input kinds) x the paths

  a  sos_pass_lanes<G = 8 | 16, float | double>, one exact segment per row (the DPP hand-over as the hardware does it),
  b  sos_pass<N = 1 .. 10, float | double>, warm-started segments,
  c  the overlap-save interior + row-end pieces, at the row length where that form starts, on one stream, as two phases,
  d  a file with one or two neighbouring files (d4w_fir_fft_halo_f32, d4w_sosfiltfilt_ends_sides_f32),
  e  the switches the library reads once per process (D4W_SOS_LANES, D4W_SOS_F64), each in a child process,
  f  the public band-pass on two tones of known gain,

each proven taken (d4w_sosfiltfilt_last_form: the kernel and the state precision the library dispatched; a form that returns
None when it does not apply), each result against scipy.signal.sosfiltfilt in float64 on the same float32 rows at 1e-5 of the block's max|ref|.  Rows of a
low-pass whose offset is 1e3 / 1e5 x their signal are judged one by one against two bars: 1e-5 of the row's max|ref|, and --
the one that matters -- 1e-5 of max|ref - row mean| plus 1 ulp of float32 at max|ref| (sos_cases.heavy_bar: what storing
offset + signal in a float32 costs).  Every case's float32-workspace figure is asserted below 1e-6 first."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.signal as sps
import torch

from tests import sos_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES_NX = (1, 5, 33, 67)
LANES_NS = (64, 65, 255, 257, 1205)


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import das4whales_amd as dw_
    return dw_


def gpu(x):
    return torch.from_numpy(np.array(x, dtype=np.float32, order="C")).cuda()      # a copy: the table's rows are read-only


def worst(figs, new):
    for k, v in new.items():
        figs[k] = max(figs.get(k, 0.0), v)
    return figs


def lanes_shapes(padlen):
    return [(nx, ns) for ns in sorted({padlen + 1} | {n for n in LANES_NS if n > padlen}) for nx in LANES_NX]


def last_form():
    from das4whales_amd._lib import lib
    return int(lib.d4w_sosfiltfilt_last_form())


def run_lanes(dsp, name, shapes, lanes=True, forced=None, save=None):
    """One exact segment per row on the given shapes, the kernel and state precision the library reports asserted; the worst
    figures.  `save`: a file that receives the (last) judged output."""
    sos = sc.design(name)
    figs = {}
    for nx, ns in shapes:
        x, ref, kinds, padlen = sc.case(name, nx, ns)
        y = dsp._sosfiltfilt_recursive(gpu(x), sos, padlen, seg_len=0, warm=0).cpu().numpy()
        assert last_form() == sc.expected_form(name, lanes, forced), (name, last_form())
        worst(figs, sc.judge(y, ref, kinds, "%s %dx%d" % (name, nx, ns)))
        if save:
            np.save(save, y)
        worst(figs, {"cond": sc.conditioning(name, ns, padlen)})
    return figs


@pytest.mark.parametrize("name", sc.NAMES)
def test_lanes_kernel_one_exact_segment(dw, name):
    """a: every design x nx in {1, 5, 33, 67} (ragged lanes, waves and workgroups at 8 and 4 rows per wave) x ns in
    {padlen + 1, 64, 65, 255, 257, 1205} above padlen (the 64-sample chunk, the four-chunk ring)."""
    figs = run_lanes(dw.dsp, name, lanes_shapes(sc.default_padlen(sc.design(name))))
    print("a lanes %-6s %-6s G=%d %s" % (name, sc.states(name), 8 if sc.DESIGNS[name][3] <= 8 else 16, json.dumps(figs)))


@pytest.mark.parametrize("name", sc.ONE_PER_NSEC)
def test_lane_per_row_kernel_segmented(dw, name):
    """b: one design per section count 1 .. 10 plus the double-state designs, 67 rows (a full wave and a ragged one), warm as
    dsp._sosfiltfilt_recursive derives it, at least three segments, a row length that is no multiple of 32."""
    sos = sc.design(name)
    seg_len, warm, ns = sc.segmentation(sos, dw.dsp._sos_decay_samples(sos))
    assert warm == -(-int(1.5 * dw.dsp._sos_decay_samples(sos)) // 32) * 32
    assert -(-ns // seg_len) >= 3 and seg_len + 2 * warm < ns and ns % 32
    x, ref, kinds, padlen = sc.case(name, 67, ns)
    y = dw.dsp._sosfiltfilt_device(gpu(x), sos, padlen, seg_len, warm)
    assert last_form() == sc.expected_form(name, lanes=False), (name, last_form())
    figs = sc.judge(y.cpu().numpy(), ref, kinds, name)
    figs["cond"] = sc.conditioning(name, ns, padlen)
    print("b segmented %-6s %-6s N=%d ns=%d seg=%d warm=%d %s" % (name, sc.states(name), sos.shape[0], ns, seg_len, warm, json.dumps(figs)))


def fft_geometry(dsp, name):
    sos = sc.design(name)
    zp = dsp._zero_phase_taps(sos, torch.device("cuda", torch.cuda.current_device()))
    assert zp is not None, name
    _, K, E, _ = zp
    assert E >= K
    return sos, sc.default_padlen(sos), int(K), int(E), 2 * int(E)


@pytest.mark.parametrize("name", sc.FFT_DESIGNS)
def test_overlap_save_form_at_its_first_row_lengths(dw, name, monkeypatch):
    """c: the public dsp.sosfiltfilt at ns = 4 P - 1 (the recursion answers: _sosfiltfilt_fft returns None), 4 P and 4 P + 3
    (the overlap-save interior + row-end pieces answer), nx in {1, 9}; at 4 P + 3 also on one stream (D4W_BP_OVERLAP=0)."""
    sos, padlen, K, E, P = fft_geometry(dw.dsp, name)
    figs = {}
    for ns in (4 * P - 1, 4 * P, 4 * P + 3):
        for nx in (1, 9):
            x, ref, kinds, pl = sc.case(name, nx, ns)
            assert pl == padlen
            xd = gpu(x)
            direct = dw.dsp._sosfiltfilt_fft(xd, sos, padlen)
            assert (direct is None) == (ns < 4 * P), (name, ns)
            y = dw.dsp.sosfiltfilt(sos, xd, axis=1)
            # the row-end pieces (overlap-save form) always run the lanes kernel; the recursion at 4 P - 1 picks its own
            # segmentation: only the state precision is pinned there
            assert last_form() // 100 == sc.expected_form(name) // 100 and (ns < 4 * P or last_form() == sc.expected_form(name))
            if direct is not None:
                assert torch.equal(y, direct)
            what = "%s %dx%d" % (name, nx, ns)
            worst(figs, sc.judge(y.cpu().numpy(), ref, kinds, what))
            worst(figs, {"cond": sc.conditioning(name, ns, padlen)})
            if ns == 4 * P + 3:
                monkeypatch.setenv("D4W_BP_OVERLAP", "0")
                y1 = dw.dsp.sosfiltfilt(sos, xd, axis=1)
                monkeypatch.delenv("D4W_BP_OVERLAP")
                assert torch.equal(y1, y), what                   # same kernels on one stream: the same bits
                sc.judge(y1.cpu().numpy(), ref, kinds, what + " one stream")
    print("c overlap-save %-6s %-6s K=%d E=%d %s" % (name, sc.states(name), K, E, json.dumps(figs)))


@pytest.mark.parametrize("name", sc.FFT_DESIGNS)
def test_row_end_pieces_as_two_phases(dw, name):
    """c: d4w_sosfiltfilt_ends_f32 through the C ABI at ns = 4 P + 3, nx = 9, piece = P, keep = E: phase 1 then phase 2 equal
    phase 0 bit for bit, the kept columns hold the bar against float64 on the gathered pieces, every other column of a
    pre-filled y is untouched; each side alone (d4w_sosfiltfilt_ends_sides_f32) writes its columns of the same result."""
    from das4whales_amd._lib import lib
    sos, padlen, K, E, P = fft_geometry(dw.dsp, name)
    nx, ns = 9, 4 * P + 3
    x = sc.rows(name, nx, ns)
    xd = gpu(x)
    zi = np.ascontiguousarray(sps.sosfilt_zi(sos), dtype=np.float64)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ws = torch.empty(int(lib.d4w_sosfiltfilt_ends_ws_bytes(nx, P, padlen)), dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(phases, sides):
        y = torch.full_like(xd, 7.5)
        for ph in phases:
            if sides == 3:
                rc = lib.d4w_sosfiltfilt_ends_f32(xd.data_ptr(), y.data_ptr(), nx, ns, dp(sos), dp(zi), sos.shape[0], padlen, P, E, ph,
                                                  ws.data_ptr(), st)
            else:
                rc = lib.d4w_sosfiltfilt_ends_sides_f32(xd.data_ptr(), y.data_ptr(), nx, ns, dp(sos), dp(zi), sos.shape[0], padlen, P, E,
                                                        ph, sides, ws.data_ptr(), st)
            assert rc == 0, lib.d4w_last_error()
        return y.cpu().numpy()
    figs = sc.check_row_ends(run, name, x, sc.row_kinds(name, nx), padlen, P, E)
    assert last_form() == sc.expected_form(name)
    print("c row ends %-6s %-6s %s" % (name, sc.states(name), json.dumps(figs)))


@pytest.mark.parametrize("name", sc.FFT_DESIGNS)
def test_file_with_one_or_two_neighbours(dw, name):
    """d: a record of three files of n = 4 P + 3 samples, 9 rows.  First and last file through _sosfiltfilt_one_neighbour,
    the middle one through _sosfiltfilt_between, with halos of exactly K columns of their own and with halos that are views
    of the neighbouring file (row pitch n, not K) -- against float64 sosfiltfilt of the whole record on that file's columns.
    ALL n columns of every file are compared: the record's true ends are n > E samples away from the middle file, beyond the
    reach E of filtfilt's edge rule."""
    sos, padlen, K, E, P = fft_geometry(dw.dsp, name)
    nx, n = 9, 4 * P + 3
    assert n > E
    x, ref, kinds, pl = sc.case(name, nx, 3 * n)
    xd = gpu(x)
    files = [xd[:, k * n:(k + 1) * n].contiguous() for k in range(3)]
    figs = {"cond": sc.conditioning(name, 3 * n, pl)}
    for how in ("own", "view"):
        tail = lambda f: f[:, n - K:].clone() if how == "own" else f[:, n - K:]
        head = lambda f: f[:, :K].clone() if how == "own" else f[:, :K]
        assert (head(files[1]).stride(0) == K) == (how == "own")
        ys = [dw.dsp._sosfiltfilt_one_neighbour(files[0], None, head(files[1]), sos, padlen),
              dw.dsp._sosfiltfilt_between(files[1], tail(files[0]), head(files[2]), sos),
              dw.dsp._sosfiltfilt_one_neighbour(files[2], tail(files[1]), None, sos, padlen)]
        assert last_form() == sc.expected_form(name)               # the free side's pieces of the first and the last file
        for k, y in enumerate(ys):
            assert y is not None, (name, how, k)
            worst(figs, sc.judge(y.cpu().numpy(), ref[:, k * n:(k + 1) * n], kinds, "%s file %d halos %s" % (name, k, how)))
    print("d neighbours %-6s %-6s n=%d K=%d %s" % (name, sc.states(name), n, K, json.dumps(figs)))


CHILD = """
import json, sys
import das4whales_amd as dw
from tests.test_sos_paths_gpu import run_lanes
lanes, forced = sys.argv[2] == "lanes", sys.argv[3] if sys.argv[3] != "-" else None
out = {}
for name in sys.argv[4:]:
    out[name] = run_lanes(dw.dsp, name, [(33, 1205)], lanes=lanes, forced=forced, save=sys.argv[1] + "/" + name + ".npy")
    out[name]["y"] = sys.argv[1] + "/" + name + ".npy"
print("RESULT " + json.dumps(out))
"""


def child(env_add, names, tmp_path, lanes=True, forced=None):
    """run_lanes at 33 x 1205 for `names` in a fresh interpreter with the switch set (the library reads it once per process):
    the child asserts the bars (sos_cases.judge) and the kernel / state precision the switch must lead to; its figures and
    the very outputs it judged come back."""
    env = dict(os.environ, **env_add)
    env["PYTHONPATH"] = ROOT + os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else ROOT
    p = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path), "lanes" if lanes else "rows", forced or "-"] + list(names), cwd=ROOT, env=env, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert sorted(got) == sorted(names)
    return got


def default_run(dsp, name):
    x, _, _, padlen = sc.case(name, 33, 1205)
    y = dsp._sosfiltfilt_recursive(gpu(x), sc.design(name), padlen, seg_len=0, warm=0).cpu().numpy()
    assert last_form() == sc.expected_form(name)
    return y


def test_switch_lane_per_row_kernel_for_whole_rows(dw, tmp_path):
    """e: D4W_SOS_LANES=0 sends one exact segment per row through sos_pass<N>: one design per section count (and every
    double-state design) at 33 x 1205, to the same bars; the library reports one row per lane for every call."""
    got = child({"D4W_SOS_LANES": "0"}, sc.ONE_PER_NSEC, tmp_path, lanes=False)
    for name, f in got.items():
        print("e D4W_SOS_LANES=0 %-6s %-6s %s" % (name, sc.states(name), json.dumps({k: v for k, v in f.items() if k != "y"})))


def test_switch_double_states_forced(dw, tmp_path):
    """e: D4W_SOS_F64=1 runs float-state designs (bp8: 8 lanes per row, bp10: 16) with double states: inside the bar, and
    not the bits of the default float run -- the switch was read, and the library reports double states."""
    got = child({"D4W_SOS_F64": "1"}, ["bp8", "bp10"], tmp_path, forced="double")
    for name, f in got.items():
        assert sc.states(name) == "float"
        assert not np.array_equal(np.load(f["y"]), default_run(dw.dsp, name)), name
        print("e D4W_SOS_F64=1 %-6s %s" % (name, json.dumps({k: v for k, v in f.items() if k != "y"})))


def test_switch_float_states_forced(dw, tmp_path):
    """e: D4W_SOS_F64=0 keeps bp8 and bp10 on float states: inside the bar, and the bits of the default run."""
    got = child({"D4W_SOS_F64": "0"}, ["bp8", "bp10"], tmp_path, forced="float")
    for name, f in got.items():
        assert np.array_equal(np.load(f["y"]), default_run(dw.dsp, name)), name
        print("e D4W_SOS_F64=0 %-6s %s" % (name, json.dumps({k: v for k, v in f.items() if k != "y"})))


def test_bp_filt_two_tones_of_known_gain(dw):
    """f: the public dsp.bp_filt (14 - 30 Hz, order 8) on a row of two tones of amplitude 1: away from the row ends the
    20 Hz tone comes back with the amplitude |H(20 Hz)|^2 of the design to 1e-5, the 5 Hz tone below 1e-5."""
    ns = 6001
    t = np.arange(ns) / sc.FS
    x = (np.sin(2 * np.pi * 20.0 * t + 0.4) + np.sin(2 * np.pi * 5.0 * t + 1.1)).astype(np.float32)
    y = dw.dsp.bp_filt(x.astype(np.float64), sc.FS, 14, 30)
    assert y.shape == (ns,) and y.dtype == np.float64
    mid = slice(1500, 4500)
    basis = np.stack([np.sin(2 * np.pi * 20.0 * t), np.cos(2 * np.pi * 20.0 * t), np.sin(2 * np.pi * 5.0 * t),
                      np.cos(2 * np.pi * 5.0 * t)], axis=1)
    c, *_ = np.linalg.lstsq(basis[mid], y[mid], rcond=None)
    _, h = sps.sosfreqz(sc.design("bp8"), worN=[20.0, 5.0], fs=sc.FS)
    g20, g5 = np.abs(h) ** 2
    a20, a5 = float(np.hypot(c[0], c[1])), float(np.hypot(c[2], c[3]))
    print("f two tones: 20 Hz amplitude %.8f (|H|^2 %.8f), 5 Hz amplitude %.2e (|H|^2 %.2e)" % (a20, g20, a5, g5))
    assert abs(a20 - g20) < sc.TOL and a5 < sc.TOL and g5 < sc.TOL
    assert np.max(np.abs(y[mid] - basis[mid] @ c)) < sc.TOL            # nothing but the two tones comes back
