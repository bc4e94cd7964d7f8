"""Time the coherence of located calls (csrc/coherence.hip, loc.beam_coherence) on a resident CUDA block against the
delay-and-sum beam it shares its gather with: HIP events around each call, warm-ups first, the forms ALTERNATING inside every
repetition, median (and spread) of --reps repetitions.

Per shape (default 11020 x 12000, one 60-s file at 200 Hz), for 1 and 64 calls and orders 0 and 3, with the delay tables built
beforehand, start 0, the file's length and preallocated outputs and workspaces, all through the C ABI:
  * d4w_beamform_f32(normalize = 1) of --baseline-lib (a build of the commit to compare with), where one is given;
  * d4w_beamform_f32(normalize = 1) of the packaged library;
  * d4w_coherence_f32 + d4w_coherence_peak_f32, semblance only, at half window --half (default 100) -- and for the first
    configuration also at 0 and at the limit: what the window costs;
  * the same with the imaginary block (phase coherence).
Beside them loc.beam_coherence through the public interface (allocations, the time axis and the peak included).
Prints one JSON line; --out also writes it to a file.

    python scripts/time_coherence.py [--reps 10] [--shapes 11020x12000] [--calls 1,64] [--orders 0,3] [--half 100]
                                     [--baseline-lib path/to/libd4w.so] [--out profiles/coherence/time_coherence.json]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import das4whales_amd as dw  # noqa: E402
from das4whales_amd import _lib  # noqa: E402
from scripts.time_beam import C0, FS, geometry  # noqa: E402

I64 = ctypes.c_int64


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating(forms, reps, warmup):
    """forms: {name: callable}.  Every repetition times each form once, in turn; {name: median / min / max in ms}."""
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            ms[name].append(event_ms(fn))
    return {name: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))} for name, v in ms.items()}


def load_baseline(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    lib.d4w_last_error.restype = ctypes.c_char_p
    for name in ("d4w_beam_ws_bytes", "d4w_beamform_f32"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = _lib.SIGNATURES[name][1]
    return lib


def time_block(nch, ns, reps, warmup, calls, orders, half, baseline):
    g = torch.Generator(device="cuda").manual_seed(nch + ns)
    x, y = (torch.empty((nch, ns), dtype=torch.float32, device="cuda") for _ in range(2))
    for r0 in range(0, nch, 2048):                                    # in slabs: no block-sized temporary
        x[r0:r0 + 2048].normal_(generator=g)
        y[r0:r0 + 2048].normal_(generator=g)                          # stands for the Hilbert transform: the kernel's work is the same
    limits = dict(zip(("max_calls", "max_length", "max_half_window", "segment"), dw.loc.coherence_limits()))
    out = {"shape": [nch, ns], "reps": reps, "fs": FS, "half_window": half, "limits": limits, "runs": []}
    first = True
    for ncalls in calls:
        cable, pos = geometry(nch, ncalls)
        cable_d, pos_d = torch.from_numpy(cable).cuda(), torch.from_numpy(pos).cuda()
        start = torch.zeros(ncalls, dtype=torch.int64, device="cuda")
        outs = [torch.empty((ncalls, ns), dtype=torch.float32, device="cuda") for _ in range(4)]
        peak, index = torch.empty(ncalls, dtype=torch.float32, device="cuda"), torch.empty(ncalls, dtype=torch.int32, device="cuda")
        n = ctypes.c_size_t()
        _lib.check(_lib.lib.d4w_coherence_ws_bytes(nch, ncalls, ns, 1, ctypes.byref(n)))
        ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")    # the largest of the workspaces: shared by every form
        for order in orders:
            d = dw.loc.beam_delays(cable_d, C0, FS, pos_d, rounded=order == 0)
            kr, f = (d, None) if order == 0 else d

            def beam(lib):
                rc = lib.d4w_beamform_f32(ptr(x), I64(ns), nch, ns, None, I64(0), 0, ptr(kr), ptr(f), None, ptr(start), ncalls, ns, order, 1, ptr(outs[0]),
                                          ptr(ws), stream())
                assert rc == 0, lib.d4w_last_error()

            def coherence(H, phase):
                rc = _lib.lib.d4w_coherence_f32(ptr(x), I64(ns), nch, ns, None, I64(0), 0, ptr(y) if phase else None, I64(ns), None, I64(0), ptr(kr), ptr(f),
                                                None, ptr(start), ncalls, ns, order, H, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]) if phase else None,
                                                ptr(outs[3]), ptr(ws), stream())
                assert rc == 0, _lib.lib.d4w_last_error()
                assert _lib.lib.d4w_coherence_peak_f32(ptr(outs[1]), ncalls, ns, 0, ns, ptr(peak), ptr(index), stream()) == 0

            forms = {}
            if baseline is not None:
                forms["beamform_normalize_baseline"] = lambda: beam(baseline)
            forms["beamform_normalize"] = lambda: beam(_lib.lib)
            forms["semblance"] = lambda: coherence(half, False)
            forms["semblance_and_phase"] = lambda: coherence(half, True)
            if first:
                forms["semblance_H0"] = lambda: coherence(0, False)
                forms["semblance_Hmax"] = lambda: coherence(limits["max_half_window"], False)
            forms["beam_coherence_public"] = lambda: dw.loc.beam_coherence(x, FS, cable_d, C0, pos_d, 0, ns, half, order, delays=d)
            run = {"ncalls": ncalls, "order": order, "ms": alternating(forms, reps, warmup)}
            ref = run["ms"].get("beamform_normalize_baseline", run["ms"]["beamform_normalize"])["median_ms"]
            run["over_the_beam"] = {name: v["median_ms"] / ref for name, v in run["ms"].items()}
            print(json.dumps(run), flush=True)
            out["runs"].append(run)
            first = False
        del outs, ws
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="11020x12000")
    ap.add_argument("--calls", default="1,64")
    ap.add_argument("--orders", default="0,3")
    ap.add_argument("--half", type=int, default=100)
    ap.add_argument("--baseline-lib", default=None, help="a libd4w.so of the commit to compare with; its beamform is timed in turn with the rest")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU: there is no CPU fallback"
    base = load_baseline(a.baseline_lib) if a.baseline_lib else None
    shapes = [[int(v) for v in s.split("x")] for s in a.shapes.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "baseline_lib": bool(base),
           "blocks": [time_block(nch, ns, a.reps, a.warmup, [int(v) for v in a.calls.split(",")], [int(v) for v in a.orders.split(",")], a.half, base)
                      for nch, ns in shapes]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
