"""Time tools.spec (Welch PSD of every 3000-sample chunk, csrc/welch.hip) and tools.energy_TimeDomain on a resident CUDA
tensor: HIP events around each call, warm-ups first, median (and spread) of --reps calls, at the file block
11020 x 12000 and at 20000 x 120000.  Beside each, in the same process and alternating with it, a device-to-device copy
of the same block: the project's measure of a one-pass kernel.  A copy moves 8 B / sample (read +
write), the two kernels read 4 B / sample and write next to nothing; the ratio kernel / copy is what is reported, with
the algorithmic read rate 4 nx ns / t.  The result of spec is compared once per shape, on the first rows, with
scipy.signal.welch.  Prints one JSON line; --out also writes it to a file.

    python scripts/time_welch.py [--reps 20] [--shapes 11020x12000,20000x120000] [--out profiles/welch/time_welch.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import das4whales_amd as dw  # noqa: E402


def _events(fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def _stat(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def time_shape(nx, ns, reps, warmup):
    g = torch.Generator(device="cuda").manual_seed(nx + ns)
    x = torch.empty((nx, ns), dtype=torch.float32, device="cuda")
    for r0 in range(0, nx, 2048):                                     # in slabs: no second block-sized temporary
        x[r0:r0 + 2048].normal_(generator=g)
    x += 3.0
    y = torch.empty_like(x)
    calls = {"spec": lambda: dw.tools.spec(x),
             "energy_TimeDomain chunk 3000": lambda: dw.tools.energy_TimeDomain(x, chunk=3000),
             "copy": lambda: y.copy_(x)}
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    import scipy.signal as sps
    rows = min(nx, 4)
    p = dw.tools.spec(x[:rows]).cpu().numpy().astype(np.float64)
    xh = x[:rows].cpu().numpy().astype(np.float64)
    ref = np.stack([sps.welch(xh[:, j * 3000:(j + 1) * 3000], fs=200, nperseg=1024)[1] for j in range(ns // 3000)], axis=1)
    err = float(np.max(np.abs(p - ref).reshape(rows, -1).max(axis=1) / ref.reshape(rows, -1).max(axis=1)))
    ms = {k: [] for k in calls}
    for _ in range(reps):                                             # alternating: a drift of the machine meets all alike
        for k, fn in calls.items():
            ms[k] += _events(fn, 1)
    out = {"shape": [nx, ns], "reps": reps, "spec_rel_err_vs_scipy": err, "block_GB": nx * ns * 4 / 1e9}
    for k in calls:
        out[k] = _stat(ms[k])
    for k in ("spec", "energy_TimeDomain chunk 3000"):
        out[k]["read_TB_s"] = nx * ns * 4 / (out[k]["median_ms"] * 1e-3) / 1e12
        out[k]["ratio_to_copy"] = out[k]["median_ms"] / out["copy"]["median_ms"]
    out["copy"]["read_plus_write_TB_s"] = nx * ns * 8 / (out["copy"]["median_ms"] * 1e-3) / 1e12
    del x, y
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="11020x12000,20000x120000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU: there is no CPU fallback"
    res = {"device": torch.cuda.get_device_name(0),
           "runs": [time_shape(*[int(v) for v in s.split("x")], a.reps, a.warmup) for s in a.shapes.split(",")]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
