"""Time the polyphase resampler (csrc/resample.hip) on resident CUDA tensors: HIP events around each call, warm-ups first,
median (and spread) of --reps calls, the calls of a shape alternating.

  * dsp.decimate(q = 5) and dsp.resample_poly(2, 5) on float32 blocks (default 11020 x 60000, one 60-s file at 1 kHz, and
    20000 x 120000), beside a device-to-device copy of the block and, at the first shape, what a user of the package could do
    without the kernel: torch.nn.functional.conv1d(stride = 5) with the same taps on the same tensor;
  * the fused ingest of an int32 and an int16 raw file (load_das_data_array(decimate = 5)) beside load_das_data_array
    followed by dsp.decimate;
  * scipy.signal.decimate(ftype = 'fir') on one core at --cpu-rows rows, scaled to the block.

Every kernel time is held against its algorithmic bytes -- (4 + 4 up / down) B per input sample for a float32 block, two reads
of the raw row + 4 / q B for the fused ingest -- over --copy-rate (TB/s; 5.4 = the resident-workgroup copy rate measured on
this part, README).  Results are compared once per shape, on the first rows, with SciPy.  Prints one JSON line; --out also
writes it to a file.

    python scripts/time_resample.py [--reps 20] [--shapes 11020x60000,20000x120000] [--out profiles/resample/time_resample.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import das4whales_amd as dw  # noqa: E402


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stat(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def _alternate(calls, reps, warmup):
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(reps):                                             # alternating: a drift of the machine meets all alike
        for k, fn in calls.items():
            ms[k].append(_event_ms(fn))
    return {k: _stat(v) for k, v in ms.items()}


def _bound(entry, nbytes, copy_rate):
    entry["algorithmic_GB"] = nbytes / 1e9
    entry["algorithmic_TB_s"] = nbytes / (entry["median_ms"] * 1e-3) / 1e12
    entry["time_over_bytes_at_copy_rate"] = entry["median_ms"] * 1e-3 / (nbytes / (copy_rate * 1e12))


def _rel_err(y, ref):
    return float(np.max(np.abs(y - ref).max(axis=1) / np.abs(ref).max(axis=1)))


def time_block(nx, ns, reps, warmup, copy_rate, conv1d):
    import scipy.signal as sps
    g = torch.Generator(device="cuda").manual_seed(nx + ns)
    x = torch.empty((nx, ns), dtype=torch.float32, device="cuda")
    for r0 in range(0, nx, 2048):                                     # in slabs: no second block-sized temporary
        x[r0:r0 + 2048].normal_(generator=g)
    x += 3.0
    y = torch.empty_like(x)
    calls = {"decimate q=5": lambda: dw.dsp.decimate(x, 5),
             "resample_poly 2/5": lambda: dw.dsp.resample_poly(x, 2, 5),
             "copy": lambda: y.copy_(x)}
    h = None
    if conv1d:
        h = torch.from_numpy(np.ascontiguousarray(dw.dsp._decimate_taps(5)[::-1], dtype=np.float32)).cuda().view(1, 1, -1)
        calls["torch conv1d stride 5"] = lambda: torch.nn.functional.conv1d(x[:, None, :], h, stride=5, padding=50)
    out = {"shape": [nx, ns], "reps": reps, "block_GB": nx * ns * 4 / 1e9}
    out.update(_alternate(calls, reps, warmup))
    _bound(out["decimate q=5"], nx * ns * (4 + 4 / 5), copy_rate)
    _bound(out["resample_poly 2/5"], nx * ns * (4 + 4 * 2 / 5), copy_rate)
    out["copy"]["read_plus_write_TB_s"] = nx * ns * 8 / (out["copy"]["median_ms"] * 1e-3) / 1e12
    for k in ("decimate q=5", "resample_poly 2/5"):
        out[k]["ratio_to_copy_of_the_block"] = out[k]["median_ms"] / out["copy"]["median_ms"]
    if conv1d:
        out["torch conv1d stride 5"]["ratio_to_decimate"] = out["torch conv1d stride 5"]["median_ms"] / out["decimate q=5"]["median_ms"]
    rows = min(nx, 4)
    xh = x[:rows].cpu().numpy().astype(np.float64)
    out["decimate_rel_err_vs_scipy"] = _rel_err(dw.dsp.decimate(x[:rows], 5).cpu().numpy(), sps.decimate(xh, 5, ftype="fir"))
    out["resample_poly_rel_err_vs_scipy"] = _rel_err(dw.dsp.resample_poly(x[:rows], 2, 5).cpu().numpy(),
                                                     sps.resample_poly(xh, 2, 5, axis=-1))
    del x, y
    torch.cuda.empty_cache()
    return out


def time_ingest(nx, ns, reps, warmup, copy_rate):
    import scipy.signal as sps
    meta = {"fs": 1000.0, "dx": 2.0419, "scale_factor": 1.7e-9}
    out = {"shape": [nx, ns], "reps": reps}
    for dtype, esz, amp, offset in ((torch.int32, 4, 1e5, 1e6), (torch.int16, 2, 1e3, 2e4)):
        g = torch.Generator(device="cuda").manual_seed(nx + esz)
        raw = torch.empty((nx, ns), dtype=dtype, device="cuda")
        for r0 in range(0, nx, 1024):
            raw[r0:r0 + 1024] = (torch.randn((min(1024, nx - r0), ns), generator=g, device="cuda") * amp + offset).to(dtype)
        sel = [0, nx, 1]
        calls = {"fused decimate=5": lambda: dw.data_handle.load_das_data_array(raw, sel, meta, decimate=5),
                 "ingest, then dsp.decimate": lambda: dw.dsp.decimate(dw.data_handle.load_das_data_array(raw, sel, meta)[0], 5)}
        res = _alternate(calls, reps, warmup)
        _bound(res["fused decimate=5"], nx * ns * (2 * esz + 4 / 5), copy_rate)
        _bound(res["ingest, then dsp.decimate"], nx * ns * (esz + 4 + 4 + 4 / 5), copy_rate)
        res["fused_over_two_step"] = res["fused decimate=5"]["median_ms"] / res["ingest, then dsp.decimate"]["median_ms"]
        rows = min(nx, 4)
        rh = raw[:rows].cpu().numpy().astype(np.float64)
        ref = sps.decimate((rh - rh.mean(axis=1, keepdims=True)) * meta["scale_factor"], 5, ftype="fir")
        res["rel_err_vs_scipy"] = _rel_err(dw.data_handle.load_das_data_array(raw, [0, rows, 1], meta, decimate=5)[0].cpu().numpy(), ref)
        out[str(dtype).replace("torch.", "")] = res
        del raw
        torch.cuda.empty_cache()
    return out


def time_cpu(nx, ns, cpu_rows):
    import scipy.signal as sps
    x = np.random.default_rng(1).standard_normal((cpu_rows, ns)).astype(np.float32)
    sps.decimate(x[:2], 5, ftype="fir")
    t0 = time.perf_counter()
    sps.decimate(x, 5, ftype="fir")
    dt = time.perf_counter() - t0
    return {"rows_timed": cpu_rows, "ns": ns, "seconds": dt, "scaled_to_rows": nx, "scaled_seconds": dt * nx / cpu_rows,
            "note": "scipy.signal.decimate(ftype='fir') on float32 rows, one call, whatever threads SciPy uses (upfirdn: one)"}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="11020x60000,20000x120000")
    ap.add_argument("--ingest-shape", default="11020x60000")
    ap.add_argument("--cpu-rows", type=int, default=64)
    ap.add_argument("--copy-rate", type=float, default=5.4)
    ap.add_argument("--no-conv1d", action="store_true")
    ap.add_argument("--no-ingest", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU: there is no CPU fallback"
    shapes = [[int(v) for v in s.split("x")] for s in a.shapes.split(",")]
    inx, ins = [int(v) for v in a.ingest_shape.split("x")]
    res = {"device": torch.cuda.get_device_name(0), "copy_rate_TB_s": a.copy_rate,
           "blocks": [time_block(nx, ns, a.reps, a.warmup, a.copy_rate, conv1d=(i == 0 and not a.no_conv1d))
                      for i, (nx, ns) in enumerate(shapes)],
           "ingest": None if a.no_ingest else time_ingest(inx, ins, a.reps, a.warmup, a.copy_rate),
           "scipy_one_core": time_cpu(shapes[0][0], shapes[0][1], a.cpu_rows)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
