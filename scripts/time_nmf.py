"""Time the window-normalised matched filter (csrc/nmf.hip, detect.compute_nmf_correlograms) on resident CUDA tensors: HIP events
around each call, warm-ups first, median (and spread) of --reps calls, the calls of a shape alternating.

Per shape (default 11020 x 12000, one 60-s file, and 20000 x 120000), HF + LF fin-whale pair:
  * detect.compute_cross_correlograms -- the yardstick: the peak-normalised matched filter (this change leaves its code alone);
  * the numerator alone (detect._matched_filter with the de-meaned supports, no tail);
  * the normaliser alone (d4w_nmf_normalise_f32 in place on a resident pair, with and without the row-maxima epilogue);
  * the whole public call detect.compute_nmf_correlograms (row statistics remembered from the first call, as for the yardstick);
  * a device-to-device copy of the block.
Every time is held against its algorithmic bytes (per sample: yardstick and numerator 12, normaliser 20, whole call 32) over
--copy-rate (TB/s).  The error against a float64 restatement is measured on the first --check-rows rows.  Prints one JSON
line; --out also writes it to a file.

    python scripts/time_nmf.py [--reps 20] [--shapes 11020x12000,20000x120000] [--out profiles/nmf/time_nmf.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import das4whales_amd as dw  # noqa: E402
from das4whales_amd._lib import lib, check  # noqa: E402

FS = 200.0


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


def _float64_nmf(x, template, center=True, floor=1e-6):
    """The definition in float64 (np.longdouble prefix sums for the windows) on a few rows."""
    t = np.asarray(template, dtype=np.float64)
    h = t[:int(np.nonzero(t)[0][-1]) + 1]
    hp = h - h.mean()
    m = len(hp)
    x = x.astype(np.float64)
    xe = np.zeros((x.shape[0], x.shape[1] + m - 1))
    xe[:, :x.shape[1]] = (x - x.mean(axis=1, keepdims=True)) / np.abs(x).max(axis=1, keepdims=True)
    xl = xe.astype(np.longdouble)
    z = np.zeros((x.shape[0], 1), dtype=np.longdouble)
    p1, p2 = np.concatenate((z, np.cumsum(xl, axis=1)), axis=1), np.concatenate((z, np.cumsum(xl * xl, axis=1)), axis=1)
    s1, s2 = p1[:, m:] - p1[:, :-m], p2[:, m:] - p2[:, :-m]
    V = (s2 - s1 * s1 / m if center else s2).astype(np.float64)
    c = np.stack([np.correlate(r, hp, "valid") for r in xe])
    live = V > floor * floor * m
    return np.where(live, c / (np.sqrt(np.sum(hp * hp)) * np.sqrt(np.where(live, V, 1.0))), 0.0)


def time_block(nx, ns, reps, warmup, copy_rate, check_rows):
    g = torch.Generator(device="cuda").manual_seed(nx + ns)
    x = torch.empty((nx, ns), dtype=torch.float32, device="cuda")
    for r0 in range(0, nx, 2048):                                     # in slabs: no second block-sized temporary
        x[r0:r0 + 2048].normal_(generator=g)
    x += 0.3
    t = np.arange(ns) / FS
    templates = [dw.detect.gen_template_fincall(t, FS, 17.8, 28.8, 0.68), dw.detect.gen_template_fincall(t, FS, 14.7, 21.8, 0.78)]
    parts = [dw.detect._nmf_parts(tp) for tp in templates]
    taps, ms_ = [h for h, _ in parts], [len(h) for h, _ in parts]
    mean, mx = dw.detect._row_stats_cached(x)
    pair = torch.empty((2, nx, ns), dtype=torch.float32, device="cuda")
    pair.uniform_(-1.0, 1.0, generator=g)
    rmax = [torch.empty(nx, dtype=torch.float32, device="cuda") for _ in range(2)]
    # norms that keep the in-place pair near its size over the repetitions (the time does not depend on the values)
    rms = float((x[:64] - x[:64].mean(dim=1, keepdim=True)).std()) / float(mx[:64].mean())
    norms = [1.0 / (rms * np.sqrt(m)) for m in ms_]
    st = torch.cuda.current_stream().cuda_stream

    def normalise(want_max):
        check(lib.d4w_nmf_normalise_f32(x.data_ptr(), nx, ns, None, 0, 0, mean.data_ptr(), mx.data_ptr(), 2, ms_[0], ms_[1], norms[0], norms[1],
                                        1, 1e-6, pair[0].data_ptr(), pair[1].data_ptr(), rmax[0].data_ptr() if want_max else None,
                                        rmax[1].data_ptr() if want_max else None, st))
    y = torch.empty_like(x)
    calls = {"compute_cross_correlograms (yardstick)": lambda: dw.detect.compute_cross_correlograms(x, templates),
             "numerator alone": lambda: dw.detect._matched_filter(x, taps, [0.0, 0.0]),
             "normaliser alone": lambda: normalise(False),
             "normaliser with row maxima": lambda: normalise(True),
             "compute_nmf_correlograms": lambda: dw.detect.compute_nmf_correlograms(x, templates),
             "copy": lambda: y.copy_(x)}
    out = {"shape": [nx, ns], "reps": reps, "block_GB": nx * ns * 4 / 1e9, "supports": ms_}
    out.update(_alternate(calls, reps, warmup))
    n = nx * ns
    _bound(out["compute_cross_correlograms (yardstick)"], 12 * n, copy_rate)
    _bound(out["numerator alone"], 12 * n, copy_rate)
    _bound(out["normaliser alone"], 20 * n, copy_rate)
    _bound(out["normaliser with row maxima"], 20 * n, copy_rate)
    _bound(out["compute_nmf_correlograms"], 32 * n, copy_rate)
    out["copy"]["read_plus_write_TB_s"] = n * 8 / (out["copy"]["median_ms"] * 1e-3) / 1e12
    yard = out["compute_cross_correlograms (yardstick)"]["median_ms"]
    out["nmf_over_yardstick"] = out["compute_nmf_correlograms"]["median_ms"] / yard
    out["normaliser_over_yardstick"] = out["normaliser alone"]["median_ms"] / yard
    rows = min(nx, check_rows)
    got = dw.detect.compute_nmf_correlograms(x[:rows].clone(), templates)
    xh = x[:rows].cpu().numpy()
    out["max_abs_err_vs_float64"] = [float(np.max(np.abs(g_.cpu().numpy() - _float64_nmf(xh, tp)))) for g_, tp in zip(got, templates)]
    out["max_abs_nmf"] = [float(g_.abs().max()) for g_ in got]
    del x, y, pair
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="11020x12000,20000x120000")
    ap.add_argument("--copy-rate", type=float, default=5.4)
    ap.add_argument("--check-rows", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU: there is no CPU fallback"
    shapes = [[int(v) for v in s.split("x")] for s in a.shapes.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "copy_rate_TB_s": a.copy_rate,
           "blocks": [time_block(nx, ns, a.reps, a.warmup, a.copy_rate, a.check_rows) for nx, ns in shapes]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
