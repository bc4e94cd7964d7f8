"""Time the STA/LTA detector (csrc/stalta.hip) on resident CUDA tensors: HIP events around each launch, warm-ups first, median
(and spread) of --reps launches, the calls of a shape alternating so that a drift of the machine meets all alike.

Per shape (default 11020 x 12000, one 60-s file, and 20000 x 120000), (nsta, nlta, gap) = (100, 2000, 100), unit noise with a
burst every 15 s, an explicit scale:
  * d4w_stalta_f32 -> ratio, classic and recursive (8 B per sample);
  * d4w_trigger_onset_f32 on the classic ratio (4 B per sample);
  * d4w_stalta_f32 -> events only, classic and recursive (the fused form: 4 B per sample);
  * detect.sta_lta_events, the public fused call (thresholds, one host synchronisation, packing);
  * yardsticks in the same process: d4w_nmf_normalise_f32 for one template of support 2000 (12 B per sample, the nearest relative)
    and a device-to-device copy of the block (8 B per sample).
Every time is held against its algorithmic bytes over --hbm-peak (TB/s, the specified peak) and over the copy's own rate.
Prints one JSON line and a table; --out writes both to a file.

    python scripts/time_stalta.py [--reps 20] [--shapes 11020x12000,20000x120000] [--out profiles/stalta/time.txt]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import das4whales_amd as dw  # noqa: E402
from das4whales_amd._lib import lib, check  # noqa: E402

NSTA, NLTA, GAP, ON, OFF, CAP = 100, 2000, 100, 3.0, 1.5, 64


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _alternate(calls, reps, warmup):
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            ms[k].append(_event_ms(fn))
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))} for k, v in ms.items()}


def time_block(nx, ns, reps, warmup, hbm_peak):
    g = torch.Generator(device="cuda").manual_seed(nx + ns)
    x = torch.empty((nx, ns), dtype=torch.float32, device="cuda")
    for r0 in range(0, nx, 2048):                                     # in slabs: no second block-sized temporary
        x[r0:r0 + 2048].normal_(generator=g)
    for k in range(2500, ns - 200, 3000):
        x[:, k:k + 200] *= 4.0
    y = torch.empty_like(x)                                           # the ratio; the copy's and the NMF pass's destination
    scale = torch.ones(nx, dtype=torch.float32, device="cuda")
    on = torch.full((nx,), ON, dtype=torch.float64, device="cuda")
    off = torch.full((nx,), OFF, dtype=torch.float64, device="cuda")
    ev = torch.empty((nx, CAP, 3), dtype=torch.int32, device="cuda")
    pk = torch.empty((nx, CAP), dtype=torch.float32, device="cuda")
    cnt = torch.empty(nx, dtype=torch.int32, device="cuda")
    act = torch.empty(nx, dtype=torch.int32, device="cuda")
    rout = torch.empty((nx, 2), dtype=torch.float64, device="cuda")
    mean, mx = dw.detect._row_stats_cached(x)
    st = torch.cuda.current_stream().cuda_stream

    def stalta(form, ratio, events):
        check(lib.d4w_stalta_f32(x.data_ptr(), ns, nx, ns, None, 0, 0, form, NSTA, NLTA, GAP if form == 0 else 0, 1e-6, scale.data_ptr(), None,
                                 rout.data_ptr() if form else None, 0, y.data_ptr() if ratio else None, ns if ratio else 0,
                                 on.data_ptr() if events else None, off.data_ptr() if events else None, None, act.data_ptr() if events else None,
                                 ev.data_ptr() if events else None, pk.data_ptr() if events else None, cnt.data_ptr() if events else None,
                                 CAP if events else 0, st))

    def trigger():
        check(lib.d4w_trigger_onset_f32(y.data_ptr(), ns, nx, ns, on.data_ptr(), off.data_ptr(), None, act.data_ptr(), ev.data_ptr(), pk.data_ptr(),
                                        cnt.data_ptr(), CAP, st))

    def nmf():
        check(lib.d4w_nmf_normalise_f32(x.data_ptr(), nx, ns, None, 0, 0, mean.data_ptr(), mx.data_ptr(), 1, NLTA, NLTA, 1.0, 1.0, 1, 1e-6,
                                        y.data_ptr(), None, None, None, st))
    stalta(0, True, False)                                            # the classic ratio the trigger is timed on ...
    ratio = y.clone() if nx * ns <= (1 << 28) else None
    calls = {"sta_lta classic": lambda: stalta(0, True, False),
             "trigger_onset": trigger,                                # (y holds the classic ratio: it runs right after it)
             "sta_lta recursive": lambda: stalta(1, True, False),
             "fused classic": lambda: stalta(0, False, True),
             "fused recursive": lambda: stalta(1, False, True),
             "sta_lta_events (public, classic)": lambda: dw.detect.sta_lta_events(x, NSTA, NLTA, ON, OFF, gap=GAP, scale=scale),
             "copy": lambda: y.copy_(x),
             "nmf_normalise (1 template, support 2000)": nmf}
    order = ["sta_lta classic", "trigger_onset", "sta_lta recursive", "fused classic", "fused recursive", "sta_lta_events (public, classic)",
             "copy", "nmf_normalise (1 template, support 2000)"]
    out = {"shape": [nx, ns], "reps": reps, "block_GB": nx * ns * 4 / 1e9}
    res = _alternate({k: calls[k] for k in order}, reps, warmup)
    n = nx * ns
    per_sample = {"sta_lta classic": 8, "trigger_onset": 4, "sta_lta recursive": 8, "fused classic": 4, "fused recursive": 4,
                  "sta_lta_events (public, classic)": 4, "copy": 8, "nmf_normalise (1 template, support 2000)": 12}
    copy_rate = n * 8 / (res["copy"]["median_ms"] * 1e-3) / 1e12
    for k, e in res.items():
        e["bytes_per_sample"] = per_sample[k]
        e["algorithmic_TB_s"] = per_sample[k] * n / (e["median_ms"] * 1e-3) / 1e12
        e["fraction_of_hbm_peak"] = e["algorithmic_TB_s"] / hbm_peak
        e["fraction_of_copy_rate"] = e["algorithmic_TB_s"] / copy_rate
    out["calls"] = res
    out["copy_TB_s"] = copy_rate
    out["fused_over_ratio_plus_trigger"] = res["fused classic"]["median_ms"] / (res["sta_lta classic"]["median_ms"] + res["trigger_onset"]["median_ms"])
    stalta(0, False, True)
    out["events_per_row_mean"] = float(cnt.float().mean())
    if ratio is not None:                                             # the fused events against the composition's, on the block timed
        a = dw.detect.sta_lta_events(x, NSTA, NLTA, ON, OFF, gap=GAP, scale=scale)
        b = dw.detect.trigger_onset(ratio, ON, OFF)
        out["fused_equals_composition"] = bool(torch.equal(a.packed, b.packed) and torch.equal(a.packed_peak, b.packed_peak))
    del x, y
    torch.cuda.empty_cache()
    return out


def table(res):
    lines = ["%s, HBM peak taken as %.1f TB/s" % (res["device"], res["hbm_peak_TB_s"])]
    for b in res["blocks"]:
        lines.append("")
        lines.append("%d x %d (%.2f GB), median of %d, (%d, %d, %d); copy %.2f TB/s; %.1f events per row; fused / (ratio + trigger) = %.2f"
                     % (b["shape"][0], b["shape"][1], b["block_GB"], b["reps"], NSTA, NLTA, GAP, b["copy_TB_s"], b["events_per_row_mean"],
                        b["fused_over_ratio_plus_trigger"]))
        lines.append("%-44s %9s %9s %9s %5s %8s %8s %8s" % ("call", "median ms", "min", "max", "B/smp", "TB/s", "of peak", "of copy"))
        for k, e in b["calls"].items():
            lines.append("%-44s %9.3f %9.3f %9.3f %5d %8.2f %8.2f %8.2f" % (k, e["median_ms"], e["min_ms"], e["max_ms"], e["bytes_per_sample"],
                                                                          e["algorithmic_TB_s"], e["fraction_of_hbm_peak"], e["fraction_of_copy_rate"]))
    return "\n".join(lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="11020x12000,20000x120000")
    ap.add_argument("--hbm-peak", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU: there is no CPU fallback"
    shapes = [[int(v) for v in s.split("x")] for s in a.shapes.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_TB_s": a.hbm_peak,
           "blocks": [time_block(nx, ns, a.reps, a.warmup, a.hbm_peak) for nx, ns in shapes]}
    text = table(res) + "\n\n" + json.dumps(res) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
