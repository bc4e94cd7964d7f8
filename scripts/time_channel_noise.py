"""Time dsp.channel_noise (csrc/noise.hip noise_rows / row_quantile / row_moments) on a resident CUDA block: HIP events
around each call, warm-ups first, median (and spread) of --reps calls, the variants alternated.

Per shape (default 11020 x 12000, the one-read form; 20000x120000 is the long-row form):
  * dsp.channel_noise(x, (0.5,)) with how = "one_read" (where the rows fit) and how = "long_row", and with 8 quantiles;
  * the composition the package offered before for the same four outputs: dsp.envelope, d4w_row_median_f32 on the envelope,
    the envelope's row mean, d4w_row_var_f32, a row mean of squares;
  * detect.pick_times with one bar per channel against the scalar form, on the same block;
  * a plain device copy of the block, for scale.
B/sample = 4 x (time of the call) / (time of the copy / 2): the copy moves 8 bytes per sample.
Prints one JSON line; --out also writes it to a file.

    python scripts/time_channel_noise.py [--reps 10] [--shapes 11020x12000,20000x120000] [--out profiles/noise/time.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import das4whales_amd as dw  # noqa: E402
from das4whales_amd import _device as dev  # noqa: E402
from das4whales_amd._lib import check, lib  # noqa: E402


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _alternated(fns, reps, warmup):
    """{name: stats}: every round runs each variant once, so that drift of the machine falls on all of them alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(_event_ms(fn))
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))} for k, v in ms.items()}


def composition(x):
    """The four outputs from the calls the package had before: envelope -> median and mean of its rows; variance; mean square."""
    nx, ns = x.shape
    env = dw.dsp.envelope(x)
    med = torch.empty(nx, dtype=torch.float32, device=x.device)
    var = torch.empty(nx, dtype=torch.float32, device=x.device)
    check(lib.d4w_row_median_f32(dev.ptr(env), nx, ns, dev.ptr(med), dev.stream_ptr(x)))
    mean = env.mean(dim=1)
    check(lib.d4w_row_var_f32(dev.ptr(x), nx, ns, dev.ptr(var), dev.stream_ptr(x)))
    msq = torch.linalg.vector_norm(x, dim=1).square_() / ns
    return msq, var.sqrt_(), mean, med


def time_block(nx, ns, reps, warmup):
    g = torch.Generator(device="cuda").manual_seed(nx + ns)
    x = torch.empty((nx, ns), dtype=torch.float32, device="cuda")
    for r0 in range(0, nx, 2048):
        x[r0:r0 + 2048].normal_(generator=g)
    x *= torch.linspace(1.0, 30.0, nx, device="cuda")[:, None]
    fits = bool(lib.d4w_channel_noise_fits_lds(ns))
    q8 = (0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99)
    fns = {"composition": lambda: composition(x), "long_row": lambda: dw.dsp.channel_noise(x, (0.5,), how="long_row"),
           "long_row_nq8": lambda: dw.dsp.channel_noise(x, q8, how="long_row")}
    if fits:
        fns["one_read"] = lambda: dw.dsp.channel_noise(x, (0.5,), how="one_read")
        fns["one_read_nq8"] = lambda: dw.dsp.channel_noise(x, q8, how="one_read")
        fns["one_read_nq0"] = lambda: dw.dsp.channel_noise(x, (), how="one_read")
    fns["envelope_alone"] = lambda: dw.dsp.envelope(x)
    out = {"shape": [nx, ns], "reps": reps, "fits_lds": fits, "block_GB": nx * ns * 4 / 1e9}
    out.update(_alternated(fns, reps, warmup))
    spare = torch.empty_like(x)
    out.update(_alternated({"block_copy": lambda: spare.copy_(x)}, reps, warmup))
    del spare
    torch.cuda.empty_cache()
    per_byte = out["block_copy"]["median_ms"] / 8.0
    for k in fns:
        out[k]["bytes_per_sample_at_copy_rate"] = out[k]["median_ms"] / per_byte
    # agreement of the forms (the tests hold each against float64; this is the same block the times are of)
    ref = composition(x)
    got = dw.dsp.channel_noise(x, (0.5,))
    out["max_rel_difference_from_composition"] = [float(((a - b.reshape(a.shape)).abs().max() / a.abs().max())) for a, b in zip(ref, got)]
    # the pickers: one bar per channel against one bar
    env = dw.dsp.envelope(x)
    bars = got.env_quantiles[:, 0].contiguous()
    k = 4.0
    one = float(k * bars.median())
    one_d = torch.full((1,), one, dtype=torch.float32, device=x.device)
    picks = {"pick_times_scalar": lambda: dw.detect.pick_times(env, one),
             "pick_times_device_scalar": lambda: dw.detect.pick_times(env, dw.detect.Threshold(1.0, one_d)),
             "pick_times_per_channel_same_bars": lambda: dw.detect.pick_times(env, dw.detect.ChannelThreshold(1.0, torch.full_like(bars, one)))}
    out.update(_alternated(picks, reps, warmup))
    # k times each channel's own floor picks far fewer peaks; timed on its own, because the pickers size their index table by the
    # last call on the shape (a sparse call between two dense ones makes the next dense one run twice)
    out.update(_alternated({"pick_times_per_channel": lambda: dw.detect.pick_times(env, dw.detect.ChannelThreshold(k, bars))}, reps, warmup))
    out["picks"] = {"scalar": dw.detect.pick_times(env, one).total, "per_channel": dw.detect.pick_times(env, dw.detect.ChannelThreshold(k, bars)).total}
    del x, env
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="11020x12000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU: there is no CPU fallback"
    res = {"device": torch.cuda.get_device_name(0), "blocks": []}
    for s in a.shapes.split(","):
        nx, ns = (int(v) for v in s.split("x"))
        blk = time_block(nx, ns, a.reps, a.warmup)
        print(json.dumps(blk), flush=True)
        res["blocks"].append(blk)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
