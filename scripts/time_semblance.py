"""Time the local slant-stack semblance (csrc/semblance.hip, detect.local_semblance) on resident CUDA tensors: HIP events around
each call, warm-ups first, median (and spread) of --reps calls.

Per shape (default 11020 x 12000, one 60-s file, and 20000 x 120000), M = 10, 33 slownesses from -1/1400 to +1/1400 s/m at
dx = 2.0419 m and fs = 200 Hz, H = 25, no cube:
  * detect.local_semblance;
  * the same against the kernel's LDS-read model: per (slowness, channel, sample) (2M + 1)(1 + 1/3) ds_read_b32 words for the
    beam and (2H + 3) / 3 ds_read_b64 for the windows, 32 lanes per clock and compute unit either way, at --clock-ghz;
  * a straightforward PyTorch composition of the same definition (shifted views of a zero-padded block, lerp, window sums by
    avg_pool1d times 2H + 1, running maximum over the slownesses), the baseline a user could write today.  It runs on the
    first --baseline-rows channels and its time is scaled to the block by the channel count (every channel costs the same);
    its largest difference from the kernel's coh on those channels is reported.
Prints one JSON line; --out also writes it to a file.

    python scripts/time_semblance.py [--reps 10] [--shapes 11020x12000,20000x120000] [--out profiles/semblance/time_semblance.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import das4whales_amd as dw  # noqa: E402

FS, DX, M, NP, H, T = 200.0, 2.0419, 10, 33, 25, 3


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = [_event_ms(fn) for _ in range(reps)]
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def torch_composition(x, delays, half_window):
    """(coh, idx) of x [nx, ns] by whole-array torch operations, float32, weights of one."""
    nx, ns = x.shape
    npj, n = delays.shape
    m_half = (n - 1) // 2
    k = np.floor(delays)
    f = (delays - k).astype(np.float32)
    k = k.astype(np.int64)
    pad = int(np.abs(k).max()) + 2
    xp = torch.zeros((nx + 2 * m_half, ns + 2 * pad), dtype=torch.float32, device=x.device)
    xp[m_half:m_half + nx, pad:pad + ns] = x
    chan = torch.arange(nx, device=x.device)
    W = sum(((chan + m >= 0) & (chan + m < nx)).to(torch.float32) for m in range(-m_half, m_half + 1))
    best = torch.zeros((nx, ns), dtype=torch.float32, device=x.device)
    arg = torch.zeros((nx, ns), dtype=torch.uint8, device=x.device)
    for j in range(npj):
        b = torch.zeros((nx, ns), dtype=torch.float32, device=x.device)
        e = torch.zeros_like(b)
        for m in range(-m_half, m_half + 1):
            kk = int(k[j, m + m_half])
            v0 = xp[m_half + m:m_half + m + nx, pad + kk:pad + kk + ns]
            v1 = xp[m_half + m:m_half + m + nx, pad + kk + 1:pad + kk + 1 + ns]
            xi = torch.lerp(v0, v1, float(f[j, m + m_half]))
            b += xi
            e.addcmul_(xi, xi)
        # (a mean over 2H + 1 samples with the zero padding counted: times 2H + 1 it is the window sum)
        pool = dict(kernel_size=2 * half_window + 1, stride=1, padding=half_window, count_include_pad=True)
        N = torch.nn.functional.avg_pool1d((b * b)[None], **pool)[0] * float(2 * half_window + 1)
        den = torch.nn.functional.avg_pool1d(e[None], **pool)[0] * float(2 * half_window + 1) * W[:, None]
        S = torch.where(den > 0, N / den, torch.zeros_like(N))
        better = S > best
        best = torch.where(better, S, best)
        arg = torch.where(better, torch.full_like(arg, j), arg)
    return best, arg


def time_block(nx, ns, reps, warmup, clock_ghz, baseline_rows):
    g = torch.Generator(device="cuda").manual_seed(nx + ns)
    x = torch.empty((nx, ns), dtype=torch.float32, device="cuda")
    for r0 in range(0, nx, 2048):                                     # in slabs: no second block-sized temporary
        x[r0:r0 + 2048].normal_(generator=g)
    s = np.linspace(-1.0 / 1400.0, 1.0 / 1400.0, NP)
    d = dw.detect.slowness_delays(s, DX, FS, M)
    out = {"shape": [nx, ns], "reps": reps, "half_aperture": M, "slownesses": NP, "half_window": H,
           "max_abs_delay_samples": float(np.abs(d).max()), "block_GB": nx * ns * 4 / 1e9}
    out["local_semblance"] = _timed(lambda: dw.detect.local_semblance(x, d, H), reps, warmup)
    print("local_semblance %d x %d: %s" % (nx, ns, out["local_semblance"]), flush=True)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    clocks = (2 * M + 1) * (1 + 1 / T) / 32 + (2 * H + T) / T / 32   # per (slowness, channel, sample) and compute unit
    model_ms = NP * nx * ns * clocks / (cus * clock_ghz * 1e9) * 1e3
    out["lds_model"] = {"compute_units": cus, "clock_GHz": clock_ghz, "lds_clocks_per_element": clocks, "model_ms": model_ms,
                        "fraction_of_model_limit": model_ms / out["local_semblance"]["median_ms"]}
    out["elements_per_s"] = NP * nx * ns / (out["local_semblance"]["median_ms"] * 1e-3)
    rows = min(nx, baseline_rows)
    xs = x[:rows].contiguous()
    base = _timed(lambda: torch_composition(xs, d, H), max(2, reps // 5), 1)
    base["rows"] = rows
    base["scaled_to_block_ms"] = base["median_ms"] * nx / rows
    base["over_kernel"] = base["scaled_to_block_ms"] / out["local_semblance"]["median_ms"]
    coh, idx = dw.detect.local_semblance(xs, d, H)
    cb, ib = torch_composition(xs, d, H)
    base["max_abs_coh_difference"] = float((coh - cb).abs().max())
    base["idx_agree_fraction"] = float((idx == ib).float().mean())
    out["torch_composition"] = base
    del x, xs
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="11020x12000,20000x120000")
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--baseline-rows", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU: there is no CPU fallback"
    shapes = [[int(v) for v in s.split("x")] for s in a.shapes.split(",")]
    res = {"device": torch.cuda.get_device_name(0),
           "blocks": [time_block(nx, ns, a.reps, a.warmup, a.clock_ghz, a.baseline_rows) for nx, ns in shapes]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
