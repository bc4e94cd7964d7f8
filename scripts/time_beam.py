"""Time the delay-and-sum beam (csrc/beam.hip, loc.beamform) on a resident CUDA block: HIP events around each call, warm-ups
first, median (and spread) of --reps calls.

Per shape (default 11020 x 12000, one 60-s file at 200 Hz), for 1, 8 and 64 calls and orders 0, 1 and 3, with the delay tables
built beforehand (delays=...), start 0 and the file's length:
  * loc.beamform;
  * a plain device copy of ncalls x channels x samples x 4 bytes (the block copied ncalls times): the words the beam reads;
  * the PyTorch composition of the same definition a user could write today: an index tensor as large as the file, one
    torch.gather per tap, the validity mask, and a sum over the channels.  It is timed for one call and scaled by the number
    of calls (its calls are a Python loop, each costs the same); its largest difference from the kernel's beam is reported.
Prints one JSON line; --out also writes it to a file.

    python scripts/time_beam.py [--reps 10] [--shapes 11020x12000] [--calls 1,8,64] [--orders 0,1,3] [--out profiles/beam/time_beam.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import das4whales_amd as dw  # noqa: E402

FS, C0, DX = 200.0, 1490.0, 2.0419
CALLS, ORDERS = (1, 8, 64), (0, 1, 3)
TAPS = {0: (0,), 1: (0, 1), 3: (-1, 0, 1, 2)}


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


def geometry(nch, ncalls):
    """A cable of nch channels at DX along x with a bow in y, 300 m down, and ncalls sources 1 - 6 km off it."""
    s = np.arange(nch) * DX
    cable = np.stack([s, 600.0 * np.sin(np.pi * s / max(s[-1], 1.0)), np.full(nch, -300.0)], axis=1)
    rng = np.random.default_rng(ncalls)
    pos = np.stack([rng.uniform(0.0, max(s[-1], 1.0), ncalls), rng.uniform(1000.0, 6000.0, ncalls), np.full(ncalls, -30.0)], axis=1)
    return cable, pos


def coefficients(order, f):
    """float32 tensors [nch], one per tap."""
    if order == 0:
        return (torch.ones_like(f),)
    if order == 1:
        return (1 - f, f)
    return (-f * (f - 1) * (f - 2) / 6, (f + 1) * (f - 1) * (f - 2) / 2, -(f + 1) * f * (f - 2) / 2, (f + 1) * f * (f - 1) / 6)


def torch_composition(x, kr, f, order, start, nt):
    """One call's beam [nt] by whole-array torch operations: q [nch x nt] int64, a gather per tap, the mask, the channel sum."""
    nch, ns = x.shape
    q = kr.to(torch.int64)[:, None] + (start + torch.arange(nt, dtype=torch.int64, device=x.device))[None, :]
    taps = TAPS[order]
    ok = (q + taps[0] >= 0) & (q + taps[-1] < ns)
    v = torch.zeros((nch, nt), dtype=torch.float32, device=x.device)
    for o, l in zip(taps, coefficients(order, f if f is not None else torch.zeros(nch, device=x.device))):
        v += l[:, None] * torch.gather(x, 1, (q + o).clamp_(0, ns - 1))
    return (v * ok).sum(0)


def time_block(nch, ns, reps, warmup, calls=CALLS, orders=ORDERS):
    g = torch.Generator(device="cuda").manual_seed(nch + ns)
    x = torch.empty((nch, ns), dtype=torch.float32, device="cuda")
    for r0 in range(0, nch, 2048):                                    # in slabs: no second block-sized temporary
        x[r0:r0 + 2048].normal_(generator=g)
    spare = torch.empty_like(x)
    out = {"shape": [nch, ns], "reps": reps, "fs": FS, "block_GB": nch * ns * 4 / 1e9, "limits": dict(zip(("max_calls", "max_length", "segment", "tile"), dw.loc.beam_limits())),
           "runs": []}
    copy = _timed(lambda: spare.copy_(x), reps, warmup)
    out["block_copy"] = copy
    print("copy of the block %d x %d: %s" % (nch, ns, copy), flush=True)
    for ncalls in calls:
        cable, pos = geometry(nch, ncalls)
        cable_d, pos_d = torch.from_numpy(cable).cuda(), torch.from_numpy(pos).cuda()
        for order in orders:
            d = dw.loc.beam_delays(cable_d, C0, FS, pos_d, rounded=order == 0)
            run = {"ncalls": ncalls, "order": order}
            run["beamform"] = _timed(lambda: dw.loc.beamform(x, FS, cable_d, C0, pos_d, 0, ns, order, delays=d), reps, warmup)
            ms = run["beamform"]["median_ms"]
            run["terms_per_s"] = ncalls * nch * ns / (ms * 1e-3)
            run["block_words_GB_per_s"] = ncalls * nch * ns * 4 / (ms * 1e-3) / 1e9
            run["copy_of_the_same_bytes_ms"] = copy["median_ms"] * ncalls
            run["beam_over_copy"] = ms / run["copy_of_the_same_bytes_ms"]
            kr, f = (d, None) if order == 0 else d
            base = _timed(lambda: torch_composition(x, kr[0], f[0] if f is not None else None, order, 0, ns), max(3, reps // 3), 1)
            base["scaled_to_the_calls_ms"] = base["median_ms"] * ncalls
            base["over_kernel"] = base["scaled_to_the_calls_ms"] / ms
            beam, _ = dw.loc.beamform(x, FS, cable_d, C0, pos_d, 0, ns, order, delays=d)
            ref = torch_composition(x, kr[0], f[0] if f is not None else None, order, 0, ns)
            base["max_abs_difference"] = float((beam[0] - ref).abs().max())
            base["max_abs_beam"] = float(beam[0].abs().max())
            run["torch_composition"] = base
            print(json.dumps(run), flush=True)
            out["runs"].append(run)
            del beam, ref
            torch.cuda.empty_cache()
    del x, spare
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="11020x12000")
    ap.add_argument("--calls", default=",".join(str(c) for c in CALLS), help="numbers of calls, e.g. 1 for a kernel trace of the single call")
    ap.add_argument("--orders", default=",".join(str(o) for o in ORDERS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU: there is no CPU fallback"
    shapes = [[int(v) for v in s.split("x")] for s in a.shapes.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "blocks": [time_block(nch, ns, a.reps, a.warmup, [int(v) for v in a.calls.split(",")], [int(v) for v in a.orders.split(",")])
                      for nch, ns in shapes]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
