"""Time the received levels (csrc/levels.hip, loc.received_levels) on a resident CUDA block: HIP events around each call,
warm-ups first, median (and spread) of --reps calls.

Per shape (default 11020 x 12000, one 60-s file at 200 Hz) and number of calls (default 64), with the delay table built
beforehand (delays=...), device-resident arguments and the starts spread over the file so that every window lies inside the block:
  * loc.received_levels for each (L, N) of --windows (default 400x400 and 64x0), gap = --gap;
  * in the same process, as yardsticks from code that was there before: loc.beamform(order=0, length=L + N), which gathers the
    same number of samples per (call, channel) along the same moveout, and loc.refine_arrivals with a template of --length
    samples and --max-lag lags either side;
  * a plain device copy of ncalls x channels x (L + N) x 4 bytes: the words of the block the kernel reads.
Beside the times: the bytes of the block read and the bytes per second they amount to.  Prints one JSON line; --out also writes
it to a file.

    python scripts/time_levels.py [--reps 10] [--shapes 11020x12000] [--calls 64] [--windows 400x400,64x0] [--gap 0]
                                  [--length 400] [--max-lag 20] [--out profiles/levels/time_levels.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import das4whales_amd as dw  # noqa: E402
from scripts.time_beam import C0, FS, _timed, geometry  # noqa: E402


def time_block(nch, ns, windows, gap, tl, M, reps, warmup, calls):
    g = torch.Generator(device="cuda").manual_seed(nch + ns)
    x = torch.empty((nch, ns), dtype=torch.float32, device="cuda")
    for r0 in range(0, nch, 2048):                                    # in slabs: no second block-sized temporary
        x[r0:r0 + 2048].normal_(generator=g)
    out = {"shape": [nch, ns], "reps": reps, "fs": FS, "gap": gap, "block_GB": nch * ns * 4 / 1e9,
           "limits": dict(zip(("max_calls", "max_length", "channels_per_workgroup"), dw.loc.level_limits())), "runs": []}
    for ncalls in calls:
        cable, pos = geometry(nch, ncalls)
        cable_d, pos_d = torch.from_numpy(cable).cuda(), torch.from_numpy(pos).cuda()
        r = dw.loc.beam_delays(cable_d, C0, FS, pos_d, rounded=True)
        rmax = int(r.max())
        for L, N in windows:
            lead = N + gap + M                                        # the noise window and the leading lags inside the block
            room = ns - max(L, tl) - M - lead - rmax - 1
            assert room > 0, "the block is too short for these delays"
            start = torch.from_numpy(lead + (np.arange(ncalls) * 997) % room).cuda()
            nbytes = ncalls * nch * (L + N) * 4
            run = {"ncalls": ncalls, "length": L, "noise_length": N, "block_bytes_read_GB": nbytes / 1e9}
            run["received_levels"] = _timed(lambda: dw.loc.received_levels(x, FS, cable_d, C0, pos_d, start, L, N, gap, delays=r), reps, warmup)
            ms = run["received_levels"]["median_ms"]
            run["TB_per_s"] = nbytes / (ms * 1e-3) / 1e12
            run["beamform_order0_same_samples"] = _timed(lambda: dw.loc.beamform(x, FS, cable_d, C0, pos_d, start=start - N - gap, length=L + N,
                                                                                 order=0, delays=r), reps, warmup)
            run["beam_TB_per_s"] = nbytes / (run["beamform_order0_same_samples"]["median_ms"] * 1e-3) / 1e12
            run["levels_over_beam"] = ms / run["beamform_order0_same_samples"]["median_ms"]
            src = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
            dst = torch.empty_like(src)
            run["copy_of_the_same_bytes"] = _timed(lambda: dst.copy_(src), reps, warmup)
            run["levels_over_copy"] = ms / run["copy_of_the_same_bytes"]["median_ms"]
            del src, dst
            print(json.dumps(run), flush=True)
            out["runs"].append(run)
            torch.cuda.empty_cache()
        t = torch.randn((ncalls, tl), dtype=torch.float32, device="cuda", generator=g)
        start = torch.from_numpy(M + (np.arange(ncalls) * 997) % (ns - tl - 2 * M - rmax - 1)).cuda()
        ref = {"ncalls": ncalls, "length": tl, "max_lag": M, "block_bytes_read_GB": ncalls * nch * (tl + 2 * M) * 4 / 1e9}
        ref["refine_arrivals"] = _timed(lambda: dw.loc.refine_arrivals(x, FS, cable_d, C0, pos_d, t, start, M, delays=r), reps, warmup)
        ref["TB_per_s"] = ref["block_bytes_read_GB"] * 1e9 / (ref["refine_arrivals"]["median_ms"] * 1e-3) / 1e12
        print(json.dumps(ref), flush=True)
        out["runs"].append(ref)
    del x
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="11020x12000")
    ap.add_argument("--calls", default="64")
    ap.add_argument("--windows", default="400x400,64x0")
    ap.add_argument("--gap", type=int, default=0)
    ap.add_argument("--length", type=int, default=400)
    ap.add_argument("--max-lag", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU: there is no CPU fallback"
    shapes = [[int(v) for v in s.split("x")] for s in a.shapes.split(",")]
    windows = [tuple(int(v) for v in s.split("x")) for s in a.windows.split(",")]
    res = {"device": torch.cuda.get_device_name(0),
           "blocks": [time_block(nch, ns, windows, a.gap, a.length, a.max_lag, a.reps, a.warmup, [int(v) for v in a.calls.split(",")])
                      for nch, ns in shapes]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
