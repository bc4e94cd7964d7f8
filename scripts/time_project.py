"""Time the transpose of the beam (csrc/project.hip; loc.project_calls, loc.subtract_calls) on a resident CUDA block: HIP events
around each call, warm-ups first, median (and spread) of --reps calls.

Per shape (default 11020 x 12000, one 60-s file at 200 Hz), number of calls (default 64) and beam length (default 400, and one
call of 64 samples as the small end), with the delay tables built beforehand (delays=...), device-resident arguments and the
starts spread over the file so that every support lies inside the block:
  * loc.project_calls for each order of --orders, and in the same process, as yardsticks from code that was there before,
    loc.received_levels(L, N = 0) and loc.beamform(order=0, length=L) on the same calls: they read the same samples;
  * loc.subtract_calls out of place against a torch copy of the block (what it costs to read and write every sample once);
  * loc.subtract_calls in place, against the bytes its supports cover (read and written) at the fit's rate.
Prints one JSON line; --out also writes it to a file.

    python scripts/time_project.py [--reps 10] [--shapes 11020x12000] [--calls 64] [--length 400] [--orders 0,1,3]
                                   [--out profiles/project/time_project.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import das4whales_amd as dw  # noqa: E402
from scripts.time_beam import C0, FS, _timed, geometry  # noqa: E402


def time_block(nch, ns, runs, orders, reps, warmup):
    g = torch.Generator(device="cuda").manual_seed(nch + ns)
    x = torch.empty((nch, ns), dtype=torch.float32, device="cuda")
    for r0 in range(0, nch, 2048):                                    # in slabs: no second block-sized temporary
        x[r0:r0 + 2048].normal_(generator=g)
    spare = torch.empty_like(x)
    out = {"shape": [nch, ns], "reps": reps, "fs": FS, "block_GB": nch * ns * 4 / 1e9,
           "limits": dict(zip(("max_calls", "max_length", "channels_per_workgroup"), dw.loc.project_limits())), "runs": []}
    out["block_copy"] = _timed(lambda: spare.copy_(x), reps, warmup)
    print("copy of the block %d x %d: %s" % (nch, ns, out["block_copy"]), flush=True)
    for ncalls, L in runs:
        cable, pos = geometry(nch, ncalls)
        cable_d, pos_d = torch.from_numpy(cable).cuda(), torch.from_numpy(pos).cuda()
        r = dw.loc.beam_delays(cable_d, C0, FS, pos_d, rounded=True)
        kf = dw.loc.beam_delays(cable_d, C0, FS, pos_d)
        room = ns - L - 8 - int(r.max())
        assert room > 0, "the block is too short for these delays"
        start = torch.from_numpy(2 + (np.arange(ncalls) * 997) % room).cuda()
        beam = torch.randn((ncalls, L), dtype=torch.float32, device="cuda", generator=g)
        yard = {"ncalls": ncalls, "length": L, "block_bytes_read_GB": ncalls * nch * L * 4 / 1e9}
        yard["received_levels"] = _timed(lambda: dw.loc.received_levels(x, FS, cable_d, C0, pos_d, start, L, delays=r), reps, warmup)
        yard["beamform_order0"] = _timed(lambda: dw.loc.beamform(x, FS, cable_d, C0, pos_d, start=start, length=L, order=0, delays=r), reps, warmup)
        print(json.dumps(yard), flush=True)
        out["runs"].append(yard)
        for order in orders:
            d = r if order == 0 else kf
            nbytes = ncalls * nch * (L + order) * 4
            run = {"ncalls": ncalls, "length": L, "order": order, "block_bytes_read_GB": nbytes / 1e9}
            run["project_calls"] = _timed(lambda: dw.loc.project_calls(x, FS, cable_d, C0, pos_d, beam, start, order, delays=d), reps, warmup)
            ms = run["project_calls"]["median_ms"]
            run["TB_per_s"] = nbytes / (ms * 1e-3) / 1e12
            run["fit_over_levels"] = ms / yard["received_levels"]["median_ms"]
            run["fit_over_beam"] = ms / yard["beamform_order0"]["median_ms"]
            amp = dw.loc.project_calls(x, FS, cable_d, C0, pos_d, beam, start, order, delays=d)[0]
            run["subtract_out_of_place"] = _timed(lambda: dw.loc.subtract_calls(x, FS, cable_d, C0, pos_d, beam, start, amp, order, delays=d), reps, warmup)
            run["subtract_over_copy"] = run["subtract_out_of_place"]["median_ms"] / out["block_copy"]["median_ms"]
            spare.copy_(x)                                            # in place on a copy: the block keeps its samples for the next run
            run["subtract_in_place"] = _timed(lambda: dw.loc.subtract_calls(spare, FS, cable_d, C0, pos_d, beam, start, amp, order, inplace=True,
                                                                            delays=d), reps, warmup)
            # the supports read and written once at the fit's rate: 2 x the fit's time (the union of the supports is smaller still)
            run["subtract_in_place_over_twice_the_fit"] = run["subtract_in_place"]["median_ms"] / (2.0 * ms)
            print(json.dumps(run), flush=True)
            out["runs"].append(run)
            del amp
            torch.cuda.empty_cache()
    del x, spare
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="11020x12000")
    ap.add_argument("--calls", default="64")
    ap.add_argument("--length", type=int, default=400)
    ap.add_argument("--orders", default="0,1,3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU: there is no CPU fallback"
    shapes = [[int(v) for v in s.split("x")] for s in a.shapes.split(",")]
    runs = [(int(v), a.length) for v in a.calls.split(",")] + [(1, 64)]           # the small end: one call, L = 64
    res = {"device": torch.cuda.get_device_name(0),
           "blocks": [time_block(nch, ns, runs, [int(v) for v in a.orders.split(",")], a.reps, a.warmup) for nch, ns in shapes]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
