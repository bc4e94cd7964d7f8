"""Time the alignment against the beam (csrc/align.hip, loc.refine_arrivals) on a resident CUDA block: HIP events around each
call, warm-ups first, median (and spread) of --reps calls.

Per shape (default 11020 x 12000, one 60-s file at 200 Hz), for 1, 8 and 64 calls with templates of --length samples and
--max-lag lags either side, the delay table built beforehand (delays=...) and the starts spread over the file:
  * loc.refine_arrivals (Ti and coef only, as a user calls it);
  * a plain device copy of ncalls x channels x (L + 2M) x 4 bytes: the words of the block the kernel reads;
  * the PyTorch composition of the same definition a user could write today: per call a gather of every channel's window, its
    2M + 1 shifted views (unfold), one einsum with the template, the window energies, the quotient and an argmax.  It is timed
    for one call over all channels and scaled by the number of calls (its calls are a Python loop, each costs the same); its
    largest difference from the kernel's coefficients and the share of equal lags are reported.
Beside the times: terms = ncalls channels (2M + 1) L, terms per second and multiply-adds per second (two per term).  Prints one
JSON line; --out also writes it to a file.

    python scripts/time_align.py [--reps 10] [--shapes 11020x12000] [--calls 1,8,64] [--length 400] [--max-lag 20] [--out profiles/align/time_align.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import das4whales_amd as dw  # noqa: E402
from scripts.time_beam import C0, FS, _timed, geometry  # noqa: E402

CALLS = (1, 8, 64)


def torch_composition(x, t, n0, M):
    """One call by whole-array torch operations: (coef [nch], lag [nch]) for windows that all lie inside the block."""
    nch, L = x.shape[0], t.shape[0]
    idx = (n0 - M)[:, None] + torch.arange(L + 2 * M, dtype=torch.int64, device=x.device)[None, :]
    w = torch.gather(x, 1, idx).unfold(1, L, 1)                       # [nch x (2M + 1) x L], a view of the gathered windows
    dot = torch.einsum("cml,l->cm", w, t)
    en = torch.einsum("cml,cml->cm", w, w)
    rho = dot / torch.sqrt((t * t).sum() * en)
    coef, i = rho.max(1)
    return coef, i - M


def time_block(nch, ns, L, M, reps, warmup, calls=CALLS):
    g = torch.Generator(device="cuda").manual_seed(nch + ns)
    x = torch.empty((nch, ns), dtype=torch.float32, device="cuda")
    for r0 in range(0, nch, 2048):                                    # in slabs: no second block-sized temporary
        x[r0:r0 + 2048].normal_(generator=g)
    out = {"shape": [nch, ns], "reps": reps, "fs": FS, "length": L, "max_lag": M, "block_GB": nch * ns * 4 / 1e9,
           "limits": dict(zip(("max_calls", "max_length", "max_lag", "channels_per_workgroup"), dw.loc.align_limits())), "runs": []}
    for ncalls in calls:
        cable, pos = geometry(nch, ncalls)
        cable_d, pos_d = torch.from_numpy(cable).cuda(), torch.from_numpy(pos).cuda()
        r = dw.loc.beam_delays(cable_d, C0, FS, pos_d, rounded=True)
        room = ns - L - 2 * M - int(r.max()) - 1                      # every window inside the block
        assert room > 0, "the block is too short for these delays"
        start = torch.from_numpy(M + (np.arange(ncalls) * 997) % room).cuda()
        t = torch.randn((ncalls, L), dtype=torch.float32, device="cuda", generator=g)
        run = {"ncalls": ncalls, "terms": ncalls * nch * (2 * M + 1) * L, "block_words_read_GB": ncalls * nch * (L + 2 * M) * 4 / 1e9}
        run["refine_arrivals"] = _timed(lambda: dw.loc.refine_arrivals(x, FS, cable_d, C0, pos_d, t, start, M, delays=r), reps, warmup)
        ms = run["refine_arrivals"]["median_ms"]
        run["terms_per_s"] = run["terms"] / (ms * 1e-3)
        run["fma_per_s"] = 2 * run["terms_per_s"]
        src = torch.empty(ncalls * nch * (L + 2 * M), dtype=torch.float32, device="cuda")
        dst = torch.empty_like(src)
        run["copy_of_the_same_bytes"] = _timed(lambda: dst.copy_(src), reps, warmup)
        run["kernel_over_copy"] = ms / run["copy_of_the_same_bytes"]["median_ms"]
        del src, dst
        n0 = start[0] + r[0].to(torch.int64)
        base = _timed(lambda: torch_composition(x, t[0], n0, M), max(3, reps // 3), 1)
        base["scaled_to_the_calls_ms"] = base["median_ms"] * ncalls
        base["over_kernel"] = base["scaled_to_the_calls_ms"] / ms
        _, coef, lag, _ = dw.loc.refine_arrivals(x, FS, cable_d, C0, pos_d, t, start, M, -1.0, return_all=True, delays=r)
        rc, rl = torch_composition(x, t[0], n0, M)
        base["max_abs_coef_difference"] = float((coef[0] - rc).abs().max())
        base["equal_lags"] = float((lag[0] == rl).float().mean())
        run["torch_composition"] = base
        print(json.dumps(run), flush=True)
        out["runs"].append(run)
        del coef, lag, rc, rl
        torch.cuda.empty_cache()
    del x
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="11020x12000")
    ap.add_argument("--calls", default=",".join(str(c) for c in CALLS))
    ap.add_argument("--length", type=int, default=400)
    ap.add_argument("--max-lag", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU: there is no CPU fallback"
    shapes = [[int(v) for v in s.split("x")] for s in a.shapes.split(",")]
    res = {"device": torch.cuda.get_device_name(0),
           "blocks": [time_block(nch, ns, a.length, a.max_lag, a.reps, a.warmup, [int(v) for v in a.calls.split(",")]) for nch, ns in shapes]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
