"""Time the robust relocation (csrc/robust.hip, dw.loc.solve_robust_batch) against the unweighted solver it grew from, on
resident float64 CUDA tensors, in one run: HIP events around each public call, 2 warm-ups, the median (and spread) of 10 calls,
11 020 channels, Nbiter = 10, fix_z, 1 / 8 / 64 / 1024 calls:
  solve_lq_batch                       the parent's kernel, the yardstick
  solve_robust_batch l2                the same sums with weights of 1.0 (must cost what the yardstick costs)
  solve_robust_batch huber, bisquare   warmup 0: every iteration takes the median (two sweeps and the radix select)
  torch composition                    the same definition with batched torch.median and torch.linalg.solve
The alternation yardstick / l2 / huber / bisquare / torch is repeated per batch size, so that every ratio compares neighbours in
time.  The 10 % moved channels of tests/robust_cases.scene are in the arrival times: the select sees a realistic spread of |r|.
torch.median returns the LOWER of the two middle values of an even count; the composition averages the two middle order
statistics from torch.sort instead, to compute what the kernel computes (its largest position difference is printed).
Prints one JSON line; --out also writes it to a file.

    python scripts/time_robust.py [--out profiles/robust/time_robust.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import das4whales_amd as dw  # noqa: E402
from tests import known_answers_loc as ka  # noqa: E402

NCH, C0, NBITER = 11020, 1490.0, 10
REPS, WARMUP = 10, 2


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        y = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"reps": REPS, "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}, y


def torch_robust(Ti, cable, fg, loss, tuning):
    """The definition with torch's batched operations, fix_z, warmup 0, every channel used: [ncalls x 4]."""
    n = fg.clone()
    eye = 1e-5 * torch.eye(3, dtype=torch.float64, device=Ti.device)
    m = Ti.shape[1]
    for j in range(NBITER):
        d = n[:, None, :3] - cable[None, :, :]
        R = torch.sqrt((d * d).sum(2))
        r = Ti - (n[:, 3:4] + R / C0)
        srt = torch.sort(r.abs(), dim=1).values
        s = 1.4826 * (srt[:, (m - 1) // 2] + srt[:, m // 2]) * 0.5
        u = r.abs() / (tuning * s[:, None])
        q = torch.where(u <= 1, torch.ones_like(u), 1 / u) if loss == "huber" else torch.where(u < 1, (1 - u * u) ** 2, torch.zeros_like(u))
        q = torch.where((s > 0)[:, None], q, torch.ones_like(q))
        inv = 1.0 / (R * C0)
        G = torch.stack([d[:, :, 0] * inv, d[:, :, 1] * inv, torch.ones_like(inv)], dim=2)
        A = torch.einsum("cni,cn,cnk->cik", G, q, G) + eye
        b = torch.einsum("cni,cn->ci", G, q * r)
        dn = torch.linalg.solve(A, b)
        f = 0.7 if j < 4 else 1.0
        n = torch.stack([n[:, 0] + f * dn[:, 0], n[:, 1] + f * dn[:, 1], n[:, 2], n[:, 3] + f * dn[:, 2]], dim=1)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, nargs="*", default=[1, 8, 64, 1024])
    args = ap.parse_args()
    nmax = max(args.calls)
    cable = ka.make_cable("bent", NCH)
    rng = np.random.default_rng(7)
    srcs = np.stack([rng.uniform(33000, 43000, nmax), rng.uniform(19000, 27000, nmax), np.full(nmax, -60.0), rng.uniform(0, 30, nmax)], 1)
    Ti = np.stack([ka.arrival_times(s[3], cable, s[:3], C0) for s in srcs]) + 1e-3 * rng.standard_normal((nmax, NCH))
    moved = rng.random((nmax, NCH)) < 0.1
    Ti += np.where(moved, 0.05 * rng.choice([-1.0, 1.0], (nmax, NCH)), 0.0)
    fg = srcs + [300.0, -200.0, 0.0, 0.05]
    dc, dT, dF = torch.from_numpy(cable).cuda(), torch.from_numpy(Ti).cuda(), torch.from_numpy(fg).cuda()
    runs = []
    for ncalls in args.calls:
        t, f = dT[:ncalls].contiguous(), dF[:ncalls].contiguous()
        base, y0 = timed(lambda: dw.loc.solve_lq_batch(t, dc, C0, NBITER, True, f))
        base.update({"call": "solve_lq_batch", "ncalls": ncalls, "us_per_call": base["ms_median"] * 1e3 / ncalls})
        runs.append(base)
        for loss in ("l2", "huber", "bisquare"):
            r, y = timed(lambda: dw.loc.solve_robust_batch(t, dc, C0, loss=loss, Nbiter=NBITER, warmup=0, fix_z=True, first_guess=f))
            r.update({"call": "solve_robust_batch " + loss, "ncalls": ncalls, "us_per_call": r["ms_median"] * 1e3 / ncalls,
                      "ratio_to_solve_lq_batch": r["ms_median"] / base["ms_median"]})
            if loss == "l2":
                r["equals_solve_lq_batch"] = bool(torch.equal(y, y0))
            runs.append(r)
            if loss != "l2":
                tuning = 1.345 if loss == "huber" else 4.685
                rt, yt = timed(lambda: torch_robust(t, dc, f, loss, tuning))
                rt.update({"call": "torch composition " + loss, "ncalls": ncalls, "us_per_call": rt["ms_median"] * 1e3 / ncalls,
                           "ratio_to_solve_robust_batch": rt["ms_median"] / r["ms_median"],
                           "largest_position_difference_m": float((yt[:, :2] - y[:, :2]).abs().max())})
                runs.append(rt)
    res = {"kernels": "csrc/robust.hip: robust_solve<fix_z, resident>; csrc/loc.hip: loc_solve<fix_z>", "device": torch.cuda.get_device_name(0),
           "nch": NCH, "Nbiter": NBITER, "fix_z": True, "warmup_iterations": 0, "runs": runs}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
