"""Time the localisation kernels of csrc/loc.hip on resident float64 CUDA tensors: HIP events around each public call,
warm-ups first, median (and spread) of --reps calls:
  solve_lq_batch   1, 64 and 1024 calls x 11 020 channels, 10 iterations, free z and fix_z
  misfit_grid      512 x 512 nodes x 11 020 channels, one call
Beside each, channel rows (or node-channel pairs) per second.  With --cpu the reference's iteration in NumPy (the arithmetic
of loc.py:86-120: rows by arctan2 / cos / sin, inv(G^T G + lambda I) @ G^T @ dt, without the printing) is timed on the same
host for ONE call -- run it with OMP_NUM_THREADS=1 for the one-core figure -- and the NumPy misfit grid for 16 rows of the
512 x 512 grid (scaled to 512).
Prints one JSON line; --out also writes it to a file.

    python scripts/time_loc.py [--reps 30] [--cpu] [--out profiles/loc/time_loc.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import das4whales_amd as dw  # noqa: E402
from tests import known_answers_loc as ka  # noqa: E402

NCH, C0 = 11020, 1490.0


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        y = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"reps": reps, "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}, y


def cpu_solve(Ti, cable, nbiter, fix_z):
    """The reference's iteration, written out (loc.py:86-120)."""
    n = np.array([40000.0, 23000.0, -60.0, Ti.min()])
    idx = [0, 1, 3] if fix_z else [0, 1, 2, 3]
    for j in range(nbiter):
        G = ka.g_rows(cable, n, C0, fix_z, "trig")
        dt = Ti - ka.arrival_times(n[3], cable, n[:3], C0)
        dn = np.linalg.inv(G.T @ G + 1e-5 * np.eye(G.shape[1])) @ G.T @ dt
        n[idx] += (0.7 if j < 4 else 1.0) * dn
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    cable = ka.make_cable("line", NCH)
    rng = np.random.default_rng(7)
    srcs = np.stack([rng.uniform(28000, 55000, 1024), rng.uniform(14000, 23000, 1024), np.full(1024, -60.0), rng.uniform(0, 30, 1024)], 1)
    Ti = np.stack([ka.arrival_times(s[3], cable, s[:3], C0) for s in srcs]) + 0.01 * rng.standard_normal((1024, NCH))
    dc, dT = torch.from_numpy(cable).cuda(), torch.from_numpy(Ti).cuda()
    runs = []
    for ncalls in (1, 64, 1024):
        for fix_z in (False, True):
            t = dT[:ncalls].contiguous()
            r, y = timed(lambda: dw.loc.solve_lq_batch(t, dc, C0, 10, fix_z), args.reps, args.warmup)
            r.update({"call": "solve_lq_batch", "ncalls": ncalls, "nch": NCH, "Nbiter": 10, "fix_z": fix_z,
                      "channel_rows_per_s": 11.0 * ncalls * NCH / (r["ms_median"] * 1e-3), "us_per_call": r["ms_median"] * 1e3 / ncalls,
                      "checksum": float(y.sum())})
            runs.append(r)
    xs, ys = np.linspace(25000.0, 60000.0, 512), np.linspace(10000.0, 40000.0, 512)
    dx, dy = torch.from_numpy(xs).cuda(), torch.from_numpy(ys).cuda()
    r, y = timed(lambda: dw.loc.misfit_grid(dT[0], dc, C0, dx, dy, -60.0), args.reps, args.warmup)
    r.update({"call": "misfit_grid", "ncalls": 1, "nch": NCH, "grid": [512, 512], "node_channels_per_s": 512.0 * 512 * NCH / (r["ms_median"] * 1e-3),
              "checksum": float(y[0].sum())})
    runs.append(r)
    if args.cpu:
        torch.set_num_threads(1)
        for fix_z in (False, True):
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                cpu_solve(Ti[0], cable, 10, fix_z)
                ts.append(time.perf_counter() - t0)
            runs.append({"call": "cpu solve, one call", "fix_z": fix_z, "nch": NCH, "Nbiter": 10, "ms_median": float(np.median(ts)) * 1e3, "runs": 5})
        t0 = time.perf_counter()
        ka.misfit_grid_f64(Ti[0], cable, C0, xs, ys[:16], -60.0)
        dt = time.perf_counter() - t0
        runs.append({"call": "cpu misfit grid, 16 of 512 rows", "ms": dt * 1e3, "ms_scaled_to_512_rows": dt * 1e3 * 32})
    res = {"kernels": "csrc/loc.hip: loc_solve<fix_z>, loc_misfit_grid", "device": torch.cuda.get_device_name(0),
           "cpu_baseline": "NumPy with the BLAS threads it was given (OMP_NUM_THREADS), same host" if args.cpu else None, "runs": runs}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
