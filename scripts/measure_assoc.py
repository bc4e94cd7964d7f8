"""Timing of loc.vote_grid / loc.associate_picks (csrc/assoc.hip) on one realistic shape, with device events:
the 11 020-channel "line" cable, ~2e5 picks (16 calls on 70 % of the channels plus uniform clutter), a 97 x 97 grid,
dt = 0.25 s, max_calls = 16.  Prints the initial vote (time and (pick, node) pair evaluations per second), one association
round (best + select + subtract), the whole call, and the float64 NumPy restatement of the initial vote on one core at a
size that finishes (labelled with that size; not extrapolated).  Needs the GPU: there is no fallback.

    python scripts/measure_assoc.py [--picks 200000] [--grid 97] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import das4whales_amd as dw                                   # noqa: E402
from das4whales_amd import _lib, loc                          # noqa: E402
from das4whales_amd import _device as dev                     # noqa: E402
from tests import known_answers_assoc as ka                   # noqa: E402
from tests.known_answers_loc import C0, make_cable            # noqa: E402


def make_scene(nch, npicks, ncalls, fs, duration, xs, ys, z, seed=1):
    rng = np.random.default_rng(seed)
    cable = make_cable("line", nch)
    rows = []
    for j in range(ncalls):
        src = [rng.uniform(xs[2], xs[-3]), rng.uniform(ys[2], ys[-3]), z]
        chans = np.flatnonzero(rng.random(nch) < 0.7)
        arr = 5.0 + (duration - 35.0) * j / ncalls + np.sqrt(((cable[chans] - src) ** 2).sum(1)) / C0 + 0.004 * rng.standard_normal(len(chans))
        rows.append(np.stack([chans, np.round(arr * fs).astype(np.int64)]))
    nclutter = max(0, npicks - sum(r.shape[1] for r in rows))
    rows.append(np.stack([rng.integers(0, nch, nclutter), rng.integers(0, int(duration * fs), nclutter)]))
    return cable, ka.sort_table(np.concatenate(rows, axis=1))[0]


def timed(fn, reps, warm=3):
    """Median, min and max milliseconds of fn() over reps runs, device events around each."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=11020)
    ap.add_argument("--picks", type=int, default=200000)
    ap.add_argument("--grid", type=int, default=97)
    ap.add_argument("--dt", type=float, default=0.25)
    ap.add_argument("--max-calls", type=int, default=16)
    ap.add_argument("--min-picks", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--numpy-picks", type=int, default=4000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    fs, duration, z = 200.0, 90.0, -60.0
    xs = 42000.0 + 375.0 * (np.arange(a.grid) - a.grid // 2)
    ys = 27000.0 + 375.0 * (np.arange(a.grid) - a.grid // 2)
    cable, table = make_scene(a.channels, a.picks, a.max_calls, fs, duration, xs, ys, z)
    K, G = table.shape[1], a.grid * a.grid
    d = torch.device("cuda")
    picks_d, cable_d = torch.from_numpy(table).to(d), torch.from_numpy(cable).to(d)
    xs_d, ys_d = torch.from_numpy(xs).to(d), torch.from_numpy(ys).to(d)
    t0_range = ka.default_range(table, fs, cable, C0, xs, ys, z)
    votes, edges = loc.vote_grid(picks_d, fs, cable_d, C0, xs_d, ys_d, z, a.dt, t0_range=t0_range)
    nbins = votes.shape[2]
    res = {"channels": a.channels, "picks": K, "nodes": G, "nbins": nbins, "dt": a.dt, "max_calls": a.max_calls, "pairs": K * G}

    med, lo_, hi_ = timed(lambda: loc.vote_grid(picks_d, fs, cable_d, C0, xs_d, ys_d, z, a.dt, t0_range=t0_range), a.reps)
    res["vote_ms"] = [med, lo_, hi_]
    res["vote_pairs_per_s"] = K * G / (med * 1e-3)

    def whole():
        return loc.associate_picks(picks_d, fs, cable_d, C0, xs_d, ys_d, z, a.dt, a.min_picks, max_calls=a.max_calls, t0_range=t0_range)
    Ti, info = whole()
    res["calls_found"] = int(Ti.shape[0])
    res["npicks_per_call"] = [int(v) for v in info["npicks"].cpu()]
    med, lo_, hi_ = timed(whole, a.reps)
    res["associate_ms"] = [med, lo_, hi_]

    # one round on its own: best + select + subtract on the accumulator of the initial vote (state reset before each run)
    lib = _lib.lib
    nch = a.channels
    counts = torch.bincount(picks_d[0], minlength=nch).to(torch.int32)
    off, summ = torch.empty(nch, dtype=torch.int64, device=d), torch.empty(2, dtype=torch.int64, device=d)
    stream = dev.stream_ptr(picks_d)
    _lib.check(lib.d4w_pick_offsets_i64(dev.ptr(counts), nch, dev.ptr(off), dev.ptr(summ), stream))
    state, rec = torch.zeros(2, dtype=torch.int32, device=d), torch.zeros((1, 4), dtype=torch.int32, device=d)
    assigned = torch.zeros(K, dtype=torch.int32, device=d)
    Ti1, fg = torch.empty((1, nch), dtype=torch.float64, device=d), torch.empty((1, 4), dtype=torch.float64, device=d)
    chosen, ech = torch.empty(nch, dtype=torch.int32, device=d), torch.empty(nch, dtype=torch.float64, device=d)
    ws = torch.empty(lib.d4w_assoc_best_ws_bytes(), dtype=torch.uint8, device=d)
    acc = votes.clone()
    lo = float(t0_range[0])

    def one_round():
        _lib.check(lib.d4w_assoc_best_i32(dev.ptr(acc), a.grid, a.grid, nbins, a.min_picks, 0, dev.ptr(state), dev.ptr(rec), dev.ptr(ws), stream))
        _lib.check(lib.d4w_assoc_select_f64(dev.ptr(picks_d), K, dev.ptr(off), dev.ptr(cable_d), nch, fs, C0, dev.ptr(xs_d), a.grid, dev.ptr(ys_d),
                                            a.grid, z, lo, a.dt, nbins, 0, dev.ptr(state), dev.ptr(rec), dev.ptr(assigned), dev.ptr(Ti1),
                                            dev.ptr(chosen), dev.ptr(ech), dev.ptr(fg), stream))
        _lib.check(lib.d4w_assoc_vote_i32(dev.ptr(picks_d), K, dev.ptr(chosen), nch, -1, 1, dev.ptr(cable_d), nch, fs, C0, dev.ptr(xs_d), a.grid,
                                          dev.ptr(ys_d), a.grid, z, lo, a.dt, nbins, dev.ptr(acc), dev.ptr(state), stream))
    med, lo_, hi_ = timed(one_round, min(a.reps, a.max_calls - 3), warm=3)       # each run takes another call off the accumulator
    res["round_ms"] = [med, lo_, hi_]
    res["round_stop_flag_after"] = int(state[0].item())

    sub = table[:, np.sort(np.random.default_rng(2).choice(K, min(a.numpy_picks, K), replace=False))]
    t = time.perf_counter()
    ka.vote(sub, fs, cable, C0, xs, ys, z, a.dt, t0_range=t0_range)
    res["numpy_vote_one_core"] = {"picks": int(sub.shape[1]), "nodes": G, "seconds": time.perf_counter() - t}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
