"""Timing of the delay-and-sum stack (csrc/stack.hip) with device events, one process, warm: median (min-max) of --reps runs.

Shape: the synthetic 11 020-channel "line" cable, 12 000 samples at 200 Hz, all channels and every 4th; 33 x 33 nodes at
1125 m and 97 x 97 nodes at 375 m (the same 36 km square).  Timed: the delay table, the stack in its window and its direct
form through the C ABI, loc.stack_grid (the public call, which chooses), loc.stack_best, loc.arrivals_near for 16 calls and
the composed loc.locate_stack; and the float64 NumPy restatement of the stack on one core at a size that finishes (labelled
with that size; not extrapolated).  Rates are (node, channel, column) triples per second, set against the chip's ds_read_b32
word rate (256 CUs x 32 words/clk) and its fma rate (256 CUs x 128 /clk) at the nominal 2.4 GHz: fractions of a nominal
peak, not of a measured one.  Needs the GPU: there is no fallback.

    python scripts/measure_stack.py [--reps 20] [--out profiles/stack/measure_stack.json]
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
import das4whales_amd as dw                                   # noqa: E402,F401
from das4whales_amd import loc                                # noqa: E402
from tests import known_answers_stack as ks                   # noqa: E402
from tests.known_answers_loc import C0, make_cable            # noqa: E402

LDS_WORDS_PER_S = 256 * 32 * 2.4e9
FMA_PER_S = 256 * 128 * 2.4e9


def timed(fn, reps, warm=2):
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
    return [float(np.median(ms)), float(np.min(ms)), float(np.max(ms))]


def rates(triples, ms):
    r = triples / (ms[0] * 1e-3)
    return {"ms": ms, "triples_per_s": r, "of_lds_read_rate": r / LDS_WORDS_PER_S, "of_fma_rate": r / FMA_PER_S}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=11020)
    ap.add_argument("--samples", type=int, default=12000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--numpy-size", type=int, nargs=3, default=[9, 400, 3000], metavar=("GRID", "CHANNELS", "SAMPLES"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    fs, z = 200.0, -60.0
    d = torch.device("cuda")
    rng = np.random.default_rng(1)
    cable_all = make_cable("line", a.channels)
    env_all = torch.from_numpy(np.abs(rng.standard_normal((a.channels, a.samples))).astype(np.float32)).to(d)
    res = {"samples": a.samples, "fs": fs, "reps": a.reps, "runs": []}
    for step in (4, 1):
        cable = torch.from_numpy(np.ascontiguousarray(cable_all[::step])).to(d)
        env = env_all[::step].contiguous()
        nch = cable.shape[0]
        for n, spacing in ((33, 1125.0), (97, 375.0)):
            xs = torch.from_numpy(42000.0 + spacing * (np.arange(n) - n // 2)).to(d)
            ys = torch.from_numpy(27000.0 + spacing * (np.arange(n) - n // 2)).to(d)
            triples = n * n * nch * a.samples
            run = {"channels": nch, "nodes": n * n, "spacing_m": spacing, "triples": triples}
            run["delay_table_ms"] = timed(lambda: loc.delay_table(cable, C0, fs, xs, ys, z), a.reps)
            table = loc.delay_table(cable, C0, fs, xs, ys, z)
            stack, info = loc._stack(env, env.shape[1], table, None, n, n, 0, a.samples, False, form=0)
            run["chosen_form"], run["tile_spread"] = (int(v) for v in info.cpu())
            for name, form in (("window", 1), ("direct", 2)):
                ms = timed(lambda: loc._stack(env, env.shape[1], table, None, n, n, 0, a.samples, False, form=form), a.reps, warm=1)
                run[name] = rates(triples, ms)
            run["window_normalize"] = rates(triples, timed(
                lambda: loc._stack(env, env.shape[1], table, None, n, n, 0, a.samples, True, form=1), a.reps, warm=1))
            run["stack_grid"] = rates(triples, timed(lambda: loc.stack_grid(env, fs, cable, C0, xs, ys, z, delays=table), a.reps, warm=1))
            run["stack_best_ms"] = timed(lambda: loc.stack_best(stack), a.reps)
            peak, node = loc.stack_best(stack)
            cols = torch.linspace(500, a.samples - 3000, 16, device=d).long()
            g = node[cols].long()
            pos = torch.stack([xs[g % n], ys[g // n], torch.full((16,), z, dtype=torch.float64, device=d)], dim=1)
            t0 = cols.double() / fs
            run["arrivals_near_16_calls_ms"] = timed(lambda: loc.arrivals_near(env, fs, cable, C0, pos, t0, 20, 0.0), a.reps)
            # prominence 0: every local maximum of the trace of best values is a candidate, the 16 largest become calls
            Ti, _ = loc.locate_stack(env, fs, cable, C0, xs, ys, z, 0.0, 20, 0.0, max_calls=16)
            run["locate_stack_calls"] = int(Ti.shape[0])
            run["locate_stack"] = rates(triples, timed(lambda: loc.locate_stack(env, fs, cable, C0, xs, ys, z, 0.0, 20, 0.0, max_calls=16),
                                                       a.reps, warm=1))
            del stack
            print(json.dumps(run), flush=True)
            res["runs"].append(run)
    # the float64 NumPy restatement of the stack, one core, at a size that finishes
    g, nch, ns = a.numpy_size
    xs, ys = 42000.0 + 1500.0 * (np.arange(g) - g // 2), 27000.0 + 1500.0 * (np.arange(g) - g // 2)
    cable = make_cable("line", nch)
    env = np.abs(rng.standard_normal((nch, ns))).astype(np.float32)
    table, _ = ks.delay_table(cable, C0, 50.0, xs, ys, z)
    t = time.perf_counter()
    ks.stack_grid(env, table)
    res["numpy_stack_one_core"] = {"nodes": g * g, "channels": nch, "samples": ns, "triples": g * g * nch * ns,
                                   "seconds": time.perf_counter() - t}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
