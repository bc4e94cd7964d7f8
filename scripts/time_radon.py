"""Time improcess.compute_radon_transform on a resident CUDA tensor: HIP events around each public call, warm-ups first,
median (and spread) of --reps calls.  Shapes: the binned file image 1102 x 1200 and the fixture's binned image 24 x 160,
180 angles each.  Prints one JSON line; --out also writes it to a file.

    python scripts/time_radon.py [--reps 30] [--out profiles/<dir>/time_radon.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import das4whales_amd as dw  # noqa: E402

CPU_S_1102x1200 = 16.9      # skimage.transform.radon, float64, one CPU core, 1102 x 1200 x 180 angles (issue figure)


def time_shape(h, w, ntheta, reps, warmup):
    g = torch.Generator(device="cuda").manual_seed(h * w)
    x = torch.rand((h, w), device="cuda", generator=g) * 255.0
    theta = np.arange(ntheta, dtype=np.float64) * (180.0 / ntheta)
    for _ in range(warmup):
        dw.improcess.compute_radon_transform(x, theta)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        y = dw.improcess.compute_radon_transform(x, theta)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    P = int(y.shape[0])
    med = float(np.median(ms))
    samples = float(P) * P * ntheta                     # bilinear samples of the reference's P x P warp per angle
    return {"shape": [h, w], "ntheta": ntheta, "P": P, "reps": reps, "ms_median": med, "ms_min": float(np.min(ms)),
            "ms_max": float(np.max(ms)), "samples_per_s": samples / (med * 1e-3),
            "checksum": float(y.double().sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    res = {"kernel": "radon_rays (one thread per ray and angle, float64 sample points)", "device": torch.cuda.get_device_name(0),
           "runs": [time_shape(1102, 1200, 180, args.reps, args.warmup), time_shape(24, 160, 180, args.reps, args.warmup)]}
    res["speedup_vs_cpu_1102x1200"] = CPU_S_1102x1200 * 1e3 / res["runs"][0]["ms_median"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
