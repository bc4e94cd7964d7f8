"""Time the five image operators of csrc/edges.hip on a resident CUDA tensor: HIP events around each public call,
warm-ups first, median (and spread) of --reps calls, at the binned file image 1102 x 1200 and the file image
11020 x 12000.  Beside each, the algorithmic bytes (one read and one write of the image, 8 B/pixel) as TB/s and, for the
bilateral filter, taps/s.  Where the reference's CPU form exists here (NumPy slices, SciPy fftconvolve, CPU-torch conv2d)
it is timed on one thread on the same host (--cpu; once at the file shape, three times at the binned one).  There is no
CPU baseline for gaussian_filter and bilateral_filter: the reference calls cv2, which is not installed.  Prints one JSON
line; --out also writes it to a file.

    python scripts/time_edges.py [--reps 30] [--cpu] [--out profiles/<dir>/time_edges.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import das4whales_amd as dw  # noqa: E402

ip = dw.improcess


def _circle_taps(d):
    r = d // 2
    i = np.arange(-r, r + 1)
    return int(np.count_nonzero(i[:, None] ** 2 + i[None, :] ** 2 <= r * r))


CALLS = [
    ("gradient_oriented (1, 0)", lambda x: ip.gradient_oriented(x, (1, 0)), 0),
    ("gradient_oriented (2, 3)", lambda x: ip.gradient_oriented(x, (2, 3)), 0),
    ("detect_diagonal_edges", lambda x: ip.detect_diagonal_edges(x, 0.0), 0),
    ("diagonal_edge_detection", lambda x: ip.diagonal_edge_detection(x, 0.0), 0),
    ("gaussian_filter size 9", lambda x: ip.gaussian_filter(x, 9, 2.0), 0),
    ("gaussian_filter size 31", lambda x: ip.gaussian_filter(x, 31, 4.5), 0),
    ("bilateral_filter d 5", lambda x: ip.bilateral_filter(x, 5, 30.0, 30.0), _circle_taps(5)),
    ("bilateral_filter d 9", lambda x: ip.bilateral_filter(x, 9, 30.0, 30.0), _circle_taps(9)),
]


def cpu_forms():
    """The reference's own arithmetic for the three functions that need only NumPy, SciPy and CPU torch."""
    import scipy.signal as sp
    import torch.nn.functional as F
    d = np.array([[0, 1, 1, 1, 1], [-1, 0, 1, 1, 1], [-1, -1, 0, 1, 1], [-1, -1, -1, 0, 1], [-1, -1, -1, -1, 0]])
    wl = torch.tensor([[2, -1, -1], [-1, 2, -1], [-1, -1, 2]], dtype=torch.float32)
    wr = torch.flip(wl, [0])

    def ded(a):
        t = torch.tensor(a, dtype=torch.float32).unsqueeze(0)
        return F.conv2d(t, wl[None, None], padding=1) + F.conv2d(t, wr[None, None], padding=1)

    return {"gradient_oriented (1, 0)": lambda a: -(a[:, :-1] - a[:, 1:]),
            "gradient_oriented (2, 3)": lambda a: -(a[3:-3, :-2] - 0.5 * a[6:, 2:] - 0.5 * a[:-6, 2:]),
            "detect_diagonal_edges": lambda a: sp.fftconvolve(a, d, mode="same") + sp.fftconvolve(a, np.fliplr(d), mode="same"),
            "diagonal_edge_detection": ded}


def time_shape(h, w, reps, warmup, cpu):
    g = torch.Generator(device="cuda").manual_seed(h * w)
    x = torch.rand((h, w), device="cuda", generator=g) * 255.0
    host = x.cpu().numpy().astype(np.float64) if cpu else None
    forms = cpu_forms() if cpu else {}
    runs = []
    for name, fn, taps in CALLS:
        for _ in range(warmup):
            fn(x)
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            y = fn(x)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        med = float(np.median(ms))
        run = {"call": name, "shape": [h, w], "reps": reps, "ms_median": med, "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)),
               "algorithmic_TB_per_s": 8.0 * h * w / (med * 1e-3) / 1e12, "checksum": float(y.double().sum())}
        if taps:
            run["taps_per_pixel"] = taps
            run["taps_per_s"] = float(taps) * h * w / (med * 1e-3)
        if name in forms:
            n = 1 if h * w > (1 << 24) else 3
            ts = []
            for _ in range(n):
                t0 = time.perf_counter()
                forms[name](host)
                ts.append(time.perf_counter() - t0)
            run["cpu_one_thread_ms"] = float(np.median(ts)) * 1e3
            run["cpu_runs"] = n
        elif cpu:
            run["cpu_one_thread_ms"] = None          # cv2 is not installed: no CPU baseline exists for this call
        del y
        runs.append(run)
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    if args.cpu:
        torch.set_num_threads(1)
    res = {"kernels": "csrc/edges.hip: stencil_zero_tile, gradient_oriented, gauss_tile, bilateral_tile", "device": torch.cuda.get_device_name(0),
           "cpu_baseline": "one thread, same host; none for gaussian_filter / bilateral_filter (the reference calls cv2, not installed)",
           "runs": time_shape(1102, 1200, args.reps, args.warmup, args.cpu) + time_shape(11020, 12000, args.reps, args.warmup, args.cpu)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
