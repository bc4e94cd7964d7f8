"""bench.py's plain run, --full and --dump-outputs: the plain line carries the headline fields only, --full adds the side
measurements, and the dumped arrays are what the timed step's public calls return on the bench's seeded input."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_dump_outputs_sample_is_fixed_and_within_budget(tmp_path, monkeypatch):
    """An output larger than its share of the budget is written as seeded whole rows + seeded single elements, the same
    in every run; a small one is written whole."""
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 3 * 2 ** 20)
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn((3000, 1200), generator=g), torch.randn((3000, 1200), generator=g)
    w1 = bench.dump_outputs(str(tmp_path / "one"), {"corr_hf": a, "corr_lf": b})
    w2 = bench.dump_outputs(str(tmp_path / "two"), {"corr_hf": a, "corr_lf": b})
    assert w1 == w2 and "corr_hf_rows" in w1 and "corr_lf_points" in w1
    files = sorted(os.listdir(tmp_path / "one"))
    assert files == sorted(os.listdir(tmp_path / "two")) == sorted(k + ".npy" for k in w1)
    assert sum(os.path.getsize(tmp_path / "one" / f) for f in files) <= bench.DUMP_BUDGET
    for f in files:
        x, y = np.load(tmp_path / "one" / f), np.load(tmp_path / "two" / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), f
    rows = np.load(tmp_path / "one" / "corr_hf_row_index.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "one" / "corr_hf_rows.npy"), a.numpy()[rows])
    pts = np.load(tmp_path / "one" / "corr_lf_point_index.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "one" / "corr_lf_points.npy"), b.numpy().reshape(-1)[pts])
    small = torch.randn((40, 480), generator=g, dtype=torch.float64)
    assert bench.dump_outputs(str(tmp_path / "small"), {"filtered": small}) == {"filtered": [40, 480]}
    assert np.array_equal(np.load(tmp_path / "small" / "filtered.npy"), small.numpy())


@pytest.mark.gpu
def test_plain_run_full_run_and_dumped_outputs(tmp_path):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    nx, ns = 96, 480
    out = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--nx", str(nx), "--ns", str(ns),
                  "--dump-outputs", str(tmp_path / "dump")])
    assert all(k in out for k in HEADLINE) and out["steps"] == 3 and out["ms_per_step"] > 0
    assert out["higher_is_better"] is True and abs(out["value"] - nx * ns / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    assert "roofline" not in out and "cpu_baseline" not in out
    assert out["outputs"]["arrays"] == {"corr_hf": [nx, ns], "corr_lf": [nx, ns]}
    full = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--nx", str(nx), "--ns", str(ns), "--full", "--no-cpu"])
    assert all(k in full for k in HEADLINE) and full["steps"] == 2
    assert full["roofline"]["kernel_ms"] and "fk_classic" in full["roofline"]
    assert "ms_per_step_private_composition" in full["config"]
    # the same public calls on the bench's seeded input
    import das4whales_amd as dw
    fs, dx = 200.0, 2.0419046878814697
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(1234)
    x = torch.randn((nx, ns), dtype=torch.float32, device="cuda:0", generator=gen)
    t = np.arange(ns) / fs
    tpl = [dw.detect.gen_template_fincall(t, fs, 17.8, 28.8, 0.68), dw.detect.gen_template_fincall(t, fs, 14.7, 21.8, 0.78)]
    y = dw.dsp.fk_filter_filt(x, dw.dsp.fk_filter_design((nx, ns), [0, nx, 1], dx, fs))
    for name, c in zip(("corr_hf", "corr_lf"), dw.detect.compute_cross_correlograms(y, tpl)):
        d = np.load(tmp_path / "dump" / (name + ".npy"))
        ref = c.cpu().numpy()
        assert d.dtype == np.float32 and d.shape == (nx, ns)
        assert np.max(np.abs(d - ref)) <= 1e-5 * np.max(np.abs(ref)), name
