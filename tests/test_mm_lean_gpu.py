"""The two bodies of the two-template matched filter on the GPU (csrc/xcorr_mm.hip): the cases of tests/test_emu_mm_lean.py
(tests/mm_lean_cases.py) with 600 rows on the grid of 512 workgroups, and 300 rows on a grid of 256 (D4W_MM_WGS=1, in a fresh
process: the library reads it once) -- workgroups that walk two rows and change between the lean and the general body there.

(a) rows against a float64 correlation, 2e-6 of the row's own maximum (the first and the last twelve rows of a case);
(b) the two-template launch against the two one-template launches (the general body only), bit for bit, every row."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mm_chunk_cases as cs
from tests import mm_lean_cases as lc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX = 600


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import das4whales_amd as dw_
    return dw_


def launch(dw, xd, taps, tails, with_tail, **kw):
    return dw.detect._xcorr_device(xd, taps, normalize=True, method="mm", tails=tails if with_tail else None, **kw)


@pytest.mark.parametrize("with_tail", [False, True], ids=["tail0", "tail"])
@pytest.mark.parametrize("ns", lc.NS)
def test_lean_and_general_chunks_in_one_walk(dw, ns, with_tail):
    x, _, taps, tails = lc.case(NX, ns, with_tail)
    xd = torch.from_numpy(np.array(x)).cuda()
    plain = launch(dw, xd, taps, tails, with_tail)
    rm = []
    pair = launch(dw, xd, taps, tails, with_tail, row_max=rm)
    sel = lc.checked(NX)
    for t in range(2):
        e = cs.row_err(pair[t][list(sel)].cpu().numpy(), lc.reference(NX, ns, with_tail, t, sel))
        print("ns %d %s template %d: worst row %.2e (%s)" % (ns, "tail" if with_tail else "tail0", t, e.max(), lc.kind(sel[int(e.argmax())])))
        assert e.max() < lc.TOL, (t, e)
        (single,) = launch(dw, xd, [taps[t]], [tails[t]], with_tail)
        assert torch.equal(single, pair[t]), "lean and general body: different values"
        assert torch.equal(plain[t], pair[t]) and torch.equal(rm[t], pair[t].max(dim=1).values)


def test_workgroups_that_walk_two_rows_on_a_grid_of_256():
    """300 rows, one workgroup per compute unit: rows r and r + 256 in one workgroup, an ordinary and an offset-heavy one."""
    env = dict(os.environ)
    env["D4W_MM_WGS"] = "1"
    env["PYTHONPATH"] = ROOT + os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else ROOT
    p = subprocess.run([sys.executable, "-m", "tests.mm_lean_cases", "300", "8388", "16388"], cwd=ROOT, env=env, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print("D4W_MM_WGS=1:", got)
    assert len(got) == 4
    for key, v in got.items():
        assert v["worst"] < lc.TOL and v["pair_equals_single"] and v["row_max"], (key, v)


@pytest.mark.parametrize("with_tail", [False, True], ids=["tail0", "tail"])
def test_a_row_with_a_nan_and_an_unaligned_x(dw, with_tail):
    """A NaN in an ordinary row: NaN where the one-template kernel has NaN, a NaN maximum, the other rows untouched.  x as a view
    one float past a 16-byte boundary (no chunk is lean), with the aligned call's statistics: the aligned call's values."""
    ns = 8388
    x, _, taps, tails = lc.case(NX, ns, with_tail)
    xd = torch.from_numpy(np.array(x)).cuda()
    stats = dw.detect._row_stats_cached(xd)[:2]
    base = launch(dw, xd, taps, tails, with_tail, stats=stats)
    buf = torch.zeros(NX * ns + 4, dtype=torch.float32, device="cuda")
    xu = buf[1:1 + NX * ns].view(NX, ns)
    xu.copy_(xd)
    assert xu.data_ptr() % 16 == 4
    got = launch(dw, xu, taps, tails, with_tail, stats=stats)
    assert all(torch.equal(a, b) for a, b in zip(got, base))
    assert lc.kind(3) != "heavy"
    xn = xd.clone()
    xn[3, 5000] = float("nan")
    rm = []
    ys = launch(dw, xn, taps, tails, with_tail, row_max=rm)
    keep = torch.tensor([r for r in range(NX) if r != 3], device="cuda")
    for t in range(2):
        assert bool(torch.isnan(rm[t][3])) and bool(torch.isnan(ys[t][3]).any())
        assert torch.equal(ys[t][keep], base[t][keep]) and torch.equal(rm[t][keep], base[t][keep].max(dim=1).values)
        (one,) = launch(dw, xn, [taps[t]], [tails[t]], with_tail)
        assert lc.same(one.cpu().numpy(), ys[t].cpu().numpy())


@pytest.mark.parametrize("with_tail", [False, True], ids=["tail0", "tail"])
def test_a_continuation_shorter_than_the_halo(dw, with_tail):
    """The record continues for 50 samples (clamped samples: the general body in every chunk): the pair equals the one-template
    launches bit for bit, the last lags moved, the lags of an ordinary row that read nothing of the head are the plain call's
    -- lean chunks -- bit for bit, and without the tail term the rows meet float64 of [x | head] with x's statistics."""
    ns, n_next = 8388, 50
    x, tpls, taps, tails = lc.case(NX, ns, with_tail)
    xd = torch.from_numpy(np.array(x)).cuda()
    stats = dw.detect._row_stats_cached(xd)[:2]
    rng = np.random.default_rng(ns)
    head = np.ascontiguousarray(rng.standard_normal((NX, 64)) * x.std(axis=1, keepdims=True) + x.mean(axis=1, keepdims=True), dtype=np.float32)
    hd = torch.from_numpy(head).cuda()
    base = launch(dw, xd, taps, tails, with_tail, stats=stats)
    cont = launch(dw, xd, taps, tails, with_tail, stats=stats, cont=(hd, n_next))
    plain_rows = torch.tensor([r for r in range(NX) if lc.kind(r) != "heavy"], device="cuda")
    sel = lc.checked(NX)
    for t in range(2):
        (one,) = launch(dw, xd, [taps[t]], [tails[t]], with_tail, stats=stats, cont=(hd, n_next))
        assert torch.equal(one, cont[t])
        assert not torch.equal(cont[t][:, -100:], base[t][:, -100:])
        assert torch.equal(cont[t][plain_rows, :ns - 400], base[t][plain_rows, :ns - 400])
        if not with_tail:
            ref = cs.reference(x[list(sel)], tpls[t], False, head=head[list(sel), :n_next])
            assert cs.row_err(cont[t][list(sel)].cpu().numpy(), ref).max() < lc.TOL
