"""The peak picker (das4whales_amd/csrc/peaks.hip) on the CPU emulator build, through the C ABI on host pointers: the whole case
table of tests/peaks_cases.py against scipy.signal.find_peaks, exact indices and counts, and the assertion that the table
reaches every branch it names.  tests/test_peaks_gpu.py runs the same table on hardware."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import peaks_cases as pc
from tests.emu_util import ROOT, load_emu, vp

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def emu():
    return load_emu()


def host_alloc(n):
    return np.empty(n, dtype=np.float32)


def launch(lib, x, bar, cap=None, entry="number", scale=1.0):
    """x: a [nx, ns] float32 view; bar: a float (number), a float32 value (device value) or an [nx] float32 array (rows)."""
    nx, ns = x.shape
    cap = ns // 2 + 1 if cap is None else cap
    idx = np.full((nx, cap), pc.SENTINEL, dtype=np.int32)
    cnt = np.full(nx, pc.SENTINEL, dtype=np.int32)
    if entry == "number":
        rc = lib.d4w_find_peaks_f32(vp(x), nx, ns, ctypes.c_double(bar), vp(idx), vp(cnt), cap, None)
    else:
        val = np.ascontiguousarray(bar, dtype=np.float32).reshape(-1)
        fn = lib.d4w_find_peaks_dthr_f32 if entry == "value" else lib.d4w_find_peaks_rowthr_f32
        rc = fn(vp(x), nx, ns, vp(val), ctypes.c_double(scale), vp(idx), vp(cnt), cap, None)
    assert rc == 0, lib.d4w_last_error()
    return idx, cnt


def check_block(idx, cnt, x, row_bars, cap, where):
    for c in range(len(x)):
        pc.check_row(idx[c], cnt[c], x[c], row_bars[c], cap, (where, c))


CASES = pc.table()


@functools.lru_cache(maxsize=None)
def predicted(k):
    case = CASES[k]
    x = pc.case_block(case)
    return pc.case_branches(case, x, pc.case_bars(case, x))


@pytest.mark.parametrize("k", range(len(CASES)), ids=["%s-%d" % (c.name.replace(" ", "_"), c.ns) for c in CASES])
def test_case_table(emu, k):
    case = CASES[k]
    x = pc.case_block(case)
    xv = pc.aligned(x, case.offset, host_alloc)
    for bar in pc.case_bars(case, x):
        idx, cnt = launch(emu, xv, bar)
        check_block(idx, cnt, x, [bar] * len(x), case.ns // 2 + 1, (case.name, case.ns, bar))
    assert case.want <= predicted(k), (case.name, case.ns, sorted(case.want - predicted(k)))


def test_the_table_reaches_every_branch():
    """Every case reaches the branches it names, and together they reach all of pc.BRANCHES -- no more, no fewer names."""
    seen = set()
    for k, case in enumerate(CASES):
        got = predicted(k)
        assert case.want <= got, (case.name, case.ns, sorted(case.want - got))
        seen |= got
    assert seen == set(pc.BRANCHES), (sorted(set(pc.BRANCHES) - seen), sorted(seen - set(pc.BRANCHES)))


def test_predictors_restate_the_host_decisions():
    assert [pc.bshift_of(n) for n in (1, 131072, 131073, 262144, 262145)] == [5, 5, 6, 6, 7]
    assert pc.plan(16384).staged and not pc.plan(16385).staged
    assert pc.plan(16388).sweep and not pc.plan(16388, 1).sweep and not pc.plan(16388, 1).mark4
    assert pc.plan(2048, 2).mark4 and not pc.plan(2048, 2).vec4                  # scalar staging, four-sample marking over LDS
    assert pc.plan(131076).mark4 and not pc.plan(131076).sweep and not pc.plan(131076, 3).mark4
    # the by_block list cannot overflow: staged rows have at most 512 blocks, by_block at most a quarter of them hot, 16 maxima each
    assert (pc.ROW_LDS // 32 // 4) * 16 + pc.ROW_LDS // 32 // 4 <= pc.LIST


DESIGNED = ((6148, True, pc.DISTANCES), (16388, False, pc.DISTANCES), (131076, False, (2, 63, 2047, 2049, None)))


@pytest.mark.parametrize("ns,full,distances", DESIGNED)
def test_designed_walks(emu, ns, full, distances):
    """A peak with a higher sample at every distance of pc.DISTANCES on either side, the stopper in the same block, the next
    one, the last of the super-block or a later super-block, the base dip either side of a block or super-block edge: a dip of
    exactly the bar is accepted, one float32 ulp short of it rejected -- by 16 lanes per side and by one (the crowded rows)."""
    for k, rows in enumerate(pc.designed_rows(ns, full, distances)):
        x = np.stack([r for r, _ in rows])
        thr = pc.WALK_BARS[k]
        idx, cnt = launch(emu, x, thr)
        forms = set()
        for c, (r, what) in enumerate(rows):
            pc.check_row(idx[c], cnt[c], r, thr, ns // 2 + 1, what)
            forms |= pc.branches_of(r, thr, pc.plan(ns)) & {"walk_wave", "walk_lane"}
            p = int(what.split("p=")[1].split()[0])
            if "dip=None" not in what:
                assert (p in idx[c, :cnt[c]]) == ("exact" in what), what       # the designed decision itself
        assert forms == {"walk_wave", "walk_lane"}
    lo, hi = pc.dip_values(2.1)
    assert np.float32(8.0) - np.float32(2.1) != np.float32(8.0 - 2.1) or float(np.float32(8.0) - np.float32(2.1)) != 8.0 - 2.1
    assert 8.0 - float(lo) >= 2.1 > 8.0 - float(hi)


@pytest.mark.parametrize("ns", (2048, 16385, 16388, 131076))                     # staged, in place (scalar, swept), 64-sample blocks
def test_nan_bar_gives_no_pick_through_every_entry_point(emu, ns):
    """scipy.signal.find_peaks(x, prominence=nan) returns no peak, whatever the row: noise rows (thousands of candidates: a lane
    per side) and smooth rows (a few: 16 lanes per side) alike."""
    x = pc.block(("noise", "envelope", "noise", "slow", "alternating"), ns, seed=5)
    nx = len(x)
    for r in x:
        assert len(pc.reference(r, NAN)) == 0
    one = np.ones(nx, dtype=np.float32)
    for what, (idx, cnt) in (("number", launch(emu, x, NAN)),
                             ("value", launch(emu, x, np.float32(NAN), entry="value", scale=0.45)),
                             ("value x nan scale", launch(emu, x, np.float32(1.0), entry="value", scale=NAN)),
                             ("rows", launch(emu, x, one * np.float32(NAN), entry="rows"))):
        print(what, ns, cnt.tolist())
        assert np.all(cnt == 0) and np.all(idx == pc.SENTINEL), (what, cnt)
    mixed = one.copy()
    mixed[[0, 3]] = NAN
    idx, cnt = launch(emu, x, mixed, entry="rows")
    check_block(idx, cnt, x, mixed.astype(np.float64), ns // 2 + 1, "mixed rows")
    assert cnt[0] == 0 and cnt[3] == 0 and cnt[2] > 0


@pytest.mark.parametrize("ns", (2048, 20000))
def test_inf_sample_under_an_inf_bar_gives_no_pick(emu, ns):
    """The known deviation: SciPy keeps a +inf sample under a +inf bar (inf - finite >= inf), the kernel returns
    none -- in a row with few candidates and in one with many."""
    x = pc.block(("pinf", "pinf_smooth", "both_inf", "pinf_at_1", "noise"), ns, seed=2)
    assert len(pc.reference(x[0], INF)) == 1 and len(pc.reference(x[1], INF)) == 1
    idx, cnt = launch(emu, x, INF)
    assert np.all(cnt == 0), cnt
    check_block(idx, cnt, x, [INF] * len(x), ns // 2 + 1, "inf")


def test_capacity(emu):
    x = pc.block(("noise", "envelope", "noise"), 2048, seed=9)
    thr = 0.3 * pc.row_range(x[0])
    full = len(pc.reference(x[0], thr))
    assert full > 3
    for cap in (full, full - 1, 1):
        idx, cnt = launch(emu, x, thr, cap=cap)
        check_block(idx, cnt, x, [thr] * 3, cap, cap)
        assert cnt[0] == full and cnt[2] > cap - 1


def test_entry_points_agree_bit_for_bit(emu):
    """A number, scale x a device value and one bar per row give the same idx and counts for the same effective bar; the
    product is formed in float64: with scale and value below, the float32 product is another bar and moves a pick."""
    ns = 4100
    x = pc.block(pc.FEW_KINDS, ns, seed=4)
    nx = len(x)
    scale, value, thr, thr32, dip = pc.float64_product()
    x[0, 99:104] = (9.0, dip, 8.5, -5.0, 9.0)                                  # prominence 8.5 - dip: between the two products
    assert (101 in pc.reference(x[0], thr)) != (101 in pc.reference(x[0], thr32))
    a = launch(emu, x, thr)
    b = launch(emu, x, value, entry="value", scale=scale)
    c = launch(emu, x, np.full(nx, value, dtype=np.float32), entry="rows", scale=scale)
    for got in (b, c):
        assert np.array_equal(a[0], got[0]) and np.array_equal(a[1], got[1])
    check_block(a[0], a[1], x, [thr] * nx, ns // 2 + 1, "float64 product")
    rb = pc.row_bars(x)
    idx, cnt = launch(emu, x, rb, entry="rows", scale=1.0)
    check_block(idx, cnt, x, rb.astype(np.float64), ns // 2 + 1, "mixed bars")
    for c_ in range(nx):                                                        # ... and row by row through the number form
        i1, c1 = launch(emu, x[c_:c_ + 1], float(rb[c_]))
        assert c1[0] == cnt[c_] and np.array_equal(i1[0], idx[c_]), c_


def test_longest_row_and_the_next(emu):
    ns = pc.longest_row()
    assert pc.lds_bytes(ns) <= pc.LDS_MAX < pc.lds_bytes(ns + 1) and pc.bshift_of(ns) == 7
    x = pc.block(("envelope", "noise"), ns + 1, seed=1)
    head = np.ascontiguousarray(x[:, :ns])
    thr = 0.3 * pc.row_range(head[1])
    idx, cnt = launch(emu, head, thr)
    check_block(idx, cnt, head, [thr, thr], ns // 2 + 1, ns)
    i2 = np.full((2, 8), pc.SENTINEL, dtype=np.int32)
    c2 = np.full(2, pc.SENTINEL, dtype=np.int32)
    assert emu.d4w_find_peaks_f32(vp(x), 2, ns + 1, ctypes.c_double(thr), vp(i2), vp(c2), 8, None) == -1
    assert b"exceed the peak-picking LDS tables" in emu.d4w_last_error() and str(ns + 1).encode() in emu.d4w_last_error()
    assert np.all(i2 == pc.SENTINEL) and np.all(c2 == pc.SENTINEL)


CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
from tests import peaks_cases as pc
from tests.test_emu_peaks import check_block, launch
from tests.emu_util import load_emu
emu = load_emu()
for ns in pc.SMALL_INPLACE:
    x = pc.block(pc.ALL_KINDS, ns, seed=ns %% 89)
    for bar in pc.bars(x, "some"):
        idx, cnt = launch(emu, x, bar)
        check_block(idx, cnt, x, [bar] * len(x), ns // 2 + 1, ("in place", ns, bar))
print("in place ok", len(pc.SMALL_INPLACE))
"""


def test_small_rows_in_place():
    """D4W_FP_STAGED=0 (read once per process: one child) sends rows of every small length through the in-place form."""
    env = dict(os.environ, D4W_FP_STAGED="0")
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "in place ok %d" % len(pc.SMALL_INPLACE) in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
