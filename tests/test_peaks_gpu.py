"""The peak picker (das4whales_amd/csrc/peaks.hip) on hardware: device tensors passed straight to the C ABI, so that idx, counts
and cap are visible, and the pickers of the package on top.  Cases, reference (scipy.signal.find_peaks on the float64 row,
exact indices and counts, no tolerance) and the path predictors: tests/peaks_cases.py; tests/test_emu_peaks.py runs the same
table on the CPU emulator and asserts that it reaches every branch.  idx and counts are filled with a sentinel before every
call: nothing may be written past a row's count, and every row's count must be written."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import known_answers_noise as kn
from tests import peaks_cases as pc
from tests.known_answers import assert_picks_match

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Api:
    def __init__(self):
        assert torch.cuda.is_available(), "GPU tests need a ROCm device"
        import das4whales_amd as dw
        from das4whales_amd import _device as dev
        from das4whales_amd._lib import check, lib
        self.dw, self.dev, self.check, self.lib = dw, dev, check, lib


@pytest.fixture(scope="module")
def api():
    return Api()


def dev_block(x, offset=0):
    """The block on the device, its first sample `offset` floats after a 16-byte boundary (a view into a larger buffer)."""
    buf = torch.empty(x.size + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + x.size].view(x.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    assert view.data_ptr() % 16 == 4 * (offset % 4)
    return view


def launch_dev(api, xd, bar, cap=None, entry="number", scale=1.0):
    """-> (idx, counts) as device tensors.  bar: a float (number), a float32 value or an [nx] float32 array (both on the device)."""
    nx, ns = xd.shape
    cap = ns // 2 + 1 if cap is None else cap
    idx = torch.full((nx, cap), pc.SENTINEL, dtype=torch.int32, device=xd.device)
    cnt = torch.full((nx,), pc.SENTINEL, dtype=torch.int32, device=xd.device)
    p, s, lib = api.dev.ptr, api.dev.stream_ptr(xd), api.lib
    if entry == "number":
        api.check(lib.d4w_find_peaks_f32(p(xd), nx, ns, float(bar), p(idx), p(cnt), cap, s))
    else:
        val = torch.from_numpy(np.ascontiguousarray(bar, dtype=np.float32).reshape(-1)).to(xd.device)
        fn = lib.d4w_find_peaks_dthr_f32 if entry == "value" else lib.d4w_find_peaks_rowthr_f32
        api.check(fn(p(xd), nx, ns, p(val), float(scale), p(idx), p(cnt), cap, s))
    return idx, cnt


def launch(api, xd, bar, cap=None, entry="number", scale=1.0):
    idx, cnt = launch_dev(api, xd, bar, cap, entry, scale)
    return idx.cpu().numpy(), cnt.cpu().numpy()


def check_block(idx, cnt, x, row_bars, cap, where):
    for c in range(len(x)):
        pc.check_row(idx[c], cnt[c], x[c], row_bars[c], cap, (where, c))


CASES = pc.table()


@pytest.mark.parametrize("k", range(len(CASES)), ids=["%s-%d" % (c.name.replace(" ", "_"), c.ns) for c in CASES])
def test_case_table(api, k):
    """Every row of every case: equal count, equal indices, the sentinel past the count, the count written (rows that leave
    early included)."""
    case = CASES[k]
    x = pc.case_block(case)
    xd = dev_block(x, case.offset)
    for bar in pc.case_bars(case, x):
        idx, cnt = launch(api, xd, bar)
        check_block(idx, cnt, x, [bar] * len(x), case.ns // 2 + 1, (case.name, case.ns, bar))


@pytest.mark.parametrize("ns,full,distances", ((6148, True, pc.DISTANCES), (16388, False, pc.DISTANCES),
                                               (131076, False, (2, 63, 2047, 2049, None))))
def test_designed_walks(api, ns, full, distances):
    """pc.designed_rows: a dip of exactly the bar is accepted, one float32 ulp short of it rejected, at every distance, placement
    and direction, by 16 lanes per side (ballots in divergent groups) and by one lane per side."""
    for k, rows in enumerate(pc.designed_rows(ns, full, distances)):
        x = np.stack([r for r, _ in rows])
        thr = pc.WALK_BARS[k]
        idx, cnt = launch(api, dev_block(x), thr)
        for c, (r, what) in enumerate(rows):
            pc.check_row(idx[c], cnt[c], r, thr, ns // 2 + 1, what)
            if "dip=None" not in what:
                p = int(what.split("p=")[1].split()[0])
                assert (p in idx[c, :cnt[c]]) == ("exact" in what), what


@pytest.mark.parametrize("ns", (2048, 16385, 16388, 131076))                     # staged, in place (scalar, swept), 64-sample blocks
def test_nan_bar_gives_no_pick_through_every_entry_point(api, ns):
    x = pc.block(("noise", "envelope", "noise", "slow", "alternating"), ns, seed=5)
    xd = dev_block(x)
    nx = len(x)
    one = np.ones(nx, dtype=np.float32)
    for what, (idx, cnt) in (("number", launch(api, xd, NAN)),
                             ("value", launch(api, xd, np.float32(NAN), entry="value", scale=0.45)),
                             ("value x nan scale", launch(api, xd, np.float32(1.0), entry="value", scale=NAN)),
                             ("rows", launch(api, xd, one * np.float32(NAN), entry="rows"))):
        print(what, ns, cnt.tolist())
        assert np.all(cnt == 0) and np.all(idx == pc.SENTINEL), (what, cnt)
    mixed = one.copy()
    mixed[[0, 3]] = NAN
    idx, cnt = launch(api, xd, mixed, entry="rows")
    check_block(idx, cnt, x, mixed.astype(np.float64), ns // 2 + 1, "mixed rows")
    assert cnt[0] == 0 and cnt[3] == 0 and cnt[2] > 0


@pytest.mark.parametrize("ns", (2048, 20000))
def test_inf_sample_under_an_inf_bar_gives_no_pick(api, ns):
    """The known deviation: SciPy keeps a +inf sample under a +inf bar, the kernel returns none -- with few
    candidates in the row and with many."""
    x = pc.block(("pinf", "pinf_smooth", "both_inf", "pinf_at_1", "noise"), ns, seed=2)
    idx, cnt = launch(api, dev_block(x), INF)
    assert np.all(cnt == 0), cnt
    check_block(idx, cnt, x, [INF] * len(x), ns // 2 + 1, "inf")


@pytest.mark.parametrize("ns", (2048, 16388))
def test_capacity(api, ns):
    """cap equal to the count, one below it and 1: the true count is reported, the first cap indices are right and the
    neighbouring rows' slots hold what they should (every row of the launch is checked)."""
    x = pc.block(("noise", "envelope", "noise"), ns, seed=9)
    xd = dev_block(x)
    thr = 0.3 * pc.row_range(x[0])
    full = len(pc.reference(x[0], thr))
    assert full > 3
    for cap in (full, full - 1, 1):
        idx, cnt = launch(api, xd, thr, cap=cap)
        check_block(idx, cnt, x, [thr] * 3, cap, cap)
        assert cnt[0] == full


@pytest.mark.parametrize("ns", (4100, 16388))
def test_entry_points_agree_bit_for_bit(api, ns):
    """A number, scale x a device value and one bar per row give bit-equal idx and counts for the same effective bar.  The
    product is formed in float64: with pc.float64_product() the float32 product is another bar and moves the pick at 101."""
    x = pc.block(pc.FEW_KINDS, ns, seed=4)
    nx = len(x)
    scale, value, thr, thr32, dip = pc.float64_product()
    x[0, 99:104] = (9.0, dip, 8.5, -5.0, 9.0)
    assert (101 in pc.reference(x[0], thr)) != (101 in pc.reference(x[0], thr32))
    xd = dev_block(x)
    a = launch(api, xd, thr)
    b = launch(api, xd, value, entry="value", scale=scale)
    c = launch(api, xd, np.full(nx, value, dtype=np.float32), entry="rows", scale=scale)
    for got in (b, c):
        assert np.array_equal(a[0], got[0]) and np.array_equal(a[1], got[1])
    check_block(a[0], a[1], x, [thr] * nx, ns // 2 + 1, "float64 product")
    rb = pc.row_bars(x)                                                        # 0, negative, NaN, +inf, exact range, ordinary
    idx, cnt = launch(api, xd, rb, entry="rows")
    check_block(idx, cnt, x, rb.astype(np.float64), ns // 2 + 1, "mixed bars")
    for r in range(nx):                                                         # ... each row alone through the number form
        i1, c1 = launch(api, xd[r:r + 1], float(rb[r]))
        assert c1[0] == cnt[r] and np.array_equal(i1[0], idx[r]), r


def test_longest_row_and_the_next(api):
    ns = pc.longest_row()
    x = pc.block(("envelope", "noise"), ns + 1, seed=1)
    head = np.ascontiguousarray(x[:, :ns])
    thr = 0.3 * pc.row_range(head[1])
    idx, cnt = launch(api, dev_block(head), thr)
    check_block(idx, cnt, head, [thr, thr], ns // 2 + 1, ns)
    with pytest.raises(Exception, match="rows of %d samples exceed the peak-picking LDS tables" % (ns + 1)):
        launch(api, dev_block(x), thr, cap=8)


def _tiled(api, nx, ns, kinds, seeds, bar_of):
    """nx rows cycling through kinds x seeds, one bar per row (bar_of(row, c)); every row against SciPy (a reference per
    distinct (row, bar) pair, computed once), the launch repeated: bit-equal outputs."""
    distinct = [pc.row(k, ns, s) for s in range(seeds) for k in kinds]
    which = np.arange(nx) % len(distinct)
    x = np.stack(distinct)[which]
    rb = np.asarray([bar_of(x[c], c) for c in range(nx)], dtype=np.float32)
    xd = dev_block(x)
    cap = ns // 2 + 1
    first = launch(api, xd, rb, entry="rows")
    again = launch(api, xd, rb, entry="rows")
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    idx, cnt = first
    seen = {}
    for c in range(nx):
        key = (int(which[c]), rb[c].tobytes())
        if key not in seen:
            pc.check_row(idx[c], cnt[c], x[c], float(rb[c]), cap, (ns, c))
            seen[key] = c
        else:
            first_c = seen[key]
            assert cnt[c] == cnt[first_c] and np.array_equal(idx[c], idx[first_c]), (ns, c, first_c)
    return len(seen)


def test_many_workgroups_of_short_rows(api):
    """2048 rows of 2048 samples, every row kind with a bar of its own: workgroups side by side take different branches."""
    fr = (0.0, -1.0, NAN, INF, 1.0, 0.3, 0.05, 0.9, 0.45, 0.15, 0.6)       # 11 bars over 54 distinct rows
    n = _tiled(api, 2048, 2048, pc.ALL_KINDS, 2, lambda r, c: fr[c % 11] * (pc.row_range(r) if c % 11 >= 4 else 1.0))
    assert n == 594 - 2 * 7                                                    # (a constant row's range is 0: eight of its bars are 0)


def test_many_workgroups_of_full_rows(api):
    """1024 rows of 16 384 samples: two 70-KB workgroups share a CU."""
    fr = (0.3, 0.0, 0.45, 0.05, NAN, 0.9, 1.0)
    n = _tiled(api, 1024, 16384, ("noise", "envelope"), 4, lambda r, c: fr[c % 7] * pc.row_range(r))
    assert n == 56


CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
from tests import peaks_cases as pc
from tests.test_peaks_gpu import Api, check_block, dev_block, launch
api = Api()
for ns in pc.SMALL_INPLACE:
    x = pc.block(pc.ALL_KINDS, ns, seed=ns %% 89)
    xd = dev_block(x)
    for bar in pc.bars(x, "some"):
        idx, cnt = launch(api, xd, bar)
        check_block(idx, cnt, x, [bar] * len(x), ns // 2 + 1, ("in place", ns, bar))
print("in place ok", len(pc.SMALL_INPLACE))
"""


def test_small_rows_in_place():
    """D4W_FP_STAGED=0 (read once per process) sends small rows through the in-place form: one fresh child process under its
    own time limit."""
    env = dict(os.environ, D4W_FP_STAGED="0")
    out = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", CHILD % ROOT], env=env, cwd=ROOT,
                         capture_output=True, text=True)
    assert out.returncode == 0 and "in place ok %d" % len(pc.SMALL_INPLACE) in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


@pytest.mark.parametrize("nx", (1, 63, 64, 1024, 1025, 5000, 131070))
def test_pick_offsets(api, nx):
    """d4w_pick_offsets_i64: one row per thread, several, ragged last threads; counts with zeros; a total beyond 2^31."""
    rng = np.random.default_rng(nx)
    cnt = rng.integers(0, min(2 ** 31 - 1, 2 ** 36 // nx), nx).astype(np.int32)
    cnt[rng.random(nx) < 0.3] = 0
    if nx == 63:
        cnt[:] = 0
    cd = torch.from_numpy(cnt).cuda()
    off = torch.full((nx,), -1, dtype=torch.int64, device="cuda")
    summ = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    api.check(api.lib.d4w_pick_offsets_i64(api.dev.ptr(cd), nx, api.dev.ptr(off), api.dev.ptr(summ), api.dev.stream_ptr(cd)))
    ref = np.cumsum(cnt.astype(np.int64))
    assert nx < 64 or ref[-1] > 2 ** 31
    assert np.array_equal(off.cpu().numpy(), ref)
    assert summ.cpu().tolist() == [int(cnt.max()), int(ref[-1])]


@pytest.mark.parametrize("nx", (1, 4096, 4097, 9000))
def test_pack_picks(api, nx):
    """d4w_pack_picks_i64 past its 4096-workgroup grid, rows without picks among the others, against the table built from the
    reference; total == 0 with a null output."""
    ns, cap = 64, 33
    kinds = ("noise", "const", "quant2", "alternating", "all_nan", "envelope", "plateau_even")
    distinct = [pc.row(k, ns, s) for s in range(3) for k in kinds]
    which = (np.arange(nx) * 5 + 3) % len(distinct)
    x = np.stack(distinct)[which]
    refs = [pc.reference(r, 0.5) for r in distinct]
    xd = dev_block(x)
    idx, cnt = launch_dev(api, xd, 0.5, cap=cap)
    p, s = api.dev.ptr, api.dev.stream_ptr(xd)
    off = torch.empty(nx, dtype=torch.int64, device="cuda")
    summ = torch.empty(2, dtype=torch.int64, device="cuda")
    api.check(api.lib.d4w_pick_offsets_i64(p(cnt), nx, p(off), p(summ), s))
    total = int(summ.cpu()[1])
    want = np.asarray((np.concatenate([np.full(len(refs[w]), c) for c, w in enumerate(which)]),
                       np.concatenate([refs[w] for w in which])), dtype=np.int64)
    assert total == want.shape[1] and (nx == 1 or 0 in cnt.cpu().numpy())
    out = torch.full((2, total + 1), pc.SENTINEL, dtype=torch.int64, device="cuda")
    flat = out.view(-1)[:2 * total]
    api.check(api.lib.d4w_pack_picks_i64(p(idx), p(cnt), p(off), nx, cap, total, p(flat), s))
    assert np.array_equal(flat.cpu().numpy().reshape(2, total), want)
    assert out.view(-1)[2 * total:].cpu().tolist() == [pc.SENTINEL, pc.SENTINEL]
    quiet = dev_block(np.stack([pc.row("const", ns)] * min(nx, 8)))
    idx, cnt = launch_dev(api, quiet, 0.5, cap=cap)
    api.check(api.lib.d4w_pick_offsets_i64(p(cnt), len(quiet), p(off), p(summ), s))
    assert summ.cpu().tolist() == [0, 0]
    api.check(api.lib.d4w_pack_picks_i64(p(idx), p(cnt), p(off), len(quiet), cap, 0, None, s))


LAYER_KINDS = ("noise", "envelope", "all_nan", "osc", "quant2", "slow", "burst")


@pytest.mark.parametrize("ns,offset", ((2048, 0), (4099, 0), (4100, 1), (16385, 0), (16388, 0), (16388, 3), (131076, 0)))
def test_pick_times_on_every_form(api, ns, offset):
    """detect.pick_times on one block of every staged / in-place form: a number, a Threshold, one bar per channel, lazy against
    eager; a row with more than 1024 peaks (the capacity is regrown, the next call starts from the remembered one); an all-NaN
    channel among live ones gives no pick and leaves its neighbours exact."""
    dw = api.dw
    x = pc.block(LAYER_KINDS, ns, seed=3)
    nx = len(x)
    xd = dev_block(x, offset)
    span = float(np.float32(pc.row_range(x[0])))                               # a float32, so that the device forms hold it exactly
    value = torch.tensor([span], dtype=torch.float32, device="cuda")
    dw.detect._PICK_CAP.pop((nx, ns), None)
    for frac in (0.02, 0.3):
        thr = frac * span
        ref = [pc.reference(r, thr) for r in x]
        assert len(ref[2]) == 0 and (ns < 4099 or frac > 0.02 or len(ref[0]) > 1024)
        forms = (thr, dw.detect.Threshold(frac, value), dw.detect.ChannelThreshold(frac, value.repeat(nx)))
        for form in forms:
            got = dw.detect.pick_times(xd, form)
            assert len(got) == nx and all(np.array_equal(got[c], ref[c]) for c in range(nx)), (ns, frac, type(form))
            if ns >= 4099 and frac == 0.02:
                assert dw.detect._PICK_CAP[(nx, ns)] >= max(len(r) for r in ref) > 1024
        late = dw.detect.pick_times(xd, forms[1], lazy=True)
        assert late._packed is None and late == got and np.array_equal(late.table(), got.table())
    none = dw.detect.pick_times(xd, dw.detect.Threshold(0.45, torch.tensor([NAN], dtype=torch.float32, device="cuda")))
    assert none.total == 0 and all(len(r) == 0 for r in none)                   # a NaN bar: no pick, as in SciPy
    assert dw.detect.pick_times(xd, NAN).total == 0
    top = dw.detect.correlogram_max(xd, on_device=True)                        # the reference's 0.45 * np.max(corr_m) with a dead channel
    assert bool(torch.isnan(top).all()) and dw.detect.pick_times(xd, dw.detect.Threshold(0.45, top)).total == 0


@pytest.mark.parametrize("ns", (2048, 4095, 12000, 19683, 20000))
def test_pick_times_env_on_every_form(api, ns):
    """pick_times_env, process_corr and pick_times_par: SciPy on the float64 envelope with the marginal-pick rule of
    known_answers.assert_picks_match; exact against SciPy on the envelope the picker saw."""
    dw = api.dw
    x = pc.block(("osc", "burst", "all_nan", "few_full", "noise"), ns, seed=6)
    nx = len(x)
    xd = dev_block(x)
    seen = dw.dsp.envelope(xd).cpu().numpy()
    live = [c for c in range(nx) if c != 2]
    env64 = kn.envelope(x[live])
    for frac in (0.45, 0.2):
        thr = frac * float(np.nanmax(seen))
        got = dw.detect.pick_times_env(xd, thr)
        late = dw.detect.pick_times_env(xd, thr, lazy=True)
        par = dw.detect.pick_times_par(xd, thr)
        assert late == got and par == got and len(got[2]) == 0
        for k, c in enumerate(live):
            assert np.array_equal(got[c], pc.reference(seen[c], thr)), (ns, frac, c)
            assert_picks_match(got[c], env64[k], thr, "envelope picks, row %d of %d samples" % (c, ns))
        assert np.array_equal(dw.detect.process_corr(x[0], thr), pc.reference(dw.dsp.envelope(xd[0:1]).cpu().numpy()[0], thr))
