"""GPU tests of the STA/LTA detector and its trigger: the cases of tests/stalta_cases.py (which tests/test_emu_stalta.py runs on
the CPU emulator build) through the C ABI on the hardware, then the public calls -- detect.sta_lta, trigger_onset,
sta_lta_events with NumPy and CUDA-tensor containers, chained by StaLtaState -- and stream.FileStream(sta_lta=...), against the
float64 restatement of tests/known_answers_stalta.py (bound: 4 x 2^-24 relative, exact zeros, exact events)."""
import numpy as np
import pytest
import torch

from tests import known_answers_stalta as ks
from tests import stalta_cases as sc

pytestmark = pytest.mark.gpu
CONTAINERS = ("numpy", "tensor")
FORMS = {ks.CLASSIC: "classic", ks.RECURSIVE: "recursive"}


@pytest.fixture(scope="module")
def dw():
    assert torch.cuda.is_available()
    import das4whales_amd as dw
    return dw


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pitched(a, extra):
    """The array on the device inside a buffer with `extra` more columns per row (NaN there) -> a view with a row pitch."""
    buf = torch.full((a.shape[0], a.shape[1] + extra), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :a.shape[1]] = cuda(np.asarray(a, dtype=np.float32))
    return buf[:, :a.shape[1]]


def ptr(t):
    return t.data_ptr() if t is not None else None


def gpu_call(x, prev, form, nsta, nlta, gap, floor, scale, rstate, nseen, want_ratio, trig):
    from das4whales_amd._lib import lib, check
    nx, ns = x.shape
    xd = pitched(x, 3)
    pd = pitched(prev, 5) if prev is not None else None
    rd = pitched(np.full((nx, ns), np.nan, dtype=np.float32), 1) if want_ratio else None
    rin = cuda(np.asarray(rstate, dtype=np.float64)) if rstate is not None else None
    rout = torch.full((nx, 2), float("nan"), dtype=torch.float64, device="cuda")
    on = off = ain = act = ev = pk = cnt = None
    cap = 0
    if trig is not None:
        on, off, ain, cap = trig
        on, off = cuda(np.asarray(on, dtype=np.float64)), cuda(np.asarray(off, dtype=np.float64))
        ain = cuda(np.asarray(ain, dtype=np.int32)) if ain is not None else None
        ev = torch.full((nx, cap, 3), -7, dtype=torch.int32, device="cuda")
        pk = torch.full((nx, cap), float("nan"), dtype=torch.float32, device="cuda")
        cnt, act = (torch.full((nx,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    check(lib.d4w_stalta_f32(xd.data_ptr(), xd.stride(0), nx, ns, ptr(pd), pd.stride(0) if pd is not None else 0,
                             pd.shape[1] if pd is not None else 0, form, nsta, nlta, gap, floor, cuda(np.asarray(scale, dtype=np.float32)).data_ptr(),
                             ptr(rin), rout.data_ptr(), nseen, ptr(rd), rd.stride(0) if rd is not None else 0, ptr(on), ptr(off), ptr(ain),
                             ptr(act), ptr(ev), ptr(pk), ptr(cnt), cap, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    events = tuple(t.cpu().numpy() for t in (ev, pk, cnt, act)) if trig is not None else None
    return (rd.cpu().numpy() if want_ratio else None), rout.cpu().numpy(), events


def gpu_ratio(x, prev, form, nsta, nlta, gap, floor, scale, rstate, nseen):
    r, rout, _ = gpu_call(x, prev, form, nsta, nlta, gap, floor, scale, rstate, nseen, True, None)
    return r, rout


def gpu_fused(x, prev, form, nsta, nlta, gap, floor, scale, rstate, nseen, on, off, active, cap):
    return gpu_call(x, prev, form, nsta, nlta, gap, floor, scale, rstate, nseen, False, (on, off, active, cap))[2]


def gpu_trigger(r, on, off, active, cap):
    from das4whales_amd._lib import lib, check
    nx, ns = r.shape
    rd = pitched(r, 3)
    on, off = cuda(np.asarray(on, dtype=np.float64)), cuda(np.asarray(off, dtype=np.float64))
    ain = cuda(np.asarray(active, dtype=np.int32)) if active is not None else None
    ev = torch.full((nx, cap, 3), -7, dtype=torch.int32, device="cuda")
    pk = torch.full((nx, cap), float("nan"), dtype=torch.float32, device="cuda")
    cnt, act = (torch.full((nx,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    check(lib.d4w_trigger_onset_f32(rd.data_ptr(), rd.stride(0), nx, ns, on.data_ptr(), off.data_ptr(), ptr(ain), act.data_ptr(), ev.data_ptr(),
                                    pk.data_ptr(), cnt.data_ptr(), cap, torch.cuda.current_stream().cuda_stream))
    return tuple(t.cpu().numpy() for t in (ev, pk, cnt, act))


def test_constants(dw):
    from das4whales_amd._lib import lib
    assert lib.d4w_stalta_tile() == ks.TILE and lib.d4w_stalta_max_window() == ks.MAX_WINDOW >= 16384


@pytest.mark.parametrize("ns_form", list(sc.NS_FORMS))
@pytest.mark.parametrize("params", list(sc.PARAMS))
@pytest.mark.parametrize("form", (ks.CLASSIC, ks.RECURSIVE))
def test_kernel_alone(dw, form, params, ns_form):
    sc.check_kernel_alone(gpu_ratio, form, params, ns_form)


def test_dead_rows_and_gain(dw):
    sc.check_dead_and_gain(gpu_ratio)


def test_trigger_alone(dw):
    sc.check_trigger(gpu_trigger)


@pytest.mark.parametrize("form", (ks.CLASSIC, ks.RECURSIVE))
def test_scene_c_abi(dw, form):
    sc.check_scene(gpu_ratio, gpu_trigger, gpu_fused, form)


# ------------------------------------------------------------------------------------------
# the public calls
# ------------------------------------------------------------------------------------------
def args_of(form):
    a = dict(ks.CLASSIC_ARGS if form == ks.CLASSIC else ks.RECURSIVE_ARGS)
    on, off = a.pop("thr_on"), a.pop("thr_off")
    nsta, nlta = a.pop("nsta"), a.pop("nlta")
    return nsta, nlta, on, off, dict(a, form=FORMS[form])


def rows_of(events):
    return [[tuple(e) for e in rows.tolist()] for rows in events]


@pytest.mark.parametrize("container", CONTAINERS)
@pytest.mark.parametrize("form", (ks.CLASSIC, ks.RECURSIVE))
def test_public_scene(dw, form, container):
    """(a) the ratio of the whole record, (b) its events, (d) the fused call equal to (a) + (b), (e) the events as picks."""
    x, scale = ks.scene(), sc.scene_scale()
    nsta, nlta, on, off, kw = args_of(form)
    ref, events = sc.scene_reference(form)
    xin = cuda(x) if container == "tensor" else x
    r = dw.detect.sta_lta(xin, nsta, nlta, scale=scale, **kw)
    assert isinstance(r, torch.Tensor) and r.is_cuda if container == "tensor" else isinstance(r, np.ndarray) and r.dtype == np.float32
    sc.assert_close(r.cpu().numpy() if container == "tensor" else r, ref, ("public scene", form))
    ev = dw.detect.trigger_onset(r, on, off)
    assert isinstance(ev, dw.detect.EventRows) and len(ev) == ks.NX and ev.counts.tolist() == [5] * ks.NX and ev.total == 40
    assert [[e[:2] for e in rows] for rows in rows_of(ev)] == [[e[:2] for e in evs] for evs in events]
    fused = dw.detect.sta_lta_events(xin, nsta, nlta, on, off, scale=scale, **kw)
    assert torch.equal(fused.packed, ev.packed) and torch.equal(fused.packed_peak, ev.packed_peak) and torch.equal(fused.counts, ev.counts)
    # without an explicit scale: the row's own max|x| -- the same events (the floor is far away), ratios still in the bound
    sc.assert_close(dw.detect.sta_lta(cuda(x), nsta, nlta, **kw).cpu().numpy(), ref, ("public scene, own scale", form))
    table = ev.table()
    assert table.shape == (4, 40) and table.dtype == np.int64 and ev.peak.dtype == np.float32
    rn = r.cpu().numpy() if container == "tensor" else r
    assert np.array_equal(ev.peak, rn[table[0], table[3]])
    for which, col in (("peak", 3), ("on", 1)):
        picks = ev.picks(which)
        assert isinstance(picks, dw.detect.PickRows)
        assert np.array_equal(dw.detect.convert_pick_times(picks), table[[0, col]])
        assert [p.tolist() for p in picks] == [[e[col - 1] for e in rows] for rows in rows_of(ev)]
    sel = dw.detect.select_picked_times(dw.detect.convert_pick_times(ev.picks("peak")), 0.0, 30.0, ks.FS)
    assert np.array_equal(sel[1], table[3][table[3] <= 6000])


@pytest.mark.parametrize("fused", (False, True))
@pytest.mark.parametrize("form", (ks.CLASSIC, ks.RECURSIVE))
def test_public_three_files_chained_by_state(dw, form, fused):
    """(c): three calls chained by `state`, an explicit scale, give the record's ratios and events; the straddling events arrive
    as (on, 6000) + (-1, off).  The second file is a column slice of the record, read in place with its row pitch."""
    x, scale = ks.scene(), sc.scene_scale()
    nsta, nlta, on, off, kw = args_of(form)
    ref, events = sc.scene_reference(form)
    want = sc.split_at_seams(events)
    xd = cuda(x)
    state = None
    for f in range(3):
        blk = xd[:, f * ks.NFILE:(f + 1) * ks.NFILE]                  # a view: pitch 18000
        if fused:
            ev, state = dw.detect.sta_lta_events(blk, nsta, nlta, on, off, scale=scale, state=state, return_state=True, **kw)
        else:
            r, state = dw.detect.sta_lta(blk, nsta, nlta, scale=scale, state=state, return_state=True, **kw)
            sc.assert_close(r.cpu().numpy(), ref[:, f * ks.NFILE:(f + 1) * ks.NFILE], ("chained", form, f))
            ev, state = dw.detect.trigger_onset(r, on, off, state=state, return_state=True)
        assert isinstance(state, dw.detect.StaLtaState)
        assert [[e[:2] for e in rows] for rows in rows_of(ev)] == want[f], (form, f)
    with pytest.raises(ValueError):
        dw.detect.sta_lta(xd, nsta + 1, nlta, state=state, **kw)


def test_public_small_things(dw):
    """A short first block (the tail grows across calls), picks of events that were active on entry, per-channel thresholds in
    every form, the retry when a row holds more events than the first guess, and the argument errors."""
    det = dw.detect
    rng = np.random.default_rng(11)
    x = rng.standard_normal((3, 900)).astype(np.float32)
    scale = np.ones(3, dtype=np.float32)
    whole = det.sta_lta(x, 5, 64, gap=5, scale=scale)
    state, parts = None, []
    for a, b in ((0, 20), (20, 50), (50, 400), (400, 900)):
        r, state = det.sta_lta(x[:, a:b], 5, 64, gap=5, scale=scale, state=state, return_state=True)
        parts.append(r)
    # (the same windows summed from other tile origins: float64 noise under one float32 rounding)
    sc.assert_close(np.concatenate(parts, axis=1), whole, ("growing tail",))
    assert np.all(whole[:, :68] == 0) and np.any(whole[:, 68:] != 0)
    r, on, off, active = sc.trigger_rows()
    nx, ns = r.shape
    want = [ks.trigger(r[c], on[c], off[c], bool(active[c]))[0] for c in range(nx)]
    st = det.StaLtaState(None, active=cuda(active))
    for bars in ((on, off), (cuda(on.astype(np.float32)), cuda(off.astype(np.float32))),
                 (det.ChannelThreshold(2.0, cuda((on / 2).astype(np.float32))), det.ChannelThreshold(0.5, cuda((off * 2).astype(np.float32))))):
        ev, st2 = det.trigger_onset(cuda(r), bars[0], bars[1], state=st, return_state=True, _cap0=4)      # row 5 needs 2098 slots
        assert rows_of(ev) == [[w[:3] for w in rows] for rows in want]
        assert np.array_equal(ev.peak.view(np.uint32), np.array([w[3] for rows in want for w in rows], dtype=np.float32).view(np.uint32))
        assert st2.active.tolist() == [int(ks.trigger(r[c], on[c], off[c], bool(active[c]))[1]) for c in range(nx)]
    onp = ev.picks("on")
    assert [p.tolist() for p in onp] == [[w[0] for w in rows if w[0] >= 0] for rows in want]
    assert det.convert_pick_times(onp).shape == (2, sum(len([w for w in rows if w[0] >= 0]) for rows in want))
    empty = det.trigger_onset(np.full((2, 50), 2.0, dtype=np.float32), 3.0, 1.5)
    assert empty.total == 0 and empty.table().shape == (4, 0) and [len(e) for e in empty] == [0, 0] and empty.picks("peak").total == 0
    for bad in (dict(nsta=0), dict(nlta=0), dict(gap=-1), dict(nlta=ks.MAX_WINDOW, gap=1), dict(floor=-1.0), dict(floor=float("nan")),
                dict(form="other"), dict(form="recursive", gap=2), dict(scale=np.ones(2))):
        kw = dict(nsta=5, nlta=64, gap=0, floor=1e-6, form="classic", scale=None)
        kw.update(bad)
        nsta, nlta = kw.pop("nsta"), kw.pop("nlta")
        with pytest.raises(ValueError):
            det.sta_lta(x, nsta, nlta, **kw)
    with pytest.raises(ValueError):
        det.sta_lta(x[0], 5, 64)
    with pytest.raises(ValueError):
        det.trigger_onset(x, 1.0, 2.0)                         # thr_off > thr_on
    with pytest.raises(ValueError):
        det.trigger_onset(x, np.ones(2), 0.5)                  # one value per channel


def test_file_stream(dw):
    """Three 8 x 6000 files through FileStream(sta_lta=...): the events equal those of the package's own single-call path on the
    concatenation of the stream's own filtered blocks (that path is pinned by the scene tests: this one checks the halo
    bookkeeping); sta_lta=None leaves the result dicts as they are."""
    x, scale = ks.scene(), sc.scene_scale()
    opts = dict(nsta=100, nlta=2000, gap=100, thr_on=3.0, thr_off=1.5, scale=scale)
    files = [x[:, f * ks.NFILE:(f + 1) * ks.NFILE] for f in range(3)]
    runs = {}
    for name, sl in (("fused", opts), ("kept", dict(opts, keep_ratio=True)), ("off", None)):
        st = dw.stream.FileStream(fs=ks.FS, fmin=15, fmax=25, sta_lta=sl, templates=())
        res = []
        for f in files:
            res += st.push(f)
        runs[name] = res + st.flush()
        assert [r["index"] for r in runs[name]] == [0, 1, 2]
    assert all(set(r) == {"index", "filtered"} for r in runs["off"])
    assert all(set(r) == {"index", "filtered", "events"} for r in runs["fused"])
    assert all(set(r) == {"index", "filtered", "events", "sta_lta"} for r in runs["kept"])
    whole = torch.cat([r["filtered"] for r in runs["fused"]], dim=1)
    ratio = dw.detect.sta_lta(whole, 100, 2000, gap=100, scale=scale)
    ev = dw.detect.trigger_onset(ratio, 3.0, 1.5)
    assert ev.total >= 5 * ks.NX                               # the calls sit in the pass band
    want = sc.split_at_seams([[tuple(e) for e in rows.tolist()] for rows in ev])
    assert any(e[1] == ks.NFILE for evs in want[0] + want[1] for e in evs)          # something straddles a seam
    for f in range(3):
        for name in ("fused", "kept"):
            got = runs[name][f]["events"]
            assert [[e[:2] for e in rows] for rows in rows_of(got)] == want[f], (name, f)
        sc.assert_close(runs["kept"][f]["sta_lta"].cpu().numpy(), ratio[:, f * ks.NFILE:(f + 1) * ks.NFILE].cpu().numpy(), ("stream", f))
        assert torch.equal(runs["kept"][f]["events"].packed, runs["fused"][f]["events"].packed)
    with pytest.raises(ValueError):
        dw.stream.FileStream(ks.FS, 15, 25, sta_lta={"nsta": 100, "nlta": 2000, "thr_on": 3.0})
    with pytest.raises(ValueError):
        dw.stream.FileStream(ks.FS, 15, 25, sta_lta=dict(opts, window=3))
