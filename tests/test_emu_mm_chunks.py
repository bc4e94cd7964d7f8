"""The matched filter's chunk walk on the CPU emulator (csrc/xcorr_mm.hip): the two-template kernel takes 8192 lags per
chunk, the one-template kernels 4096, both in groups of 4096 lags with a scale, an LDS stage and a prefix carry of their own;
the chunks are walked as (row, chunk in row) without divisions, whole rows per workgroup where the template's tail is added.
Against a float64 correlation at the bounds of tests/test_emu_rowops.py (2e-6 of every row's own maximum), and the
two-template launch against the two one-template launches bit for bit: a lag's arithmetic does not depend on the chunk length."""
import ctypes

import numpy as np
import pytest

from tests import mm_chunk_cases as cs
from tests.emu_util import load_emu, vp

TOL = 2e-6          # tests/test_emu_rowops.py: the matrix-core emulator tests' bound, white rows and the template-tail test alike
# the emulator reports 2 compute units: the two-template kernel runs on 4 workgroups, the 6-step one-template kernel on 6.
# Row counts below, at and above both grids: fewer rows than workgroups, and a last round that is not full.
CASES = [(1, 4095), (3, 4096), (5, 4100), (7, 8191), (3, 8192), (5, 8193), (7, 12000), (1, 16385), (5, 16385)]


@pytest.fixture(scope="module")
def emu():
    return load_emu()


def run(lib, x, taps, tails, stats=True, want_max=False, nxt=None, n_next=0, misalign=0):
    """d4w_xcorr_mm_tail_f32 on host arrays.  misalign: x and the outputs start that many floats past a 16-byte boundary."""
    nx, ns = x.shape

    def placed(a):
        buf = np.zeros(a.size + 8, dtype=np.float32)
        off = (-(buf.ctypes.data // 4) % 4 + misalign) % 4 if misalign else 0
        v = buf[off:off + a.size].reshape(a.shape)
        v[...] = a
        assert misalign == 0 or v.ctypes.data % 16 == 4 * misalign
        return v
    xf = placed(np.ascontiguousarray(x, dtype=np.float32))
    lt = max(4, -(-max(len(t) for t in taps) // 4) * 4)
    tp = np.zeros((len(taps), lt), dtype=np.float32)
    for i, t in enumerate(taps):
        tp[i, :len(t)] = t
    mean, mx = np.empty(nx, dtype=np.float64), np.empty(nx, dtype=np.float32)
    if stats:
        assert lib.d4w_row_stats_f32(vp(xf), nx, ns, vp(mean), vp(mx), None) == 0
    ys = [placed(np.full((nx, ns), np.nan, np.float32)) for _ in taps]
    rm = [np.full(nx, np.nan, np.float32) for _ in taps] if want_max else None
    two = len(taps) > 1
    rc = lib.d4w_xcorr_mm_tail_f32(vp(xf), nx, ns, vp(nxt) if nxt is not None else None, nxt.shape[1] if nxt is not None else 0,
                                   n_next, vp(mean) if stats else None, vp(mx) if stats else None, vp(tp), len(taps), lt,
                                   len(taps[0]), len(taps[-1]), ctypes.c_double(tails[0]), ctypes.c_double(tails[-1] if two else 0.0),
                                   vp(ys[0]), vp(ys[1]) if two else None, vp(rm[0]) if want_max else None,
                                   vp(rm[1]) if want_max and two else None, None)
    assert rc == 0, lib.d4w_last_error()
    return (ys, rm) if want_max else ys


@pytest.mark.parametrize("with_tail", [False, True], ids=["tail0", "tail"])
@pytest.mark.parametrize("nx,ns", CASES)
def test_pair_and_single_kernels_against_float64(emu, nx, ns, with_tail):
    """Every row length around one and two groups and every row count around the grids; white, drifting, stepped and
    offset-heavy rows; tail coefficients exactly zero (chunks dealt over the grid) and clearly non-zero (whole rows)."""
    idx = CASES.index((nx, ns))
    sup = cs.SUPPORTS[idx % 2]
    x = cs.rows(nx, ns, seed=1000 + idx, first_kind=idx)
    tpls = [cs.template(ns, sup[t], zero_mean=not with_tail, seed=7 * idx + t) for t in range(2)]
    tt = [cs.taps_and_tail(tp, with_tail) for tp in tpls]
    taps, tails = [a for a, _ in tt], [b for _, b in tt]
    if with_tail:
        assert min(abs(c) for c in tails) > 1e-3
    pair = run(emu, x, taps, tails)
    for t in range(2):
        ref = cs.reference(x, tpls[t], with_tail)
        e = cs.row_err(pair[t], ref)
        print("nx %d ns %d %s template %d: worst row %.2e (%s)" % (nx, ns, "tail" if with_tail else "tail0", t, e.max(), cs.kinds(nx, idx)))
        assert e.max() < TOL, (t, e, cs.kinds(nx, idx))
        (single,) = run(emu, x, [taps[t]], [tails[t]])
        assert cs.row_err(single, ref).max() < TOL
        assert np.array_equal(single, pair[t]), "8192-lag and 4096-lag chunks: different values"


@pytest.mark.parametrize("ns", [4100, 8193, 12000])
def test_rows_without_statistics_scale_every_group_alone(emu, ns):
    """No statistics from the caller: every group of 4096 lags takes its own power of two, whatever the chunk length -- rows
    whose level changes a thousandfold inside a chunk, against float64 and against the one-template kernels bit for bit."""
    rng = np.random.default_rng(ns)
    nx = 5
    x = rng.standard_normal((nx, ns)) * np.where(np.arange(ns) < 4500, 1.0, 1e-3)[None, :] * 37.0
    x = np.ascontiguousarray(x, dtype=np.float32)
    t0, t1 = rng.standard_normal(163), rng.standard_normal(150) * 0.01
    y0, y1 = run(emu, x, [t0, t1], [0.0, 0.0], stats=False)
    for y, t in ((y0, t0), (y1, t1)):
        ref = np.stack([cs.orc.shift_xcorr(r.astype(np.float64), np.pad(t, (0, ns - len(t)))) for r in x])
        assert cs.row_err(y, ref).max() < TOL
        (z,) = run(emu, x, [t], [0.0], stats=False)
        assert np.array_equal(z, y)


@pytest.mark.parametrize("with_tail", [False, True], ids=["tail0", "tail"])
def test_unaligned_rows_and_a_short_continuation(emu, with_tail):
    """Rows that start 4 and 12 bytes past a 16-byte boundary with an odd length (scalar loads and stores in every chunk), and a
    record that continues in xnext for fewer samples than the halo: the same numbers as the aligned call / as correlating
    [x | head] with x's own statistics, and float64."""
    nx, ns, n_next = 5, 8193 + 4096, 50
    x = cs.rows(nx, ns, seed=77, first_kind=1)
    tpls = [cs.template(ns, s, zero_mean=not with_tail, seed=s) for s in (136, 156)]
    tt = [cs.taps_and_tail(tp, with_tail) for tp in tpls]
    taps, tails = [a for a, _ in tt], [b for _, b in tt]
    base = run(emu, x, taps, tails)
    for mis in (1, 3):
        got = run(emu, x, taps, tails, misalign=mis)
        assert all(np.array_equal(a, b) for a, b in zip(got, base))
    for t in range(2):
        assert cs.row_err(base[t], cs.reference(x, tpls[t], with_tail)).max() < TOL
    rng = np.random.default_rng(5)
    head = np.ascontiguousarray(rng.standard_normal((nx, 64)) * x.std(axis=1, keepdims=True) + x.mean(axis=1, keepdims=True), dtype=np.float32)
    cont = run(emu, x, taps, tails, nxt=head, n_next=n_next)
    mean, mx = np.empty(nx, dtype=np.float64), np.empty(nx, dtype=np.float32)
    assert emu.d4w_row_stats_f32(vp(x), nx, ns, vp(mean), vp(mx), None) == 0
    for t in range(2):
        if not with_tail:
            assert cs.row_err(cont[t], cs.reference(x, tpls[t], False, head=head[:, :n_next])).max() < TOL
        (one,) = run(emu, x, [taps[t]], [tails[t]], nxt=head, n_next=n_next)
        assert np.array_equal(one, cont[t])
        assert not np.array_equal(cont[t][:, -100:], base[t][:, -100:])        # the continuation did enter the last lags


@pytest.mark.parametrize("with_tail", [False, True], ids=["tail0", "tail"])
def test_row_maxima_and_a_row_with_nan(emu, with_tail):
    """The instantiation that leaves the rows' maxima: the maximum of what was stored, NaN for the row that holds a NaN
    (np.max), over chunks of 8192 lags (one atomic per wave and chunk)."""
    nx, ns = 5, 12000
    x = cs.rows(nx, ns, seed=99)
    tpls = [cs.template(ns, s, zero_mean=not with_tail, seed=s) for s in (136, 156)]
    tt = [cs.taps_and_tail(tp, with_tail) for tp in tpls]
    taps, tails = [a for a, _ in tt], [b for _, b in tt]
    plain = run(emu, x, taps, tails)
    ys, rm = run(emu, x, taps, tails, want_max=True)
    for t in range(2):
        assert np.array_equal(ys[t], plain[t])
        assert np.array_equal(rm[t], ys[t].max(axis=1))
    x[2, 9000] = np.nan
    ys, rm = run(emu, x, taps, tails, want_max=True)
    for t in range(2):
        assert np.isnan(rm[t][2]) and np.isnan(ys[t][2]).any()
        keep = [0, 1, 3, 4]
        assert np.array_equal(rm[t][keep], plain[t][keep].max(axis=1)) and np.array_equal(ys[t][keep], plain[t][keep])


@pytest.mark.parametrize("support", [150, 200, 330, 450])
def test_one_template_kernels_of_every_depth_with_tail_and_row_maxima(emu, support):
    """One template of 6, 7, 11 and 15 k-steps -- the 6-, 8-, 12- and 16-step kernels -- without and with the tail, without and
    with the row maxima (the 6-step kernel with both is an instantiation of its own): float64, the same values whether or not
    the maxima are formed, and the maxima of what was stored.  One sample into a third chunk of 4096 lags."""
    nx, ns = 5, 8193
    x = cs.rows(nx, ns, seed=300 + support)
    for with_tail in (False, True):
        tpl = cs.template(ns, support, zero_mean=not with_tail, seed=support)
        taps, tail = cs.taps_and_tail(tpl, with_tail)
        (plain,) = run(emu, x, [taps], [tail])
        e = cs.row_err(plain, cs.reference(x, tpl, with_tail))
        print("support %d %s: worst row %.2e" % (support, "tail" if with_tail else "tail0", e.max()))
        assert e.max() < TOL, e
        ys, rm = run(emu, x, [taps], [tail], want_max=True)
        assert np.array_equal(ys[0], plain) and np.array_equal(rm[0], plain.max(axis=1))


@pytest.mark.parametrize("with_tail", [False, True], ids=["tail0", "tail"])
def test_row_maxima_of_the_pair_of_six_and_six_steps(emu, with_tail):
    """The two-template kernel of 6 + 6 k-steps (supports 163 / 150) with the row maxima."""
    nx, ns = 5, 8193
    x = cs.rows(nx, ns, seed=98)
    tpls = [cs.template(ns, s, zero_mean=not with_tail, seed=s) for s in cs.SUPPORTS[1]]
    tt = [cs.taps_and_tail(tp, with_tail) for tp in tpls]
    taps, tails = [a for a, _ in tt], [b for _, b in tt]
    plain = run(emu, x, taps, tails)
    ys, rm = run(emu, x, taps, tails, want_max=True)
    for t in range(2):
        assert cs.row_err(plain[t], cs.reference(x, tpls[t], with_tail)).max() < TOL
        assert np.array_equal(ys[t], plain[t]) and np.array_equal(rm[t], plain[t].max(axis=1))
