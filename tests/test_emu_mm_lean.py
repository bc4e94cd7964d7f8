"""The two bodies of the two-template matched filter on the CPU emulator (csrc/xcorr_mm.hip; cases: tests/mm_lean_cases.py).
A chunk whose whole stage lies inside an ordinary row takes the LEAN loop body, every other chunk the general one, and the
software pipeline runs across the two -- so: row lengths with no, one and several lean chunks and with an end chunk of every
sort, rows that make a workgroup change body between two rows (offset-heavy rows between ordinary ones, on the emulator's
grids of 4 workgroups for the pair and 6 for one template), a row with a NaN, an unaligned x, a continuation shorter than the
halo; tail coefficients zero (chunks dealt over the grid) and non-zero (whole rows per workgroup), with and without the row
maxima.

(a) every row against a float64 correlation, 2e-6 of the row's own maximum (the bound of tests/test_emu_mm_chunks.py);
(b) the two-template launch against the two one-template launches (which have the general body only), bit for bit."""
import numpy as np
import pytest

from tests import mm_chunk_cases as cs
from tests import mm_lean_cases as lc
from tests.emu_util import load_emu
from tests.test_emu_mm_chunks import run

# rows 1 and 4 are offset-heavy.  Whole rows on 4 workgroups: workgroup 0 goes ordinary -> heavy (rows 0, 4), workgroup 1
# heavy -> ordinary (rows 1, 5); dealt chunks meet the rows in order.  (The longest rows have no lean chunk: three rows.)
NX = 6


def nx_of(ns):
    return NX if ns % 4 == 0 else 3


@pytest.fixture(scope="module")
def emu():
    return load_emu()


@pytest.fixture(scope="module")
def singles(emu):
    """The one-template launches of a case, run once: (ns, with_tail) -> [y0, y1]."""
    memo = {}

    def get(ns, with_tail):
        if (ns, with_tail) not in memo:
            x, _, taps, tails = lc.case(nx_of(ns), ns, with_tail)
            memo[(ns, with_tail)] = [run(emu, x, [taps[t]], [tails[t]])[0] for t in range(2)]
        return memo[(ns, with_tail)]
    return get


@pytest.mark.parametrize("want_max", [False, True], ids=["plain", "rowmax"])
@pytest.mark.parametrize("with_tail", [False, True], ids=["tail0", "tail"])
@pytest.mark.parametrize("ns", lc.NS)
def test_lean_and_general_chunks_in_one_walk(emu, singles, ns, with_tail, want_max):
    nx = nx_of(ns)
    x, _, taps, tails = lc.case(nx, ns, with_tail)
    got = run(emu, x, taps, tails, want_max=want_max)
    pair, rm = got if want_max else (got, None)
    for t in range(2):
        e = cs.row_err(pair[t], lc.reference(nx, ns, with_tail, t))
        print("ns %d %s template %d: worst row %.2e (%s)" % (ns, "tail" if with_tail else "tail0", t, e.max(), lc.kind(int(e.argmax()))))
        assert e.max() < lc.TOL, (t, e, lc.kinds(nx))
        assert np.array_equal(singles(ns, with_tail)[t], pair[t]), "lean and general body: different values"
        if want_max:
            assert np.array_equal(rm[t], pair[t].max(axis=1))


@pytest.mark.parametrize("with_tail", [False, True], ids=["tail0", "tail"])
def test_a_row_with_a_nan(emu, singles, with_tail):
    """A NaN in an ordinary row: its lean chunk and its end chunk store NaN, its maximum is NaN (np.max), the other rows keep
    their values and maxima, and the one-template kernel gives the same row."""
    ns = 8388
    x, _, taps, tails = lc.case(NX, ns, with_tail)
    base = singles(ns, with_tail)
    xn = np.array(x)
    assert lc.kind(3) != "heavy"
    xn[3, 5000] = np.nan
    ys, rm = run(emu, xn, taps, tails, want_max=True)
    keep = [r for r in range(NX) if r != 3]
    for t in range(2):
        assert np.isnan(rm[t][3]) and np.isnan(ys[t][3]).any()
        assert np.array_equal(ys[t][keep], base[t][keep]) and np.array_equal(rm[t][keep], base[t][keep].max(axis=1))
    (one,) = run(emu, xn, [taps[1]], [tails[1]])
    assert lc.same(one, ys[1])


@pytest.mark.parametrize("with_tail", [False, True], ids=["tail0", "tail"])
def test_an_unaligned_x(emu, with_tail):
    """x (and the outputs) one float past a 16-byte boundary: no chunk is lean.  Against float64 and the one-template launches
    on the same arrays (the statistics of an unaligned row are summed in another order: no bit comparison with the aligned call)."""
    ns = 8388
    x, _, taps, tails = lc.case(NX, ns, with_tail)
    got = run(emu, x, taps, tails, misalign=1)
    for t in range(2):
        assert cs.row_err(got[t], lc.reference(NX, ns, with_tail, t)).max() < lc.TOL
        (one,) = run(emu, x, [taps[t]], [tails[t]], misalign=1)
        assert np.array_equal(one, got[t])


@pytest.mark.parametrize("with_tail", [False, True], ids=["tail0", "tail"])
def test_a_continuation_shorter_than_the_halo(emu, singles, with_tail):
    """The record continues for 50 samples (clamped samples: the general body in every chunk).  The pair equals the one-template
    launch bit for bit, the last lags moved, the lags of an ordinary row that read nothing of the head are the plain call's
    bit for bit, and without the tail term the rows meet float64 of [x | head] with x's statistics."""
    ns, n_next = 8388, 50
    x, tpls, taps, tails = lc.case(NX, ns, with_tail)
    rng = np.random.default_rng(ns)
    head = np.ascontiguousarray(rng.standard_normal((NX, 64)) * x.std(axis=1, keepdims=True) + x.mean(axis=1, keepdims=True), dtype=np.float32)
    base = singles(ns, with_tail)
    cont = run(emu, x, taps, tails, nxt=head, n_next=n_next)
    # (an offset-heavy row's last group may take another power of two with the head in it)
    plain_rows = [r for r in range(NX) if lc.kind(r) != "heavy"]
    for t in range(2):
        assert not np.array_equal(cont[t][:, -100:], base[t][:, -100:])
        assert np.array_equal(cont[t][plain_rows, :ns - 400], base[t][plain_rows, :ns - 400])
        if not with_tail:
            assert cs.row_err(cont[t], cs.reference(x, tpls[t], False, head=head[:, :n_next])).max() < lc.TOL
    (one,) = run(emu, x, [taps[0]], [tails[0]], nxt=head, n_next=n_next)
    assert np.array_equal(one, cont[0])
