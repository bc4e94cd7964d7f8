"""Cases shared by tests/test_emu_mm_lean.py (CPU emulator) and tests/test_mm_lean_gpu.py: the two-template matched filter
(csrc/xcorr_mm.hip) computes a chunk whose whole stage (its lags + 192 samples of halo) lies inside an ordinary row -- 16-byte
aligned, a multiple of four samples, scaled by the caller's 1 / max|x| -- with a LEAN loop body, and every other chunk (a row's
end, an offset-heavy, unaligned or continued row) with the general one.  The row lengths put the boundary between the two
everywhere it can lie, and the row kinds make a workgroup change from one body to the other between two rows."""
import functools
import json
import sys

import numpy as np

from tests import mm_chunk_cases as cs

# Row lengths around the stages of chunks of 8192 lags (what the pair kernel walked when these cases were chosen) and of 4096
# (what it walks now):
#   4096    an end chunk only (either length)
#   4288    one stage of 4096 + 192 exactly: a lean chunk, then an end chunk of 192 lags
#   4292    ... and an end chunk that is four samples longer
#   8192    exactly one / two chunks, the last one's halo crosses the row end
#   8384    one stage of 8192 + 192 exactly; at 4096 lags the second chunk's stage ends with the row
#   8388    lean chunks and an end chunk of four lags (8192) / of 196 (4096)
#   16 388  several lean chunks, a chunk whose halo crosses the row end, and an end chunk of four lags
#   24 577  not a multiple of four samples -- the general body for every chunk
NS = (4096, 4288, 4292, 8192, 8384, 8388, 16388, 24577)
SUPPORTS = (136, 156)        # the fin-call templates: the 5 + 6 k-step kernel
TOL = 2e-6                   # tests/test_emu_mm_chunks.py: of every row's own maximum
FS = cs.FS


def kind(r):
    """Row r: offset-heavy (|mean| > 0.992 max|x|: scaled group by group, the general body) when r % 3 == 1, else white or
    drifting.  A workgroup that walks whole rows r, r + grid on a grid of 4 (the emulator's), 256 or 512 workgroups goes from an
    ordinary row to a heavy one (r % 3 == 0 on 4 and 256, r % 3 == 2 on 512) and from a heavy one to an ordinary one; one that
    walks dealt chunks meets the rows in order."""
    return "heavy" if r % 3 == 1 else ("white", "drift")[(r // 3) & 1]


def kinds(nx):
    return [kind(r) for r in range(nx)]


def rows(nx, ns, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(ns) / FS
    out = []
    for r in range(nx):
        w = rng.standard_normal(ns)
        k = kind(r)
        if k == "white":
            v = w + 0.3
        elif k == "drift":
            v = 0.05 * w + np.sin(2 * np.pi * t / (23.0 + r % 7) + r) + 0.2
        else:
            v = 0.37 * w + 0.37 * 2000.0 * (1.0 if r % 8 < 4 else -1.0)
        out.append(v)
    return np.ascontiguousarray(np.stack(out), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def case(nx, ns, with_tail):
    """(x, templates, taps, tails) of a case: the same for every test that asks."""
    x = rows(nx, ns, seed=5000 + ns + nx)
    x.setflags(write=False)
    tpls = [cs.template(ns, s, zero_mean=not with_tail, seed=s + ns) for s in SUPPORTS]
    tt = [cs.taps_and_tail(tp, with_tail) for tp in tpls]
    taps, tails = [a for a, _ in tt], [b for _, b in tt]
    if with_tail:
        assert min(abs(c) for c in tails) > 1e-4
    return x, tpls, taps, tails


@functools.lru_cache(maxsize=None)
def reference(nx, ns, with_tail, t, sel=None):
    """float64 correlogram of template t on the case's rows (sel: a tuple of row indices, all rows when None)."""
    x, tpls, _, _ = case(nx, ns, with_tail)
    ref = cs.reference(x if sel is None else x[list(sel)], tpls[t], with_tail)
    ref.setflags(write=False)
    return ref


def checked(nx, n=12):
    """Rows compared with float64 where there are many: the first and the last ones."""
    return tuple(int(v) for v in np.unique(np.r_[np.arange(min(nx, n)), np.arange(max(nx - n, 0), nx)]))


def same(a, b):
    """Bit for bit; a row with a NaN is NaN in the same places."""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _gpu_child(nx, lengths):
    """Run in a fresh process with D4W_MM_WGS=1 (the library reads it once): a grid of one workgroup per compute unit, fewer
    than the nx rows, so that workgroups walk several rows.  Prints the figures the parent test asserts on."""
    import torch
    import das4whales_amd as dw
    out = {}
    for ns in lengths:
        for with_tail in (False, True):
            x, tpls, taps, tails = case(nx, ns, with_tail)
            xd = torch.from_numpy(np.array(x)).cuda()
            tl = tails if with_tail else None
            rm = []
            pair = dw.detect._xcorr_device(xd, taps, normalize=True, method="mm", tails=tl, row_max=rm)
            sel = checked(nx)
            worst, equal, maxima = 0.0, True, True
            for t in range(2):
                y = pair[t].cpu().numpy()
                worst = max(worst, float(cs.row_err(y[list(sel)], reference(nx, ns, with_tail, t, sel)).max()))
                (single,) = dw.detect._xcorr_device(xd, [taps[t]], normalize=True, method="mm", tails=[tails[t]] if with_tail else None)
                equal = equal and bool(torch.equal(single, pair[t]))
                maxima = maxima and bool(torch.equal(rm[t], pair[t].max(dim=1).values))
            out["%d/%s" % (ns, "tail" if with_tail else "tail0")] = {"worst": worst, "pair_equals_single": equal, "row_max": maxima}
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    _gpu_child(int(sys.argv[1]), [int(v) for v in sys.argv[2:]])
