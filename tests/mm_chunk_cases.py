"""Cases shared by tests/test_emu_mm_chunks.py (CPU emulator) and tests/test_mm_chunks_gpu.py: the matched filter's
two-template kernel walks a row in chunks of 8192 lags, the one-template kernels in chunks of 4096, and both stage, scale
and prefix-sum in groups of 4096 -- so the row lengths sit around one and two groups, the row kinds are the ones whose
prefix sums differ most, and the row counts are set by each test around its grid."""
import numpy as np

from oracle import d4w_oracle as orc

FS = 200.0
# below one group, exactly one, one plus a remainder shorter than the halo (192), below / exactly / above one 8192-lag chunk,
# a chunk plus most of a group, two chunks plus one sample
NS = (4095, 4096, 4100, 8191, 8192, 8193, 12000, 16385)
KINDS = ("white", "drift", "step", "heavy")
# supports of the fin-call templates (136 / 156: the 5 + 6 k-step kernel) and a pair that is no multiple of 4 (6 + 6 k-steps)
SUPPORTS = ((136, 156), (163, 150))


def rows(nx, ns, seed, first_kind=0):
    """nx float32 rows of ns samples, their kinds cycling from first_kind: white noise; a slow drift under a little noise; a
    step; noise on an offset of 2000 standard deviations (|mean| > 0.992 max|x|: the kernel scales such rows group by group)."""
    rng = np.random.default_rng(seed)
    t = np.arange(ns) / FS
    out = []
    for r in range(nx):
        kind = KINDS[(first_kind + r) % 4]
        w = rng.standard_normal(ns)
        if kind == "white":
            v = w + 0.3
        elif kind == "drift":
            v = 0.05 * w + np.sin(2 * np.pi * t / (23.0 + r % 7) + r) + 0.2
        elif kind == "step":
            v = np.where(t < 0.37 * t[-1], 1.0, -1.0) + 0.01 * w + 0.2
        else:
            v = 0.37 * w + 0.37 * 2000.0 * (1.0 if r % 8 < 4 else -1.0)
        out.append(v)
    return np.ascontiguousarray(np.stack(out), dtype=np.float32)


def kinds(nx, first_kind=0):
    return [KINDS[(first_kind + r) % 4] for r in range(nx)]


def template(ns, support, zero_mean, seed):
    """A template zero-padded to ns samples.  zero_mean: the support sums to zero (no tail on the padding: tail coefficient 0
    to rounding -- the callers pass exactly 0); otherwise all taps positive, mean / max of the order of support / ns."""
    rng = np.random.default_rng(seed)
    tpl = np.zeros(ns)
    if zero_mean:
        c = rng.standard_normal(support) * np.hanning(support + 2)[1:-1]
        c -= c.mean()
    else:
        c = np.abs(rng.standard_normal(support)) + 0.2
    tpl[:support] = c
    return tpl


def taps_and_tail(tpl, with_tail):
    """What detect.compute_cross_correlograms hands the kernel: the normalised support (detect.py:158) and the coefficient of
    the constant the normalisation leaves on the padding.  with_tail=False: the template is normalised over its SUPPORT's own
    scale without the de-meaning over the padding (coefficient exactly 0)."""
    tpl = np.asarray(tpl, dtype=np.float64)
    L = int(np.max(np.nonzero(tpl)[0])) + 1
    if with_tail:
        return ((tpl - tpl.mean()) / np.max(np.abs(tpl)))[:L], float(tpl.mean() / np.max(np.abs(tpl)))
    return (tpl / np.max(np.abs(tpl)))[:L], 0.0


def reference(x32, tpl, with_tail, head=None):
    """float64 correlograms of the float32 rows the kernel sees (head: the record's continuation behind every row, entering
    the lags but not the rows' statistics)."""
    x = np.asarray(x32, dtype=np.float64)
    if with_tail and head is None:
        return orc.compute_cross_correlogram(x, tpl)
    ns = x.shape[1]
    xn = (x - x.mean(axis=1, keepdims=True)) / np.max(np.abs(x), axis=1, keepdims=True)
    if head is not None:
        hn = (np.asarray(head, dtype=np.float64) - x.mean(axis=1, keepdims=True)) / np.max(np.abs(x), axis=1, keepdims=True)
        xn = np.concatenate((xn, hn), axis=1)
    tp, _ = taps_and_tail(tpl, with_tail)
    tpad = np.pad(tp, (0, xn.shape[1] - len(tp)))
    return np.stack([orc.shift_xcorr(r, tpad)[:ns] for r in xn])


def row_err(y, ref):
    """Every row against its own maximum."""
    return np.max(np.abs(np.asarray(y, dtype=np.float64) - ref), axis=1) / np.max(np.abs(ref), axis=1)
