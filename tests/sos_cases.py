"""The zero-phase second-order-section filter's test table: designs, inputs, float64 reference and bars, shared by the
GPU path tests (tests/test_sos_paths_gpu.py) and their emulator twins (tests/test_emu_rowops.py).  No GPU import here.

A case is (design, shape).  Its input rows cycle through kinds (KINDS, plus two offset-heavy kinds for the low-passes), are
seeded, and are rounded to float32 BEFORE the reference sees them.  The reference is scipy.signal.sosfiltfilt in float64 with
the same padlen.  The bar is the suite's 1e-5 * max|ref| over the block's ordinary rows; offset-heavy rows are judged one by
one (see judge)."""
import functools

import numpy as np
import scipy.signal as sps

FS = 200.0
TOL = 1e-5
F64_DMIN = 0.015          # csrc/rowops.hip sos_prepare: float64 states below this
COND_MAX = 1e-6           # a case whose float32 workspace alone costs more than this is not a test of the kernel

# name: (order, btype, corner(s) in Hz, sections, states, (pass-band tone, stop-band tone) in Hz)
DESIGNS = {
    "hp1": (1, "hp", 5.0, 1, "float", (40.0, 0.5)),
    "hp3": (3, "hp", 10.0, 2, "float", (40.0, 2.0)),
    "hp5": (5, "hp", 2.0, 3, "double", (20.0, 0.3)),
    "lp4": (4, "lp", 30.0, 2, "float", (5.0, 60.0)),
    "bp4": (4, "bp", (10.0, 40.0), 4, "float", (20.0, 3.0)),      # so that every section count 1 .. 10 is in the table
    "bp5": (5, "bp", (10.0, 40.0), 5, "float", (20.0, 3.0)),
    "bp6": (6, "bp", (10.0, 40.0), 6, "float", (20.0, 3.0)),
    "bp7": (7, "bp", (10.0, 40.0), 7, "float", (20.0, 3.0)),
    "lp12": (12, "lp", 30.0, 6, "float", (5.0, 60.0)),
    "lp14": (14, "lp", 40.0, 7, "float", (5.0, 70.0)),
    "bp8": (8, "bp", (14.0, 30.0), 8, "float", (20.0, 5.0)),
    "bp8w": (8, "bp", (5.0, 38.0), 8, "double", (20.0, 1.0)),
    "bp9": (9, "bp", (20.0, 45.0), 9, "float", (30.0, 5.0)),
    "bp10": (10, "bp", (20.0, 45.0), 10, "float", (30.0, 5.0)),
    "lp17": (17, "lp", 40.0, 9, "float", (5.0, 70.0)),
    "bp9w": (9, "bp", (6.0, 40.0), 9, "double", (20.0, 1.0)),
    "bp10w": (10, "bp", (5.0, 38.0), 10, "double", (20.0, 1.0)),
    "lp20": (20, "lp", 10.0, 10, "double", (3.0, 30.0)),
}
NAMES = list(DESIGNS)
ONE_PER_NSEC = ["hp1", "hp3", "hp5", "bp8w", "bp4", "bp5", "bp6", "bp7", "bp8", "bp9", "bp10", "bp9w", "bp10w", "lp20", "lp4"]
FFT_DESIGNS = ["bp8", "bp10", "bp10w", "hp3", "lp12", "lp17"]

KINDS = ("white", "tones", "step", "const")
HEAVY = ("offset1e3", "offset1e5")          # low-pass designs only


@functools.lru_cache(maxsize=None)
def design(name):
    order, btype, f, nsec, _, _ = DESIGNS[name]
    sos = np.ascontiguousarray(sps.butter(order, np.asarray(f) / (FS / 2), btype, output="sos"), dtype=np.float64)
    assert sos.shape == (nsec, 6), (name, sos.shape)
    return sos


def dmin(sos):
    """sos_prepare's conditioning figure: min over the sections and 1025 points of the upper unit circle of
    |1 + a1 z^-1 + a2 z^-2|."""
    w = np.pi * np.arange(1025) / 1024.0
    z1, z2 = np.exp(-1j * w), np.exp(-2j * w)
    return float(min(np.min(np.abs(1.0 + (c[4] / c[3]) * z1 + (c[5] / c[3]) * z2)) for c in sos))


def states(name):
    """'float' or 'double', asserted to lie on the intended side of the library's threshold."""
    d, want = dmin(design(name)), DESIGNS[name][4]
    assert (d < F64_DMIN) == (want == "double"), (name, d)
    return want


def expected_form(name, lanes=True, forced=None):
    """What d4w_sosfiltfilt_last_form reports after a call on this design: lanes per row (1: sos_pass; 8 up to 8 sections, 16
    for 9 - 10: sos_pass_lanes) + 100 x bytes per state (`forced`: the precision D4W_SOS_F64 imposes)."""
    nsec = DESIGNS[name][3]
    return ((8 if nsec <= 8 else 16) if lanes else 1) + (800 if (forced or states(name)) == "double" else 400)


def default_padlen(sos):
    """scipy/signal/_signaltools.py sosfiltfilt."""
    ntaps = 2 * sos.shape[0] + 1
    ntaps -= min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum()))
    return 3 * ntaps


def kinds_of(name):
    return KINDS + (HEAVY if DESIGNS[name][1] == "lp" else ())


def row_kinds(name, nx):
    k = kinds_of(name)
    return [k[r % len(k)] for r in range(nx)]


@functools.lru_cache(maxsize=None)
def _rows(name, nx, ns):
    rng = np.random.default_rng(1000 * NAMES.index(name) + ns)
    fp, fstop = DESIGNS[name][5]
    t = np.arange(ns) / FS
    x = np.empty((nx, ns))
    for r, kind in enumerate(row_kinds(name, nx)):
        if kind == "white":
            x[r] = rng.standard_normal(ns) + 3.0 * rng.standard_normal()
        elif kind == "tones":
            x[r] = np.sin(2 * np.pi * fp * t + 0.3 * r) + 0.7 * np.sin(2 * np.pi * fstop * t + 0.1)
        elif kind == "step":
            x[r] = np.where(np.arange(ns) < ns // 3 + r, -0.5, 1.5) + 0.01 * rng.standard_normal(ns)
        elif kind == "const":
            x[r] = 1.7 + 0.1 * r
        else:
            sig = 0.37
            x[r] = sig * rng.standard_normal(ns) + sig * (1e3 if kind == "offset1e3" else 1e5) * (-1.0) ** r
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


MAX_NX = 67


def rows(name, nx, ns):
    """float32 [nx, ns]: the first nx rows of the design's 67-row block of that length (read-only, shared)."""
    assert nx <= MAX_NX
    return _rows(name, MAX_NX, ns)[:nx]


@functools.lru_cache(maxsize=None)
def _reference(name, ns, padlen):
    ref = sps.sosfiltfilt(design(name), _rows(name, MAX_NX, ns).astype(np.float64), axis=1, padlen=padlen)
    ref.setflags(write=False)
    return ref


def reference(name, nx, ns, padlen=None):
    sos = design(name)
    return _reference(name, ns, default_padlen(sos) if padlen is None else padlen)[:nx]


def filtfilt_f32_workspace(sos, x, padlen):
    """float64 filtfilt whose forward output is rounded to float32 -- what the library's workspace stores between the
    passes: the part of the error no kernel can avoid."""
    x = np.asarray(x, dtype=np.float64)
    ext = np.concatenate((2 * x[:, :1] - x[:, padlen:0:-1], x, 2 * x[:, -1:] - x[:, -2:-padlen - 2:-1]), axis=1) if padlen else x
    zi = sps.sosfilt_zi(sos)[:, None, :]
    f, _ = sps.sosfilt(sos, ext, axis=1, zi=zi * ext[:, :1][None])
    f = f.astype(np.float32).astype(np.float64)
    b, _ = sps.sosfilt(sos, f[:, ::-1], axis=1, zi=zi * f[:, -1:][None])
    b = b[:, ::-1]
    return b[:, padlen:b.shape[1] - padlen] if padlen else b


def heavy_bar(ref_row):
    """The bar of an offset-heavy row's DE-MEANED output: 1e-5 of max|ref - mean| for the filter of the signal, plus what the
    float32 OUTPUT format costs at the offset's magnitude -- the offset is put back as float(c) * float(|H(1)|^2) + y, and
    the squared DC gain of a low-pass is 1 to within its float32 rounding: half an ulp for the product, half an ulp for the
    sum = 1 ulp(max|ref|).  (1e-5 of max|ref - mean| alone, ~6e-6 here, is below half an ulp of a float32 of 3.7e4, 2e-3: no
    float32 output can hold it.)"""
    return TOL * np.max(np.abs(ref_row - ref_row.mean())) + float(np.spacing(np.float32(np.max(np.abs(ref_row)))))


def judge(y, ref, kinds, what=""):
    """Asserts y against ref and returns the figures {'rel': block error / max|ref| over the ordinary rows, 'heavy': worst
    offset-heavy row error / its own max|ref|, 'heavy_demeaned': worst such error / that row's de-meaned bar (<= 1 passes)}."""
    y = np.asarray(y, dtype=np.float64)
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    assert np.isfinite(y).all(), what
    plain = [r for r, k in enumerate(kinds) if k not in HEAVY]
    out = {"rel": 0.0, "heavy": 0.0, "heavy_demeaned": 0.0}
    if plain:
        out["rel"] = float(np.max(np.abs(y[plain] - ref[plain])) / np.max(np.abs(ref[plain])))
        assert out["rel"] < TOL, (what, out)
    for r, k in enumerate(kinds):
        if k in HEAVY:
            e = float(np.max(np.abs(y[r] - ref[r])))
            out["heavy"] = max(out["heavy"], e / float(np.max(np.abs(ref[r]))))
            out["heavy_demeaned"] = max(out["heavy_demeaned"], e / heavy_bar(ref[r]))
            assert e < TOL * np.max(np.abs(ref[r])) and e <= heavy_bar(ref[r]), (what, r, k, e, heavy_bar(ref[r]))
    return out


@functools.lru_cache(maxsize=None)
def conditioning(name, ns, padlen):
    """The float32-workspace figure of the design's 67-row block, as judge measures errors (ordinary rows over the block,
    offset-heavy rows over their own maximum): asserted below COND_MAX by every test that uses the block."""
    return cond_figure(filtfilt_f32_workspace(design(name), _rows(name, MAX_NX, ns), padlen), _reference(name, ns, padlen),
                       row_kinds(name, MAX_NX))


def cond_figure(got, ref, kinds):
    plain = [r for r, k in enumerate(kinds) if k not in HEAVY]
    fig = float(np.max(np.abs(got[plain] - ref[plain])) / np.max(np.abs(ref[plain])))
    for r, k in enumerate(kinds):
        if k in HEAVY:
            fig = max(fig, float(np.max(np.abs(got[r] - ref[r])) / np.max(np.abs(ref[r]))))
    return fig


def case(name, nx, ns, padlen=None):
    """(x float32 [nx, ns], ref float64, row kinds, padlen) of one case, its design on the intended side of the precision
    threshold and its conditioning figure below COND_MAX."""
    states(name)
    sos = design(name)
    padlen = default_padlen(sos) if padlen is None else padlen
    c = conditioning(name, ns, padlen)
    assert c < COND_MAX, (name, ns, c)
    return rows(name, nx, ns), reference(name, nx, ns, padlen), row_kinds(name, nx), padlen


def segmentation(sos, decay):
    """(seg_len, warm, ns) of the segmented form: warm as dsp._sosfiltfilt_recursive derives it from the impulse
    response's decay, segments of about half of it, the shortest ragged row that still has >= 3 segments."""
    warm = -(-int(1.5 * decay) // 32) * 32
    seg_len = max(64, -(-(warm // 2) // 32) * 32)
    ns = seg_len + 2 * warm + 37
    assert ns % 32 and seg_len + 2 * warm < ns and -(-ns // seg_len) >= 3
    return seg_len, warm, ns


def check_row_ends(run, name, x, kinds, padlen, piece, keep, fill=7.5):
    """d4w_sosfiltfilt_ends_f32 / _ends_sides_f32 on the block x.  run(phases, sides) -> the [nx, ns] output after one call
    per phase on a y pre-filled with `fill`.  Forward and backward phase as two calls equal the single call bit for bit; the
    kept columns ([0, keep) and [ns - keep, ns)) hold the bar against float64 sosfiltfilt of the gathered pieces; every other
    column keeps `fill`; one side alone writes exactly that side's columns of the two-sided result.  Returns judge's figures."""
    sos = design(name)
    states(name)
    nx, ns = x.shape
    pieces = np.concatenate((x[:, :piece], x[:, ns - piece:]), axis=0).astype(np.float64)
    ref = sps.sosfiltfilt(sos, pieces, axis=1, padlen=padlen)
    cond = cond_figure(filtfilt_f32_workspace(sos, pieces, padlen), ref, list(kinds) + list(kinds))
    assert cond < COND_MAX, (name, cond)
    left, right = ref[:nx, :keep], ref[nx:, piece - keep:]
    one, split = run((0,), 3), run((1, 2), 3)
    assert np.array_equal(one, split), name
    assert np.all(one[:, keep:ns - keep] == fill), name
    figs = judge(np.concatenate((one[:, :keep], one[:, ns - keep:]), axis=1), np.concatenate((left, right), axis=1), kinds,
                 name + " row ends")
    for sides, sl, r in ((1, slice(0, keep), left), (2, slice(ns - keep, ns), right)):
        y1 = run((0,), sides)
        judge(y1[:, sl], r, kinds, "%s sides=%d" % (name, sides))
        assert np.array_equal(y1[:, sl], one[:, sl]), (name, sides)
        rest = np.ones(ns, dtype=bool)
        rest[sl] = False
        assert np.all(y1[:, rest] == fill), (name, sides)
    figs["cond"] = cond
    return figs
