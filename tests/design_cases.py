"""Cases shared by tests/test_oracle_design_edges.py (oracle vs the recorded reference), tests/test_emu_design_edges.py (CPU
emulator build) and tests/test_design_edges_gpu.py (gfx950): the f-k mask designs at odd shapes, at band edges that move
the reference's column loops, and at grid points that sit exactly on a speed edge; the Gaussian blur alone around its
switch to the overlap-save form, on axes shorter than its radius and at odd radii.  Plain NumPy, no torch."""
import numpy as np

from oracle import d4w_oracle as orc

DX = 2.0419046878814697

DEF = dict(cs_min=1400., cp_min=1450., cp_max=3400., cs_max=3500., fmin=15., fmax=25.)      # the designers' defaults
ARGS = dict(cs_min=1350., cp_min=1450., cp_max=3300., cs_max=3450., fmin=14., fmax=30.)     # the scripts' set
TIE = dict(cs_min=1400., cp_min=1600., cp_max=3200., cs_max=3600., fmin=16., fmax=24.)
LOW = dict(cs_min=1400., cp_min=1450., cp_max=3400., cs_max=3500., fmin=2., fmax=10.)
HIGH = dict(cs_min=1400., cp_min=1450., cp_max=3400., cs_max=3500., fmin=30., fmax=45.)

# name -> (shape, selected_channels, dx, fs, parameters)
CASES = {
    "odd_odd": ((41, 481), [0, 41, 1], DX, 200.0, DEF),
    "odd_even": ((41, 480), [0, 164, 4], DX, 200.0, ARGS),
    "even_odd": ((40, 481), [0, 160, 4], DX, 200.0, ARGS),
    "tiny": ((7, 14), [0, 7, 1], DX, 200.0, DEF),
    "one_channel": ((1, 64), [0, 1, 1], DX, 200.0, DEF),
    # a round channel spacing (4 x 2.0 m): |f / k| is exactly 1400, 1600, 3200 or 3600 at many grid points
    "ties_a": ((64, 64), [0, 256, 4], 2.0, 200.0, TIE),
    "ties_b": ((96, 128), [0, 384, 4], 2.0, 200.0, TIE),
    # fmin - 4 and fmin - 14 below zero: the column loops start in the negative-frequency half
    "low_band": ((63, 400), [0, 252, 4], DX, 200.0, LOW),
    # fmax + 14 above Nyquist (50 Hz): np.argmax finds nothing and returns 0, the speed part of hybrid_ninf is skipped
    "high_band": ((63, 400), [0, 252, 4], DX, 100.0, HIGH),
    "wide": ((130, 600), [0, 520, 4], DX, 200.0, ARGS),
    # either axis just past 2048 columns: the blur of that axis runs as overlap-save FFT passes, the other one in LDS
    "ns_2048": ((70, 2050), [0, 280, 4], DX, 200.0, ARGS),
    "nx_2048": ((2049, 66), [0, 2049, 1], DX, 200.0, ARGS),
}
FIXTURE_CASES = tuple(CASES)[:10]             # recorded from the real reference in tests/golden/design_edges.npz
TIE_CASES = ("ties_a", "ties_b")
# points with |f / k| exactly on (cs_min, cp_min, cp_max, cs_max), counted on the float64 axes
TIE_COUNTS = {"ties_a": (14, 125, 62, 12), "ties_b": (30, 61, 30, 56)}
EDGE_CASES = ("ties_a", "ties_b", "low_band", "high_band")      # every point on the right side of its edge

DESIGNS = ("classic", "hybrid", "ninf", "gs", "ninf_gs")
CLOSED = ("classic", "hybrid", "ninf")
_KEYS = {"classic": ("cs_min", "cp_min", "cp_max", "cs_max"),
         "hybrid": ("cs_min", "cp_min", "fmin", "fmax"),
         "ninf": ("cs_min", "cp_min", "cp_max", "cs_max", "fmin", "fmax"),
         "gs": ("cs_min", "cp_min", "fmin", "fmax"),
         "ninf_gs": ("cs_min", "cp_min", "cp_max", "cs_max", "fmin", "fmax")}
FUNCS = {"classic": "fk_filter_design", "hybrid": "hybrid_filter_design", "ninf": "hybrid_ninf_filter_design",
         "gs": "hybrid_gs_filter_design", "ninf_gs": "hybrid_ninf_gs_filter_design"}
# the bounds tests/test_design_gpu.py holds the designs to (max abs)
BOUNDS = {"classic": 5e-7, "hybrid": 5e-7, "ninf": 1e-6, "gs": 3e-6, "ninf_gs": 3e-6}

FKFILT_ARGS = (1, 200., 4, DX, 1400., 3400.)
FKFILT_SHAPES = ((41, 480), (40, 481), (33, 77))

# blur alone: below / at / above the radius, several reflections (5 x 3, 1 x 1), 2047 / 2048 / 2049 columns on either
# axis (LDS kernel | overlap-save form), partial 64 x 64 transpose tiles (65 x 129), more than one FFT block (3 x 4200)
BLUR_SHAPES = ((37, 201), (100, 64), (5, 3), (1, 1), (9, 1100), (30, 2047), (30, 2048), (30, 2049), (2048, 24), (2100, 24),
               (65, 129), (3, 4200))
BLUR_SIGMAS = (20.0, 3.0, 5.2, 0.6, 31.9)     # radii 80, 12, 21 (odd), 2, 128 (the largest the kernels carry)
BLUR_BOUND = 2e-6                             # max abs on values in [0, 1): what tests/test_emu_design.py holds the blur to

FLIP_SHAPES = ((1, 1), (1, 2), (2, 1), (7, 14), (40, 480), (41, 481), (3, 16500))      # the last: beyond 64 x 256 columns
TAPER_NS = (1, 2, 66, 67, 68, 481, 12000)     # floor(0.03 (ns - 1) / 2) goes from 0 to 1 at 68

# closed form into the plan == dense mask into the plan: (case, plan options); the shapes with built-in specialised
# kernels also with the generic passes forced, and a shape whose factors (19, 29) are prime radices
GENERIC = (-1, 0, 0, 0, 0, 0)
FOLD_SHAPES = {"18x48": (18, 48), "8x480": (8, 480), "100x600": (100, 600), "38x406": (38, 406)}
_FOLD_SHAPE_CASES = {name: (shape, [0, 4 * shape[0], 4], DX, 200.0, ARGS) for name, shape in FOLD_SHAPES.items()}
FOLDS = tuple((c, None) for c in ("odd_even", "tiny", "ties_b", "low_band", "high_band", "wide")) + \
    (("18x48", None), ("18x48", GENERIC), ("8x480", None), ("8x480", GENERIC), ("100x600", None), ("100x600", GENERIC),
     ("38x406", (19, 2, 7, 29, 4, 4)))
FOLD_MODES = (("classic", 0.0), ("hybrid", 0.0), ("ninf", 0.0), ("ninf", 4e-6))         # (design, prune_eps): modes 0, 1, 2, 2


def get(case):
    return CASES[case] if case in CASES else _FOLD_SHAPE_CASES[case]


def has_design(case, design):
    """hybrid_ninf_filter_design needs an even ns (the package raises ValueError; the reference returns an
    [nx, ns - 1] mask that no record of that length can be multiplied with)."""
    return not (design == "ninf" and get(case)[0][1] % 2)


def kwargs(design, params):
    return {k: params[k] for k in _KEYS[design]}


def call(module, design, case):
    """module.<designer>(shape, selected_channels, dx, fs, **the design's own parameters) for the oracle, the package's dsp
    or the reference's dsp."""
    shape, sel, dx, fs, params = get(case)
    return getattr(module, FUNCS[design])(shape, sel, dx, fs, **kwargs(design, params))


_oracle = {}


def oracle(case, design):
    """The float64 oracle's mask, computed once per process and shared (read-only)."""
    key = (case, design)
    if key not in _oracle:
        m = np.ascontiguousarray(call(orc, design, case), dtype=np.float64)
        m.setflags(write=False)
        _oracle[key] = m
    return _oracle[key]


def axes(case):
    shape, sel, dx, fs, _ = get(case)
    return orc._shifted_axes(shape, sel, dx, fs)


def tie_counts(case):
    """How many grid points have |f / k| exactly equal to each of the four speeds, from the float64 axes."""
    k, f = axes(case)
    p = get(case)[4]
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.abs(f[None, :] / k[:, None])
    return tuple(int(np.count_nonzero(s == p[n])) for n in ("cs_min", "cp_min", "cp_max", "cs_max"))


def loop_range(case, margin):
    """(i0, i1) of the reference's column loop: first indices with f >= fmin - margin and f >= fmax + margin."""
    _, f = axes(case)
    p = get(case)[4]
    return orc._first_index_ge(f, p["fmin"] - margin), orc._first_index_ge(f, p["fmax"] + margin)


def butter_row(case):
    """The |H|^2 row of hybrid_ninf (host, SciPy) as the package forms it (reference dsp.py:348-349)."""
    import scipy.signal as sps
    shape, _, _, fs, p = get(case)
    ns = shape[1]
    b, a = sps.butter(8, [p["fmin"] / (fs / 2), p["fmax"] / (fs / 2)], "bp")
    return np.concatenate((np.zeros(ns // 2), np.abs(sps.freqz(b, a, worN=ns // 2)[1]) ** 2))


def kernel_args(case, design):
    """What the package hands d4w_design_mask_f32 / d4w_fk_set_mask_design_f32 for a design: (mode, k spacing, t spacing,
    parameters, i0, i1, |H|^2 row or None).  gs is blurred afterwards; ninf_gs is blurred, then flip-summed."""
    _, sel, dx, fs, p = get(case)
    step, dt = sel[2] * dx, 1.0 / fs
    if design == "classic":
        return 0, step, dt, [p[k] for k in _KEYS["classic"]], 0, 0, None
    if design in ("hybrid", "gs"):
        i0, i1 = loop_range(case, 4.0)
        return (1 if design == "hybrid" else 3), step, dt, [p["cs_min"], p["cp_min"], p["fmin"], p["fmax"]], i0, i1, None
    if design == "ninf":
        i0, i1 = loop_range(case, 14.0)
        return 2, step, dt, [p[k] for k in _KEYS["classic"]], i0, i1, butter_row(case)
    i0, i1 = loop_range(case, 4.0)
    return 4, step, dt, [p[k] for k in _KEYS["ninf_gs"]], i0, i1, None


def sides_agree(mask, ref):
    """Every grid point on the right side of its edge: (mask != 0) == (ref != 0), zeros included, leaving out the non-zero
    points with |ref| < 1e-6 (float32 flushes the far Butterworth tails of hybrid_ninf, down to 1e-48, to zero; the
    reference's cos(pi / 2) = 6.1e-17 in hybrid's column at fmax + 4 Hz is rounding, not a side).  Returns (points on the
    wrong side, points left out in the columns where ref reaches 1e-6 at all, grid points of those columns): outside
    those columns nothing is above the threshold whichever side of a speed edge it is on."""
    ref = np.asarray(ref)
    tiny = (np.abs(ref) < 1e-6) & (ref != 0)
    wrong = int(np.count_nonzero(((np.asarray(mask) != 0) != (ref != 0)) & ~tiny))
    live = (np.abs(ref) >= 1e-6).any(axis=0)
    return wrong, int(np.count_nonzero(tiny[:, live])), int(ref.shape[0] * np.count_nonzero(live))


def blur_input(shape):
    return np.random.default_rng(1000 * shape[0] + shape[1]).random(shape).astype(np.float32)


_blur_ref = {}


def blur_reference(shape, sigma):
    """scipy.ndimage.gaussian_filter (reflect boundary, truncate 4) of the float64 copy of blur_input(shape)."""
    from scipy import ndimage
    key = (tuple(shape), float(sigma))
    if key not in _blur_ref:
        r = ndimage.gaussian_filter(blur_input(shape).astype(np.float64), sigma)
        r.setflags(write=False)
        _blur_ref[key] = r
    return _blur_ref[key]


def flip_sum_reference(m32):
    """M + fliplr(M), then + flipud, in float32 and in the kernel's order: (a + b) + (c + d)."""
    m = np.asarray(m32, dtype=np.float32)
    return (m + m[:, ::-1]) + (m[::-1, :] + m[::-1, ::-1])


def fkfilt_block(shape):
    return np.random.default_rng(7000 + 100 * shape[0] + shape[1]).standard_normal(shape)


def fold_block(shape):
    return np.random.default_rng(shape[0] * shape[1]).standard_normal(shape).astype(np.float32)


def rel(y, ref):
    return float(np.max(np.abs(np.asarray(y, dtype=np.float64) - ref)) / np.max(np.abs(ref)))
