"""Cases, inputs and float64 references shared by tests/test_emu_resample.py (CPU emulator) and tests/test_resample_gpu.py.

Reference: scipy.signal.resample_poly / scipy.signal.decimate(ftype='fir') in float64 on the float32-rounded input.
Tolerance: the project's per-row bound (tests/welch_cases.py check_rows), max|y - ref| <= 1e-5 * max|ref| over each row; a
float32 running sum over the 101 taps of q = 5 is 3.4e-7 .. 3.9e-7 of the row maximum, so the bound leaves room without hiding
an indexing error.  Rows of every case: seeded white noise; the same with an offset of 1000 x its rms; a 20 Hz tone (at
1 kHz) plus noise."""
import functools

import numpy as np
import scipy.signal as sps

TOL = 1e-5
FS = 1000.0
DEFAULT_WINDOW = ("kaiser", 5.0)


def window_of(name):
    """The `window` argument of a case: SciPy's default, or the taps themselves (odd and even length)."""
    if name is None:
        return DEFAULT_WINDOW
    if name == "taps101":
        return sps.firwin(101, 0.2, window="hamming")
    if name == "taps40":
        return sps.firwin(40, 0.25)
    raise KeyError(name)


# id -> (nx, ns, up, down, window name, padtype, cval)
CASES = {
    # odd and even strides, every gcd of the stride with the bank count
    "1000_1_5": (3, 1000, 1, 5, None, "constant", None),
    "1001_1_5": (3, 1001, 1, 5, None, "constant", None),
    "999_1_2": (3, 999, 1, 2, None, "constant", None),
    "1000_1_4": (3, 1000, 1, 4, None, "constant", None),
    "1000_1_8": (3, 1000, 1, 8, None, "constant", None),
    "1003_1_10": (3, 1003, 1, 10, None, "constant", None),
    "1300_1_13": (3, 1300, 1, 13, None, "constant", None),
    # up > 1; the last reduces to 2 / 3
    "777_2_5": (3, 777, 2, 5, None, "constant", None),
    "1000_3_2": (3, 1000, 3, 2, None, "constant", None),
    "500_5_1": (3, 500, 5, 1, None, "constant", None),
    "1000_4_6": (3, 1000, 4, 6, None, "constant", None),
    # rows shorter than the taps
    "61_1_5": (3, 61, 1, 5, None, "constant", None),
    "40_1_5": (3, 40, 1, 5, None, "constant", None),
    "1_1_5": (3, 1, 1, 5, None, "constant", None),
    # a long row: at least three tiles
    "12000_1_5": (3, 12000, 1, 5, None, "constant", None),
    # the taps themselves, odd and even length
    "taps101_1_5": (3, 1000, 1, 5, "taps101", "constant", None),
    "taps40_1_4": (3, 1000, 1, 4, "taps40", "constant", None),
    "taps40_2_5": (3, 777, 2, 5, "taps40", "constant", None),
    # what is removed before the filter and put back after it
    "mean_1_5": (3, 1000, 1, 5, None, "mean", None),
    "mean_2_5": (3, 777, 2, 5, None, "mean", None),
    "cval_1_5": (3, 1000, 1, 5, None, "constant", 3.5),
    "cval_3_2": (3, 1000, 3, 2, None, "constant", 3.5),
}
COPY_CASE = (3, 1000, 3, 3)
# more than one wave of workgroups (GPU file only)
GPU_CASES = dict(CASES, rows_64x12000=(64, 12000, 1, 5, None, "constant", None))
DECIMATE_CASES = {"q2": (1000, 2, None), "q5": (1001, 5, None), "q13": (1300, 13, None), "q5_n30": (1000, 5, 30)}


def rows(nx, ns, seed):
    """float32 [nx, ns], read-only: noise / noise at an offset of 1000 x its rms / a 20 Hz tone plus noise, in turn."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nx, ns))
    t = np.arange(ns) / FS
    for r in range(nx):
        if r % 3 == 1:
            x[r] += 1000.0 * np.sqrt(np.mean(x[r] ** 2))
        elif r % 3 == 2:
            x[r] = np.sin(2.0 * np.pi * 20.0 * t + 0.3 * r) + 0.1 * x[r]
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def make_input(name):
    nx, ns = GPU_CASES[name][:2]
    return rows(nx, ns, sorted(GPU_CASES).index(name) + 300)


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 [nx, ceil(ns up / down)]."""
    nx, ns, up, down, win, padtype, cval = GPU_CASES[name]
    ref = sps.resample_poly(make_input(name).astype(np.float64), up, down, axis=-1, window=window_of(win), padtype=padtype,
                            cval=cval)
    assert ref.shape == (nx, -(-ns * up // down))
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def decimate_input(name):
    return rows(3, DECIMATE_CASES[name][0], sorted(DECIMATE_CASES).index(name) + 400)


@functools.lru_cache(maxsize=None)
def decimate_reference(name):
    _, q, n = DECIMATE_CASES[name]
    ref = sps.decimate(decimate_input(name).astype(np.float64), q, n=n, ftype="fir", axis=-1, zero_phase=True)
    ref.setflags(write=False)
    return ref


def check_rows(y, ref, what=""):
    """Every row within TOL of its own largest reference value; prints the worst figure before it asserts."""
    y = np.asarray(y, dtype=np.float64)
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    err = np.abs(y - ref).max(axis=1) / np.abs(ref).max(axis=1)
    print("resample %s: max row error / row maximum = %.3e (rows %s)" % (what, err.max(), np.array2string(err[:4], precision=2)))
    assert np.all(np.isfinite(y)), what
    assert err.max() <= TOL, (what, err)


# ---- continuation: a 3 x 3000 record cut into three files of 1000 -----------------------------------------------------------
RECORD_FILES, RECORD_FILE_NS = 3, 1000
# (up, down, window name).  The designed taps (20 max(up, down) + 1 of them at a cut-off of 1 / max(up, down)) end on zeros of
# the sinc: their outermost taps are ~1e-18 and a neighbour block one sample short of the reach gives the same float32 bits.
# "One sample short differs" therefore runs on 99 taps at the same cut-off (the ends fall between two zeros of the sinc);
# "bit for bit with the whole record" runs on both.
CONTINUATION = {"1_5": (1, 5, None), "2_5": (2, 5, None), "1_5_taps99": (1, 5, "taps99"), "2_5_taps99": (2, 5, "taps99")}


def continuation_window(name):
    return sps.firwin(99, 0.2, window="hamming") if name == "taps99" else window_of(name)


@functools.lru_cache(maxsize=None)
def record():
    return rows(3, RECORD_FILES * RECORD_FILE_NS, 500)


# ---- fused ingest: raw [10, 4000], rows 1:9:2, q = 5 ---------------------------------------------------------------------------
INGEST_SEL = [1, 9, 2]
INGEST_Q = 5
INGEST_META = {"fs": FS, "dx": 2.0419, "scale_factor": 1e-9 * 1.7}
INGEST_OFFSETS = {"int32": (0.0, 1e6, -3e5, 2e9), "int16": (0.0, 30000.0, -20000.0), "float32": (0.0, 30000.0, -20000.0)}


@functools.lru_cache(maxsize=None)
def ingest_raw(dtype):
    """raw [10, 4000] of `dtype`: row c is offset[(c // 2) % len] + 100 x noise (rounded for the integer types), so that the
    selected rows 1, 3, 5, 7 take the offsets in turn.  A kernel that converts to float32 before it removes the mean fails
    the 2e9 row by orders of magnitude (float32 resolves 128 there)."""
    rng = np.random.default_rng(600 + sorted(INGEST_OFFSETS).index(dtype))
    offs = INGEST_OFFSETS[dtype]
    v = np.array([offs[(c // 2) % len(offs)] for c in range(10)])[:, None] + 100.0 * rng.standard_normal((10, 4000))
    raw = np.round(v).astype(dtype) if dtype.startswith("int") else v.astype(dtype)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def ingest_reference(dtype):
    sel = ingest_raw(dtype)[INGEST_SEL[0]:INGEST_SEL[1]:INGEST_SEL[2]].astype(np.float64)
    strain = (sel - sel.mean(axis=1, keepdims=True)) * INGEST_META["scale_factor"]
    ref = sps.resample_poly(strain, 1, INGEST_Q, axis=-1, window=sps.firwin(101, 0.2, window="hamming"))
    ref.setflags(write=False)
    return ref
