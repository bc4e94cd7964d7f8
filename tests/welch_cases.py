"""Cases, inputs and float64 references shared by tests/test_emu_welch.py (CPU emulator) and tests/test_welch_gpu.py.

Reference: scipy.signal.welch in float64 on the float32-rounded input, chunk by chunk.  Tolerance: the project's 1e-5
(tests/test_spectral_gpu.py) per row, max|p - ref| <= 1e-5 * max(ref) over that row's chunks and bins.
Rows of every case: seeded white noise; the same with a DC offset of 1000 x its rms (a drifting raw strain row: a float32
segment mean alone leaves 4e-5 in bins 0 and 1); a pure tone halfway between two bins plus noise at 1e-3 of its amplitude
(the leak shape at the row maximum; its floor is below float32 resolution of the line, which the bound relative to the
row maximum does not ask for)."""
import functools

import numpy as np
import scipy.signal as sps

TOL = 1e-5
ENERGY_RTOL = 1e-6

# id -> (nx, ns, chunk, nperseg, noverlap or None for SciPy's nperseg // 2)
CASES = {
    "one_exact_segment": (3, 1024, 1024, 1024, None),       # a single segment that fills the chunk
    "tail_ignored": (3, 1535, 1535, 1024, None),            # still one segment; the rest is dropped
    "reference_case": (3, 7000, 3000, 1024, None),          # two chunks of four segments; 1000 samples left over
    "odd_sizes": (3, 7001, 3001, 256, 100),                 # unaligned chunk starts, 18 segments per chunk (two groups)
    "non_power_of_two": (3, 1700, 1700, 400, 0),            # 400 = 4 x 10 x 10, no overlap
    "small_transform": (3, 200, 64, 16, None),              # the smallest accepted transform
    # every other path of the kernel
    "prime_radix": (3, 905, 450, 112, 30),                  # 112 = 8 x 2 x 7: the loop-free prime stage
    "two_groups_1024": (3, 6144, 6144, 1024, None),         # 11 segments: a group of 8 and an odd one of 3
    "largest_transform": (3, 8200, 8200, 4096, None),       # 3 segments, one pair per group, > 64 KiB of LDS
}
# the reference's row length with enough rows for more than one wave of workgroups (GPU file only)
GPU_CASES = dict(CASES, rows_64x12000=(64, 12000, 3000, 1024, None))

# id -> (ns, chunk or None for the whole record)
ENERGY_CASES = {
    "partial_last_chunk": (7001, 3000),                     # 3 chunks, the last of 1001 samples
    "whole_record": (7001, None),
    "exact_chunks": (6000, 3000),
    "short_chunks": (200, 64),
}


def noverlap_of(nperseg, noverlap):
    return nperseg // 2 if noverlap is None else noverlap


@functools.lru_cache(maxsize=None)
def make_input(name):
    """float32 [nx, ns], read-only."""
    nx, ns, _, nperseg, _ = GPU_CASES[name]
    rng = np.random.default_rng(sorted(GPU_CASES).index(name) + 20)
    x = rng.standard_normal((nx, ns))
    t = np.arange(ns)
    for r in range(nx):
        if r % 3 == 1:
            x[r] += 1000.0 * np.sqrt(np.mean(x[r] ** 2))
        elif r % 3 == 2:
            k0 = max(2, nperseg // 8) + r // 3
            x[r] = np.sin(2.0 * np.pi * (k0 + 0.5) / nperseg * t + 0.3 * r) + 1e-3 * x[r]
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(name, fs=200.0):
    """float64 [nx, ns // chunk, nperseg // 2 + 1] and the segment count of a chunk."""
    nx, ns, chunk, nperseg, noverlap = GPU_CASES[name]
    nov = noverlap_of(nperseg, noverlap)
    x = make_input(name).astype(np.float64)
    nchunks = ns // chunk
    ref = np.empty((nx, nchunks, nperseg // 2 + 1))
    for j in range(nchunks):
        ref[:, j] = sps.welch(x[:, j * chunk:(j + 1) * chunk], fs=fs, nperseg=nperseg, noverlap=nov, axis=-1)[1]
    nseg = sps.spectrogram(x[0, :chunk], fs=fs, nperseg=nperseg, noverlap=nov)[1].size      # SciPy's own segment count
    ref.setflags(write=False)
    return ref, nseg


def check_rows(p, ref, what=""):
    """Every row within TOL of its own maximum; prints the worst figure before it asserts."""
    p = np.asarray(p, dtype=np.float64)
    assert p.shape == ref.shape, (what, p.shape, ref.shape)
    nx = ref.shape[0]
    err = np.abs(p - ref).reshape(nx, -1).max(axis=1) / ref.reshape(nx, -1).max(axis=1)
    print("welch %s: max row error / row maximum = %.3e (rows %s)" % (what, err.max(), np.array2string(err[:3], precision=2)))
    assert np.all(np.isfinite(p)), what
    assert err.max() <= TOL, (what, err)


@functools.lru_cache(maxsize=None)
def energy_input(name):
    ns, _ = ENERGY_CASES[name]
    rng = np.random.default_rng(sorted(ENERGY_CASES).index(name) + 70)
    x = rng.standard_normal((3, ns))
    x[1] += 1000.0 * np.sqrt(np.mean(x[1] ** 2))                      # an offset row
    x[2] *= np.linspace(0.01, 3.0, ns)
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


def energy_reference(name):
    ns, chunk = ENERGY_CASES[name]
    x = energy_input(name).astype(np.float64)
    return np.add.reduceat(x * x, np.arange(0, ns, ns if chunk is None else chunk), axis=1)
