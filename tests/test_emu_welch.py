"""Welch PSD and chunk energy LOGIC (csrc/welch.hip) on the CPU emulator build: same HIP source, same C ABI, host
pointers, against scipy.signal.welch in float64 on the float32-rounded input (cases and tolerance: tests/welch_cases.py)."""
import ctypes

import numpy as np
import pytest

from tests import welch_cases as wc
from tests.emu_util import load_emu, vp

FS = 200.0


@pytest.fixture(scope="module")
def emu():
    return load_emu()


def welch(lib, x, chunk, nperseg, noverlap, fs=FS):
    nx, ns = x.shape
    pxx = np.full((nx, ns // chunk, lib.d4w_welch_bins(nperseg)), np.nan, dtype=np.float32)
    rc = lib.d4w_welch_f32(vp(x), nx, ns, chunk, nperseg, noverlap, ctypes.c_double(fs), vp(pxx), None)
    assert rc == 0, lib.d4w_last_error()
    return pxx


@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_welch_matches_scipy(emu, name):
    nx, ns, chunk, nperseg, noverlap = wc.CASES[name]
    nov = wc.noverlap_of(nperseg, noverlap)
    ref, nseg = wc.reference(name, FS)
    assert emu.d4w_welch_supported(nperseg) == 1
    assert emu.d4w_welch_bins(nperseg) == nperseg // 2 + 1 == ref.shape[2]
    assert emu.d4w_welch_segments(chunk, nperseg, nov) == nseg
    wc.check_rows(welch(emu, wc.make_input(name), chunk, nperseg, nov), ref, name)


def test_welch_unaligned_base(emu):
    """The block itself starts 4, 8 and 12 bytes into a 16-byte slot: every place of the scalar prologue."""
    name = "reference_case"
    nx, ns, chunk, nperseg, _ = wc.CASES[name]
    ref, _ = wc.reference(name, FS)
    buf = np.zeros(nx * ns + 4, dtype=np.float32)
    for shift in (1, 2, 3):
        x = buf[shift:shift + nx * ns].reshape(nx, ns)
        x[:] = wc.make_input(name)
        wc.check_rows(welch(emu, x, chunk, nperseg, nperseg // 2), ref, "%s + %d floats" % (name, shift))


def test_welch_segments():
    lib = load_emu()
    assert lib.d4w_welch_segments(3000, 1024, 512) == 4
    assert lib.d4w_welch_segments(3001, 256, 100) == 18
    assert lib.d4w_welch_segments(1024, 1024, 512) == 1
    assert lib.d4w_welch_segments(1023, 1024, 512) == 0            # n < nperseg
    assert lib.d4w_welch_segments(1700, 400, 0) == 4
    assert [lib.d4w_welch_supported(n) for n in (16, 400, 4096, 2 * 31, 8, 4098, 17, 2 * 37, 1025)] == [1, 1, 1, 1, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("name", sorted(wc.ENERGY_CASES))
def test_chunk_energy(emu, name):
    ns, chunk = wc.ENERGY_CASES[name]
    x = wc.energy_input(name)
    ref = wc.energy_reference(name)
    e = np.full(ref.shape, np.nan, dtype=np.float32)
    rc = emu.d4w_chunk_energy_f32(vp(x), x.shape[0], ns, ns if chunk is None else chunk, vp(e), None)
    assert rc == 0, emu.d4w_last_error()
    print("energy %s: max relative error %.3e" % (name, np.max(np.abs(e - ref) / ref)))
    np.testing.assert_allclose(e, ref, rtol=wc.ENERGY_RTOL, atol=0.0)


@pytest.mark.parametrize("what,ns,chunk,nperseg,noverlap", [
    ("odd nperseg", 4000, 3000, 1023, 511),
    ("nperseg 8", 4000, 3000, 8, 4),
    ("nperseg 4098", 9000, 9000, 4098, 2049),
    ("prime factor 37", 4000, 3000, 2 * 37, 37),
    ("noverlap = nperseg", 4000, 3000, 1024, 1024),
    ("noverlap > nperseg", 4000, 3000, 1024, 2000),
    ("negative noverlap", 4000, 3000, 1024, -1),
    ("chunk < nperseg", 4000, 1000, 1024, 512),
    ("chunk > ns", 4000, 4001, 1024, 512),
])
def test_welch_argument_errors(emu, what, ns, chunk, nperseg, noverlap):
    x = np.zeros((2, ns), dtype=np.float32)
    pxx = np.zeros((2, max(1, ns // chunk), abs(nperseg) // 2 + 1), dtype=np.float32)
    rc = emu.d4w_welch_f32(vp(x), 2, ns, chunk, nperseg, noverlap, ctypes.c_double(FS), vp(pxx), None)
    assert rc == -1, what                                          # D4W_EINVAL
    assert len(emu.d4w_last_error()) > 0
    assert not pxx.any()


def test_chunk_energy_argument_errors(emu):
    x = np.zeros((2, 100), dtype=np.float32)
    e = np.zeros((2, 4), dtype=np.float32)
    for chunk in (0, -3, 101):
        assert emu.d4w_chunk_energy_f32(vp(x), 2, 100, chunk, vp(e), None) == -1
        assert len(emu.d4w_last_error()) > 0
