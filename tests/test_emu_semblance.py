"""Local slant-stack semblance (csrc/semblance.hip) in the CPU emulator build through the C ABI, against the float64 restatement
of tests/known_answers_semblance.py: the cases of tests/semblance_cases.py, which tests/test_semblance_gpu.py runs on the
hardware.  Kernel logic only, host pointers."""
import ctypes

import numpy as np
import pytest

from tests import known_answers_semblance as ks
from tests import semblance_cases as sc
from tests.emu_util import load_emu, vp


@pytest.fixture(scope="module")
def lib():
    return load_emu()


@pytest.fixture(scope="module")
def tile(lib):
    tc, ts = ctypes.c_int(), ctypes.c_int()
    assert lib.d4w_semblance_tile(ctypes.byref(tc), ctypes.byref(ts)) == 0
    return tc.value, ts.value


def call(lib, buf, ns, k, f, w, H, return_all, want_rc=0):
    nx, pitch = buf.shape
    npj, n = k.shape
    coh = np.full((nx, ns), np.nan, dtype=np.float32)
    idx = np.full((nx, ns), 255, dtype=np.uint8)
    cube = np.full((npj, nx, ns), np.nan, dtype=np.float32) if return_all else None
    rc = lib.d4w_semblance_f32(vp(buf), ctypes.c_int64(pitch), nx, ns, vp(np.ascontiguousarray(k, dtype=np.int32)),
                               vp(np.ascontiguousarray(f, dtype=np.float32)), npj, (n - 1) // 2, vp(np.ascontiguousarray(w, dtype=np.float32)),
                               H, vp(coh), vp(idx), vp(cube) if return_all else None, None)
    assert rc == want_rc, lib.d4w_last_error()
    return coh, idx, cube


def runner(lib):
    def run(buf, ns, delays, H, w, return_all):
        k, f = ks.split_delays(delays)
        return call(lib, np.ascontiguousarray(buf, dtype=np.float32), ns, k, f, w, H, return_all)
    return run


def test_limits_and_case_list(lib, tile):
    v = [ctypes.c_int() for _ in range(4)]
    assert lib.d4w_semblance_limits(*[ctypes.byref(c) for c in v]) == 0
    assert v[0].value >= sc.MAX_M and v[1].value >= sc.MAX_NP and v[2].value >= sc.MAX_H and v[3].value >= sc.MAX_DELAY
    assert tile[0] >= 1 and tile[1] >= 1
    cases = sc.parity_cases()
    assert 35 <= len(cases) <= 45 and cases[0][:5] == ("tc+1", "2ts+5", 16, 64, 64)
    for axis, values in enumerate((sc.NX_FORMS, sc.NS_FORMS, sc.MS, sc.HS, sc.NPS, sc.INPUTS)):
        assert {c[axis] for c in cases} == set(values)
    k, f = ks.split_delays(np.concatenate([sc.delays_table(8, M) for M in sc.MS for _ in (0,)], axis=None).reshape(1, -1))
    d = k + f.astype(np.float64)
    assert d.max() == sc.MAX_DELAY and d.min() == -sc.MAX_DELAY and (k == 0).any()
    assert ((f > 0) & (f < 0.01)).any() and (f > 0.99).any() and np.all(f < 1)
    kc, fc = ks.split_delays(np.array([[-1e-9, 0.0, 1.0 - 1e-9]]))                  # fractions that round to 1.0f are carried
    assert kc.tolist() == [[0, 0, 1]] and not fc.any()


@pytest.mark.parametrize("case", sc.parity_cases(), ids=sc.case_id)
def test_parity(lib, tile, case):
    sc.check_parity(runner(lib), case, tile)


def test_plane_wave_is_exactly_one(lib, tile):
    sc.check_plane_wave(runner(lib), tile)


def test_single_channel(lib, tile):
    sc.check_single_channel(runner(lib), tile)


def test_zeros(lib, tile):
    sc.check_zeros(runner(lib), tile)


def test_scaling_and_repeat_are_bit_identical(lib, tile):
    sc.check_scaling_and_repeat(runner(lib), tile)


def test_weightless_neighbour_is_not_read(lib, tile):
    """A channel of NaNs that its neighbours see only under weight 0 (a dead channel masked out) changes none of their results.
    Its own row is unspecified: there the NaNs sit under the centre weight."""
    M, H = 1, 2
    x = np.random.default_rng(6).standard_normal((3, 50)).astype(np.float32)
    w = np.array([0.0, 1.0, 1.0], dtype=np.float32)
    k, f = ks.split_delays(sc.delays_table(3, M, 0))
    ref = call(lib, x, 50, k, f, w, H, True)
    y = x.copy()
    y[0] = np.nan                                       # channel 0 is neighbour m = -1 of channel 1 only: weight 0
    got = call(lib, y, 50, k, f, w, H, True)
    assert np.array_equal(got[0][1:], ref[0][1:]) and np.array_equal(got[1][1:], ref[1][1:]) and np.array_equal(got[2][:, 1:], ref[2][:, 1:])


def test_bad_arguments(lib):
    M, H, npj, nx, ns = 2, 3, 4, 3, 40
    x = np.ones((nx, ns), dtype=np.float32)
    k0, f0 = ks.split_delays(sc.delays_table(npj, M, 0))
    w0 = np.ones(2 * M + 1, dtype=np.float32)
    coh, idx = np.zeros((nx, ns), dtype=np.float32), np.zeros((nx, ns), dtype=np.uint8)

    def go(x=x, pitch=ns, nx=nx, ns=ns, k=k0, f=f0, npj=npj, M=M, w=w0, H=H, coh=coh, idx=idx):
        p = lambda a: vp(a) if a is not None else None
        return lib.d4w_semblance_f32(p(x), ctypes.c_int64(pitch), nx, ns, p(k), p(f), npj, M, p(w), H, p(coh), p(idx), None, None)

    def edit(a, at, v):
        b = a.copy()
        b[at] = v
        return b
    assert go() == 0
    big = np.zeros((sc.MAX_NP + 1, 2 * M + 1))
    for kw in (dict(x=None), dict(k=None), dict(f=None), dict(w=None), dict(coh=None), dict(idx=None), dict(nx=0), dict(ns=0), dict(pitch=ns - 1),
               dict(M=0), dict(M=sc.MAX_M + 1), dict(npj=0), dict(npj=sc.MAX_NP + 1, k=big.astype(np.int32), f=big.astype(np.float32)),
               dict(H=-1), dict(H=sc.MAX_H + 1), dict(k=edit(k0, (1, 0), sc.MAX_DELAY + 1)), dict(k=edit(k0, (1, 0), -sc.MAX_DELAY - 1)),
               dict(k=edit(k0, (1, 0), sc.MAX_DELAY), f=edit(f0, (1, 0), 0.5)), dict(f=edit(f0, (1, 0), 1.0)), dict(f=edit(f0, (1, 0), -0.25)),
               dict(f=edit(f0, (1, 0), np.nan)), dict(k=edit(k0, (2, M), 1)), dict(f=edit(f0, (2, M), 0.5)), dict(w=edit(w0, 0, -1.0)),
               dict(w=edit(w0, 1, np.nan)), dict(w=edit(w0, 1, np.inf)), dict(w=edit(w0, M, 0.0))):
        assert go(**kw) == -1, kw
        assert len(lib.d4w_last_error()) > 0
