"""The cases of the local slant-stack semblance that tests/test_emu_semblance.py (CPU emulator, C ABI) and
tests/test_semblance_gpu.py (hardware, dw.detect.local_semblance) both run.  A runner is
    run(buf, ns, delays, H, weights, return_all) -> (coh float32 [nx, ns], idx uint8 [nx, ns], cube float32 [np, nx, ns] or None)
where buf is float32 [nx, pitch >= ns] and the record is buf[:, :ns] (pitch > ns: the rows are read in place)."""
import functools

import numpy as np

from tests import known_answers_semblance as ks

MAX_M, MAX_NP, MAX_H, MAX_DELAY = 16, 64, 64, 64            # the minima the issue sets; the library's limits are checked against them
NX_FORMS = ("1", "2", "M", "2M+1", "tc+1")
NS_FORMS = ("1", "63", "ts+1", "2ts+5")
MS, HS, NPS = (1, 3, 16), (0, 4, 64), (1, 6, 64)
INPUTS = ("noise", "spike", "dead", "zero_w", "pitch")


def delays_table(npj, M, rot=0, max_delay=MAX_DELAY):
    """float64 [np, 2M + 1] from slopes in samples per channel: 0, exact integers, fractions near 0 and near 1, one that rounds
    to 1.0f (carried), and the slopes that reach +-max_delay at the aperture's ends."""
    top = max_delay / M
    special = [0.0, 1.0, -2.0, 1e-3, -(1.0 - 1e-3), top, -1e-9, -top]
    if npj <= len(special):
        slopes = [special[(rot + q) % len(special)] for q in range(npj)]
    else:
        slopes = special + list(np.linspace(-top, top, npj - len(special)))
    m = np.arange(-M, M + 1, dtype=np.float64)
    return np.clip(np.asarray(slopes, dtype=np.float64)[:, None] * m[None, :], -max_delay, max_delay)


def _dim(form, M, tile):
    return {"1": 1, "2": 2, "M": M, "2M+1": 2 * M + 1, "tc+1": tile[0] + 1, "63": 63, "ts+1": tile[1] + 1, "2ts+5": 2 * tile[1] + 5}[form]


def parity_cases():
    """About 40 (nx form, ns form, M, H, np, input, rot): every value of every axis, and the all-maximum corner first."""
    cases = [("tc+1", "2ts+5", 16, 64, 64, "noise", 5)]
    i = 0
    for inp in INPUTS:
        for q in range(8):
            npj = NPS[(i + i // 3) % 3]
            nsf = NS_FORMS[(i + i // 4) % 4]
            if npj == 64 and nsf == "2ts+5":                 # the corner above has that pair; keep the rest quick
                nsf = "63"
            cases.append((NX_FORMS[i % 5], nsf, MS[i % 3], HS[(i // 3) % 3], npj, inp, i))
            i += 1
    return cases


def case_id(c):
    return "nx%s-ns%s-M%d-H%d-np%d-%s" % c[:6]


def make_case(case, tile):
    nxf, nsf, M, H, npj, inp, rot = case
    nx, ns = _dim(nxf, M, tile), _dim(nsf, M, tile)
    rng = np.random.default_rng(1000 + rot)
    pitch = ns + 3 if inp == "pitch" else ns
    buf = rng.standard_normal((nx, pitch)).astype(np.float32)
    w = np.ones(2 * M + 1, dtype=np.float32)
    if inp == "spike":
        buf[nx // 2, min(ns - 1, 5)] = 1e4                   # next to unit noise: a float32 prefix difference loses the windows behind it
    elif inp == "dead":
        buf[min(nx - 1, 1), :] = 0.0                         # inside the aperture of its neighbours
    elif inp == "zero_w":
        w = rng.uniform(0.5, 2.0, 2 * M + 1).astype(np.float32)
        w[0] = 0.0
        if M > 1:
            w[M + 2] = 0.0
    return buf, ns, delays_table(npj, M, rot), H, w


@functools.lru_cache(maxsize=None)
def reference(case, tile):
    """The case and its float64 answer, computed once for every test that needs it (left unchanged by all of them)."""
    buf, ns, delays, H, w = make_case(case, tile)
    k, f = ks.split_delays(delays)
    S, R = ks.semblance_ref(buf[:, :ns], k, f, w, H)
    for a in (buf, delays, w, S, R):
        a.setflags(write=False)
    return buf, ns, delays, H, w, S, R


def check_parity(run, case, tile):
    buf, ns, delays, H, w, S, R = reference(case, tile)
    coh, idx, cube = run(buf, ns, delays, H, w, True)
    worst = ks.check_against_ref(coh, idx, cube, S, R, case[2], H)
    print("%s: worst cube error / tolerance = %.3g" % (case_id(case), worst))
    coh2, idx2, none = run(buf, ns, delays, H, w, False)     # without the cube: the same bits
    assert none is None and np.array_equal(coh, coh2) and np.array_equal(idx, idx2)


# ---- exact known answers ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plane_wave(tile):
    """x[c, t] = g[t - c], g on a 2^-6 grid: along 1 sample per channel every neighbour holds the same value, all sums are exact."""
    M, H = 3, 4
    nx, ns = tile[0] + 2, tile[1] + 20
    g = np.random.default_rng(3).integers(-8, 9, ns + nx).astype(np.float32) / 64.0
    x = np.stack([g[nx - c:nx - c + ns] for c in range(nx)])
    m = np.arange(-M, M + 1, dtype=np.float64)
    delays = np.asarray([-1.0, 0.0, 0.5, 1.0, 2.0])[:, None] * m[None, :]
    return x, delays, M, H, 3


def check_plane_wave(run, tile):
    x, delays, M, H, want = plane_wave(tile)
    ns = x.shape[1]
    coh, idx, _ = run(x, ns, delays, H, np.ones(2 * M + 1, dtype=np.float32), False)
    inner = slice(H + M + 1, ns - (H + M + 1))
    assert np.all(coh[:, inner] == np.float32(1.0)) and np.all(idx[:, inner] == want)          # every channel, the edge ones included


def check_single_channel(run, tile):
    M, H = 3, 4
    ns = tile[1] + 30
    x = np.random.default_rng(4).standard_normal((1, ns)).astype(np.float32)
    x[0, 100:140] = 0.0                                      # longer than the window: some windows hold nothing
    x[0, :12] = 0.0
    coh, idx, _ = run(x, ns, delays_table(6, M, 0), H, np.ones(2 * M + 1, dtype=np.float32), False)
    nz = np.convolve((x[0] != 0).astype(np.float64), np.ones(2 * H + 1), mode="same") > 0
    assert np.all(coh[0, nz] == np.float32(1.0)) and np.all(coh[0, ~nz] == 0) and (~nz).sum() >= 30
    assert np.all(idx == 0)                                  # every trial gives the same: the tie goes to the smallest


def check_zeros(run, tile):
    x = np.zeros((tile[0] + 1, 70), dtype=np.float32)
    coh, idx, cube = run(x, 70, delays_table(6, 3, 0), 4, np.ones(7, dtype=np.float32), True)
    assert not coh.any() and not idx.any() and not cube.any()


def check_scaling_and_repeat(run, tile):
    M, H = 3, 4
    nx, ns = tile[0] + 1, tile[1] + 1
    x = np.random.default_rng(5).standard_normal((nx, ns)).astype(np.float32)
    w = np.ones(2 * M + 1, dtype=np.float32)
    d = delays_table(6, M, 0)
    first = run(x, ns, d, H, w, True)
    for other in (run(x, ns, d, H, w, True), run(x * np.float32(2.0 ** 10), ns, d, H, w, True), run(x * np.float32(2.0 ** -10), ns, d, H, w, True)):
        for a, b in zip(first, other):
            assert a.dtype == b.dtype and np.array_equal(a, b)                                  # bit for bit
