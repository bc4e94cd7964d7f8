"""Every rank of the distributed f-k filter on hardware against float64: the harness of tests/fk_dist_cases.py builds the
plans of ALL ranks of a world of 1-8 in this one process, runs their time / channel / inverse-time phases on the one GPU
a test box has, and plays the two all-to-all exchanges on the host.  What tests/test_fk_dist_gpu.py (world 1, rank 0) and the
one-thread-at-a-time emulator of tests/test_emu_fk_dist.py leave out: rank > 0 layouts of the packed send buffer, slabs
narrower than the half spectrum, ranks without a sub-row, the row-chunked entry points and their statistics epilogue,
D4W_FKD_BT_CHUNK / D4W_FKD_BZ_CHUNK and the live-column list, C1 > 1 in the generic channel phase -- with real barriers,
in-place passes, persistent grids and float64 atomics.  All results against oracle.d4w_oracle.fk_filter_filt on float64
inputs: max|y - ref| / max|ref| < 1e-5; every case prints its worst ratio ("fkd ratio <family> ...")."""
import functools

import numpy as np
import pytest

from oracle import d4w_oracle as orc
from tests import fk_dist_cases as fc

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def be():
    return fc.GpuBackend()


@functools.lru_cache(maxsize=None)
def case(nx, ns, seed, kind="dense", taper=False):
    """(x, mask, float64 reference) of a case, computed once and left unchanged."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nx, ns))
    m = rng.uniform(0, 1, (nx, ns))
    if kind == "dead":
        m = fc.dead_rows(m)
    ref = orc.fk_filter_filt(x, m, tapering=taper)
    for a in (x, m, ref):
        a.setflags(write=False)
    return x, m, ref


def check(family, label, y, ref, tol=TOL):
    r = fc.rel(y, ref)
    print("fkd ratio %s %s %.3e" % (family, label, r))
    assert r < tol, (family, label, r)
    return r


def recording_setter(be, m, seen):
    """Sets the dense mask on every rank and records d4w_fkd_plan_live_columns of each."""
    mbuf = fc.upload(be, m)

    def setter(rk):
        fc.set_dense(be, rk, mbuf)
        seen.append(fc.live_columns(be, rk))
    return setter


# ---- packed plan -----------------------------------------------------------------------------------------------------------
def packed_nq(nx, ns, world):
    if (nx, ns) == (100, 600):                               # N1 = 5: classes {0}, {1, 4}, {2, 3} dealt to the least loaded rank
        return {1: [5], 2: [3, 2], 3: [1, 2, 2], 5: [1, 2, 2, 0, 0]}[world]
    return [2] if world == 1 else [1, 1] + [0] * (world - 2)                  # N1 = 2


@pytest.mark.parametrize("nx,ns", [(18, 48), (8, 480), (100, 600), (154, 48), (1102, 48)])
@pytest.mark.parametrize("world", [1, 2, 3, 5])
def test_packed_every_rank(be, nx, ns, world):
    """Shapes with built-in specialised kernels (154 x 48: radices 7 and 11, 1102 x 48: 19 and 29): per-destination qoff / qpitch
    layouts, ranks owning 0, 1, 2 or 3 sub-rows, uneven channel blocks; a dense mask, then the mask with dead wavenumber rows
    (pruned per rank) and the taper.  Both time phases also in 1, 2 and 3 row chunks, bit for bit, with the row statistics."""
    seed = nx * 7 + ns + world
    expect = {"nq": packed_nq(nx, ns, world)}
    x, m, ref = case(nx, ns, seed)
    check("packed", "%dx%d world %d dense" % (nx, ns, world), fc.fk_sharded_packed(be, x, m, world, expect=expect), ref)
    x, m, ref = case(nx, ns, seed, "dead", True)
    check("packed", "%dx%d world %d dead rows + taper" % (nx, ns, world), fc.fk_sharded_packed(be, x, m, world, taper=True, expect=expect), ref)


def test_packed_identity_and_zero_masks(be):
    nx, ns, world = 100, 600, 3
    x = case(nx, ns, 5)[0]
    check("packed", "100x600 world 3 all-ones mask", fc.fk_sharded_packed(be, x, np.ones((nx, ns)), world), x)
    assert not fc.fk_sharded_packed(be, x, np.zeros((nx, ns)), world).any()                 # exact zeros


# ---- generic plan ----------------------------------------------------------------------------------------------------------
PLAIN = [
    (40, 480, 1, {}),
    (40, 480, 3, {"nq": [4, 4, 4]}),
    (30, 360, 4, {"blocks": [8, 8, 7, 7]}),
    (24, 96, 8, {"N2": 1, "nq": [7, 6, 6, 6, 6, 6, 5, 6]}),
    (2 * 19, 2 * 7 * 11 * 3 * 2, 3, {}),                      # 38 x 924: loop-based prime radices on both axes
    (2048, 24, 3, {"C1": 2, "C2": 1024}),                    # C1 > 1 in the channel phase
    (1536, 40, 3, {"C1": 2, "C2": 768, "nq": [7, 6, 7]}),
]


@pytest.mark.parametrize("nx,ns,world,expect", PLAIN, ids=["%dx%d-w%d" % c[:3] for c in PLAIN])
def test_generic_plain_radices(be, nx, ns, world, expect):
    x, m, ref = case(nx, ns, nx + ns + world)
    seen = []
    y = fc.fk_sharded(be, x, None, world, setter=recording_setter(be, m, seen), expect=expect)
    check("generic", "%dx%d world %d" % (nx, ns, world), y, ref)
    assert all(s == (0, 0) for s in seen), seen              # not the Bluestein channel phase


def test_generic_plan_of_a_specialised_shape(be, monkeypatch):
    """100 x 600 forced onto the generic plan (D4W_FKD_GENERIC is read at every plan build): the oracle's filter, and the
    packed plan's result to the rounding the project allows between its packed and single-device paths."""
    nx, ns, world = 100, 600, 3
    x, m, ref = case(nx, ns, nx * 7 + ns + world)
    y_packed = fc.fk_sharded_packed(be, x, m, world, nchunks=(1,))
    monkeypatch.setenv("D4W_FKD_GENERIC", "1")
    y = fc.fk_sharded(be, x, m, world)
    monkeypatch.delenv("D4W_FKD_GENERIC")
    check("generic", "100x600 world 3 forced generic", y, ref)
    d = float(np.max(np.abs(y.astype(np.float64) - y_packed)) / np.max(np.abs(ref)))
    print("generic vs packed 100x600 world 3: %.3e" % d)
    assert d < 3e-6


BZ = [(37, 48, 1, 0, {}), (37, 48, 2, 0, {}), (74, 120, 3, 0, {}), (2 * 43, 96, 2, 16, {}), (131, 40, 1, 5, {}), (211, 24, 4, 0, {}),
      (2062, 24, 2, 0, {"C1": 5, "C2": 1000})]


@pytest.mark.parametrize("nx,ns,world,chunk,expect", BZ, ids=["%dx%d-w%d-chunk%d" % c[:4] for c in BZ])
def test_generic_channel_bluestein(be, nx, ns, world, chunk, expect, monkeypatch):
    """A channel count with a prime factor > 31: the slab's channel transform as a Bluestein convolution in global memory
    (fkd_bz_*), D4W_FKD_BZ_CHUNK pinning a chunk of slab columns narrower than the slab with a ragged last one; 2062 x 24
    with C1 = 5 in the padded length's passes."""
    if chunk:
        monkeypatch.setenv("D4W_FKD_BZ_CHUNK", str(chunk))
    x, m, ref = case(nx, ns, nx + world)
    seen = []
    y = fc.fk_sharded(be, x, None, world, setter=recording_setter(be, m, seen), expect=expect)
    label = "%dx%d world %d chunk %d" % (nx, ns, world, chunk)
    check("bz", label, y, ref)
    assert sum(b for _, b in seen) == ns // 2 and all(a == b for a, b in seen), seen        # Bluestein form, dense mask: all live
    if world == 2:
        check("bz", label + " taper", fc.fk_sharded(be, x, m, world, taper=True), case(nx, ns, nx + world, "dense", True)[2])
        check("bz", label + " all-ones mask", fc.fk_sharded(be, x, np.ones((nx, ns)), world), x)


@pytest.mark.parametrize("nx,ns,world,chunk", [(37, 96, 1, 7), (74, 120, 2, 0), (131, 80, 1, 5)])
def test_generic_channel_bluestein_live_columns(be, nx, ns, world, chunk, monkeypatch):
    """Band masks on the Bluestein channel phase: only the slab columns with a non-zero folded gain (or whose Hermitian partner
    column has one) go through the scratch (bz_cols), a chunk narrower than the live set; an all-zero mask gives zeros."""
    if chunk:
        monkeypatch.setenv("D4W_FKD_BZ_CHUNK", str(chunk))
    rng = np.random.default_rng(nx * 7 + world)
    x = rng.standard_normal((nx, ns))
    for i, m in enumerate(fc.band_masks(rng, nx, ns)):
        seen = []
        y = fc.fk_sharded(be, x, None, world, setter=recording_setter(be, m, seen))
        check("bz", "%dx%d world %d chunk %d band %d" % (nx, ns, world, chunk, i), y, orc.fk_filter_filt(x, m))
        live, total = sum(a for a, _ in seen), sum(b for _, b in seen)
        assert total == ns // 2 and 0 < live < 0.8 * total, seen
    assert not fc.fk_sharded(be, x, np.zeros((nx, ns)), world).any()


@pytest.mark.parametrize("bt_chunk", [0, 3])
@pytest.mark.parametrize("nx,ns,world", [(12, 74, 1), (10, 2 * 41 * 3, 2), (37, 2 * 43, 3)])
def test_generic_time_bluestein(be, nx, ns, world, bt_chunk, monkeypatch):
    """ns / 2 with a prime factor > 31: the local rows' time transform in the global-memory Bluestein form (fkd_bt_*), N1 = 1
    and rank 0 alone in the channel phase.  D4W_FKD_BT_CHUNK=3 rows per pass through the scratch: 12 rows in 4 chunks,
    blocks of 5 rows in 2 chunks with a ragged second one, blocks of 13, 12 and 12 rows with a ragged last chunk on rank 0."""
    if bt_chunk:
        monkeypatch.setenv("D4W_FKD_BT_CHUNK", str(bt_chunk))
    expect = {"N1": 1, "nq": [1] + [0] * (world - 1)}
    for taper in (False, True):
        x, m, ref = case(nx, ns, ns + world, "dense", taper)
        y = fc.fk_sharded(be, x, m, world, taper=taper, expect=expect)
        check("bt", "%dx%d world %d chunk %d%s" % (nx, ns, world, bt_chunk, " taper" if taper else ""), y, ref)


@pytest.mark.parametrize("world", [1, 3])
def test_generic_design_straight_into_the_plans(be, world):
    """d4w_fkd_set_mask_design_f32 == designing the dense mask (d4w_design_mask_f32) and folding it, bit for bit."""
    nx, ns = 40, 480
    x = np.random.default_rng(3).standard_normal((nx, ns))
    dense = fc.design_dense(be, nx, ns)
    y_design = fc.fk_sharded(be, x, None, world, setter=fc.design_setter(be))
    y_dense = fc.fk_sharded(be, x, dense, world)
    assert np.array_equal(y_design, y_dense)
    check("generic", "40x480 world %d closed-form design" % world, y_design, orc.fk_filter_filt(x, dense.astype(np.float64)))


def test_run_time_compiled_shape(be):
    """96 x 480 with kernels compiled at run time (the build step leaves them cached): whichever protocol the plan reports."""
    import ctypes

    import das4whales_amd as dw
    nx, ns, world = 96, 480, 3
    assert dw.dsp.compile_fk_shape(nx, ns)
    h = ctypes.c_void_p()
    assert be.lib.d4w_fkd_plan_create(nx, ns, world, 0, ctypes.byref(h)) == 0
    packed = be.lib.d4w_fkd_plan_is_packed(h)
    be.lib.d4w_fkd_plan_destroy(h)
    print("96 x 480 world 3: %s plan" % ("packed" if packed else "generic"))
    x, m, ref = case(nx, ns, 96)
    y = (fc.fk_sharded_packed if packed else fc.fk_sharded)(be, x, m, world)
    check("packed" if packed else "generic", "96x480 world 3 run-time compiled", y, ref)
