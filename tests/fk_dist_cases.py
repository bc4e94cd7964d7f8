"""The multi-rank harness of the distributed f-k filter that tests/test_emu_fk_dist.py (CPU emulator) and
tests/test_fk_dist_ranks_gpu.py (hardware) both run: the per-rank C-ABI phases (d4w_fkd_time_fwd / chan_apply / time_inv and
their packed forms) of EVERY rank of a world in ONE process, on one device, the two all-to-all exchanges played by NumPy on the
host exactly as include/d4w.h describes them.  No process group, no second GPU.

A backend says where the buffers live:
    EmuBackend(lib)   NumPy arrays, host pointers, a NULL stream (the emulator build of tests/emu_util.py)
    GpuBackend()      torch CUDA tensors, data_ptr(), torch's current stream (das4whales_amd._lib)
Every buffer a kernel writes lies between two guards of GUARD elements holding a fixed bit pattern, inside the harness's own
allocation: a store past either end of the region handed to the library does not fault inside a caching allocator's block, it
corrupts silently -- the guards are how that shows.  Buffers a kernel must write completely start as NaN."""
import ctypes

import numpy as np

GUARD = 256
_PATTERN = {4: 0x5AC3A53C, 8: 0x5AC3A53C5AC3A53C}         # not a NaN, not a value any transform produces
_INT = {4: np.int32, 8: np.int64}


def rel(y, ref):
    return float(np.max(np.abs(np.asarray(y, dtype=np.float64) - ref)) / np.max(np.abs(ref)))


class _HostBuf:
    def __init__(self, n, dtype, guarded=True):
        g = GUARD if guarded else 0
        self.g, self.n = g, n
        self.raw = np.empty(n + 2 * g, dtype=dtype)
        self.raw.view(_INT[self.raw.itemsize])[...] = _PATTERN[self.raw.itemsize]
        self.a = self.raw[g:g + n]

    @property
    def ptr(self):
        return self.a.ctypes.data_as(ctypes.c_void_p)

    def get(self):
        return self.a.copy()

    def put(self, v):
        self.a[...] = np.asarray(v).reshape(-1)

    def fill(self, v):
        self.a[...] = v

    def guards_intact(self):
        i = self.raw.view(_INT[self.raw.itemsize])
        return bool(np.all(i[:self.g] == _PATTERN[self.raw.itemsize]) and np.all(i[self.g + self.n:] == _PATTERN[self.raw.itemsize]))


class EmuBackend:
    name = "emu"
    stream = None

    def __init__(self, lib):
        self.lib = lib
        cd, ci, cv = ctypes.c_double, ctypes.c_int, ctypes.c_void_p
        lib.d4w_design_mask_f32.argtypes = [ci, ci, ci, cd, cd, cv, ci, ci, cv, cv, cv]
        lib.d4w_fkd_set_mask_design_f32.argtypes = [cv, ci, cd, cd, cv, ci, ci, cv, cv]

    def ok(self, rc):
        assert rc == 0, self.lib.d4w_last_error()

    def alloc(self, n, dtype=np.float32, guarded=True):
        return _HostBuf(int(n), dtype, guarded)

    def sync(self):
        pass


class _DevBuf:
    def __init__(self, n, dtype, guarded=True):
        import torch
        self._torch = torch
        g = GUARD if guarded else 0
        self.g, self.n = g, n
        self.tdtype = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}[np.dtype(dtype)]
        self.idtype = {torch.float32: torch.int32, torch.float64: torch.int64}[self.tdtype]
        self.raw = torch.empty(n + 2 * g, dtype=self.tdtype, device="cuda")
        self.pattern = _PATTERN[self.raw.element_size()]
        self.raw.view(self.idtype).fill_(self.pattern)
        self.t = self.raw[g:g + n]

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def get(self):
        return self.t.cpu().numpy()

    def put(self, v):
        self.t.copy_(self._torch.from_numpy(np.ascontiguousarray(v).reshape(-1)))

    def fill(self, v):
        self.t.fill_(v)

    def guards_intact(self):
        i = self.raw.view(self.idtype)
        return bool((i[:self.g] == self.pattern).all().item() and (i[self.g + self.n:] == self.pattern).all().item())


class GpuBackend:
    name = "gpu"

    def __init__(self):
        import torch
        from das4whales_amd._lib import check, lib
        assert torch.cuda.is_available(), "GPU tests need a ROCm device"
        self._torch, self.lib, self.ok = torch, lib, check

    @property
    def stream(self):
        return ctypes.c_void_p(self._torch.cuda.current_stream().cuda_stream)

    def alloc(self, n, dtype=np.float32, guarded=True):
        return _DevBuf(int(n), dtype, guarded)

    def sync(self):
        self._torch.cuda.current_stream().synchronize()


def upload(be, a, dtype=np.float32):
    """A read-only input of the library (no guards: nothing writes it)."""
    a = np.ascontiguousarray(a, dtype=dtype)
    b = be.alloc(a.size, dtype, guarded=False)
    b.put(a)
    return b


def _intact(*bufs):
    assert all(b.guards_intact() for b in bufs), "a kernel wrote outside the region it was handed"


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(_INT[a.itemsize]), b.view(_INT[b.itemsize]))


class Rank:
    def __init__(self, lib, nx, ns, world, rank):
        self.lib = lib
        self.h = ctypes.c_void_p()
        assert lib.d4w_fkd_plan_create(nx, ns, world, rank, ctypes.byref(self.h)) == 0, lib.d4w_last_error()
        info = (ctypes.c_int * 12)()
        assert lib.d4w_fkd_plan_info(self.h, info) == 0
        (_, _, _, _, self.a, self.b, self.N1, self.N2, self.nq, self.C1, self.C2, _) = list(info)
        own = (ctypes.c_int * self.N1)()
        assert lib.d4w_fkd_plan_q1_owner(self.h, own) == 0
        self.owner = np.array(list(own))

    def close(self):
        self.lib.d4w_fkd_plan_destroy(self.h)


def _expect(ranks, expect):
    """Plan geometry a case pins (what makes it the case it is): nq and channel-block size per rank, N1, N2, C1, C2."""
    for key, want in (expect or {}).items():
        got = {"nq": [rk.nq for rk in ranks], "blocks": [rk.b - rk.a for rk in ranks]}.get(key) or getattr(ranks[0], key)
        assert got == want, (key, got, want)


def set_dense(be, rk, mbuf):
    be.ok(be.lib.d4w_fkd_set_mask_dense_f32(rk.h, mbuf.ptr, be.stream))


def fk_sharded(be, x, mask, world, taper=False, setter=None, expect=None):
    """The generic protocol: z_loc [nxl][N1][N2] complex per rank, sub-row q1 of every channel to rank owner[q1]."""
    lib = be.lib
    nx, ns = x.shape
    M = ns // 2
    ranks = [Rank(lib, nx, ns, world, r) for r in range(world)]
    try:
        assert all(lib.d4w_fkd_plan_is_packed(rk.h) == 0 for rk in ranks)
        N1, N2 = ranks[0].N1, ranks[0].N2
        owner = ranks[0].owner
        assert all(np.array_equal(rk.owner, owner) for rk in ranks)          # every rank derives the same map
        assert ranks[0].a == 0 and ranks[-1].b == nx and all(ranks[i].b == ranks[i + 1].a for i in range(world - 1))
        assert sorted(owner.tolist()) == sorted(sum(([r] * ranks[r].nq for r in range(world)), []))
        _expect(ranks, expect)
        mbuf = upload(be, mask) if mask is not None else None
        xf = np.ascontiguousarray(x, dtype=np.float32)
        z, zbuf, keep = [], [], []
        for rk in ranks:
            if setter is not None:
                setter(rk)
            else:
                set_dense(be, rk, mbuf)
            nxl = rk.b - rk.a
            xl = upload(be, xf[rk.a:rk.b])
            zb = be.alloc(nxl * N1 * N2 * 2)
            zb.fill(np.nan)
            be.ok(lib.d4w_fkd_time_fwd_f32(rk.h, xl.ptr, zb.ptr, int(taper), be.stream))
            zl = zb.get().reshape(nxl, N1, N2, 2)
            assert not np.isnan(zl).any()                                    # the whole half spectrum of every local row
            _intact(zb)
            z.append(zl)
            zbuf.append(zb)
            keep.append(xl)
        # all-to-all: sub-row q1 of every channel -> rank owner[q1]; receiver concatenates in rank order
        qidx = [np.nonzero(owner == s)[0] for s in range(world)]
        slabs = [np.ascontiguousarray(np.concatenate([z[r][:, qidx[s]] for r in range(world)], axis=0))
                 for s in range(world)]
        for s, rk in enumerate(ranks):
            assert slabs[s].shape == (nx, rk.nq, N2, 2)
            sb = be.alloc(slabs[s].size)
            sb.put(slabs[s])
            be.ok(lib.d4w_fkd_chan_apply_f32(rk.h, sb.ptr if rk.nq else None, be.stream))
            slabs[s] = sb.get().reshape(slabs[s].shape)
            assert np.isfinite(slabs[s]).all()
            _intact(sb)
        # all-to-all back
        y = np.empty((nx, ns), dtype=np.float32)
        for r, rk in enumerate(ranks):
            zl = z[r]
            for s in range(world):
                zl[:, qidx[s]] = slabs[s][rk.a:rk.b]
            zbuf[r].put(zl)
            be.ok(lib.d4w_fkd_time_inv_f32(rk.h, zbuf[r].ptr, be.stream))
            y[rk.a:rk.b] = zbuf[r].get().reshape(rk.b - rk.a, ns)
            _intact(zbuf[r])
        assert np.isfinite(y).all()
        assert M == N1 * N2
        be.sync()
        return y
    finally:
        be.sync()
        for rk in ranks:
            rk.close()


def chunk_ranges(nxl, C1, nch):
    """Local row ranges [l0, l1) of nch chunks of nxl rows, boundaries at multiples of C1 (the time-phase tile; a ragged last
    chunk where nxl % C1 != 0) -- the rule of das4whales_amd.shard.ShardedFkPlan._chunks."""
    grp = -(-nxl // C1)
    cut = [min(nxl, C1 * ((grp * j) // nch)) for j in range(nch)] + [nxl]
    return [(cut[j], cut[j + 1]) for j in range(nch)]


def fk_sharded_packed(be, x, mask, world, taper=False, nchunks=(1, 2, 3), expect=None):
    """The PACKED protocol of include/d4w.h (shapes with specialised kernels): the time phase writes the send buffer,
    destination rank major; the exchanges are plain concatenations -- no index packing anywhere.  Both time phases also run
    through their row-chunked entry points, in each of `nchunks` chunks per rank (fewer where a rank has fewer groups of C1
    rows, as ShardedFkPlan.exchange_chunks clamps it): a chunk leaves the rows behind it untouched -- their transfer may be in
    flight -- and the chunks together give the bits of the unchunked call; so does the pass with the row statistics."""
    lib = be.lib
    nx, ns = x.shape
    ranks = [Rank(lib, nx, ns, world, r) for r in range(world)]
    try:
        assert all(lib.d4w_fkd_plan_is_packed(rk.h) == 1 for rk in ranks)
        N1, N2 = ranks[0].N1, ranks[0].N2
        per = N2 * 2
        owner = ranks[0].owner
        assert all(np.array_equal(rk.owner, owner) for rk in ranks)
        nq = [int(np.sum(owner == s)) for s in range(world)]
        assert [rk.nq for rk in ranks] == nq
        _expect(ranks, expect)
        groups = min(-(-(rk.b - rk.a) // rk.C1) for rk in ranks)
        counts = sorted({max(1, min(int(n), groups)) for n in nchunks})
        mbuf = upload(be, mask)
        xf = np.ascontiguousarray(x, dtype=np.float32)

        def splits(r):                                       # all_to_all_single: rank r's block for s = elements [off[s], off[s+1])
            nxl = ranks[r].b - ranks[r].a
            return np.concatenate(([0], np.cumsum([nxl * nq[s] * per for s in range(world)])))

        def rows_done(r, flat, l1):
            """Of rank r's packed buffer: rows < l1 of every destination's block written, rows >= l1 still NaN."""
            off, nxl = splits(r), ranks[r].b - ranks[r].a
            for s in range(world):
                blk = flat[off[s]:off[s + 1]].reshape(nxl, nq[s] * per)
                if np.isnan(blk[:l1]).any() or not np.isnan(blk[l1:]).all():
                    return False
            return True

        send = []
        for r, rk in enumerate(ranks):
            set_dense(be, rk, mbuf)
            nxl = rk.b - rk.a
            xl = upload(be, xf[rk.a:rk.b])
            buf = be.alloc(nxl * N1 * per)
            buf.fill(np.nan)
            be.ok(lib.d4w_fkd_time_fwd_packed_f32(rk.h, xl.ptr, buf.ptr, int(taper), be.stream))
            whole = buf.get()
            assert not np.isnan(whole).any()
            _intact(buf)
            for nch in counts:
                buf.fill(np.nan)
                for l0, l1 in chunk_ranges(nxl, rk.C1, nch):
                    be.ok(lib.d4w_fkd_time_fwd_packed_rows_f32(rk.h, xl.ptr, buf.ptr, int(taper), l0, l1, be.stream))
                    assert rows_done(r, buf.get(), l1), (r, nch, l0, l1)
                assert _same_bits(buf.get(), whole), (r, nch)
                _intact(buf)
            send.append(whole)
        slabs = []
        for s, rk in enumerate(ranks):
            parts = [send[r][splits(r)[s]:splits(r)[s + 1]] for r in range(world)]
            slab = np.ascontiguousarray(np.concatenate(parts))
            assert slab.size == nx * nq[s] * per
            sb = be.alloc(slab.size)
            sb.put(slab)
            be.ok(lib.d4w_fkd_chan_apply_f32(rk.h, sb.ptr if nq[s] else None, be.stream))
            slabs.append(sb.get())
            assert np.isfinite(slabs[s]).all()
            _intact(sb)
        y = np.empty((nx, ns), dtype=np.float32)
        for r, rk in enumerate(ranks):
            nxl = rk.b - rk.a
            parts = [slabs[s][rk.a * nq[s] * per:rk.b * nq[s] * per] for s in range(world)]
            back = upload(be, np.concatenate(parts))
            yb = be.alloc(nxl * ns)
            yb.fill(np.nan)
            be.ok(lib.d4w_fkd_time_inv_packed_f32(rk.h, back.ptr, yb.ptr, be.stream))
            yl = yb.get().reshape(nxl, ns)
            assert not np.isnan(yl).any()
            _intact(yb)
            y[rk.a:rk.b] = yl
            mean, mx = be.alloc(nxl, np.float64), be.alloc(nxl, np.float32)      # float64 row means (include/d4w.h)
            for nch in counts:
                chunks = chunk_ranges(nxl, rk.C1, nch)
                yb.fill(np.nan)
                for l0, l1 in chunks:
                    be.ok(lib.d4w_fkd_time_inv_packed_rows_f32(rk.h, back.ptr, yb.ptr, l0, l1, be.stream))
                    part = yb.get().reshape(nxl, ns)
                    assert not np.isnan(part[:l1]).any() and np.isnan(part[l1:]).all(), (r, nch, l0, l1)
                assert _same_bits(yb.get().reshape(nxl, ns), yl), (r, nch)
                # the same pass with the row statistics in its epilogue (the caller zeroes them before the first chunk)
                yb.fill(np.nan)
                mean.fill(0.0)
                mx.fill(0.0)
                for l0, l1 in chunks:
                    be.ok(lib.d4w_fkd_time_inv_packed_rows_stats_f32(rk.h, back.ptr, yb.ptr, l0, l1, mean.ptr, mx.ptr, be.stream))
                assert _same_bits(yb.get().reshape(nxl, ns), yl), (r, nch)
                assert np.array_equal(mx.get(), np.abs(yl).max(axis=1)), (r, nch)         # an atomic max over float bits
                assert np.max(np.abs(mean.get() - yl.astype(np.float64).mean(axis=1))) < 1e-6 * max(np.abs(yl).max(), 1e-30)
                _intact(yb, mean, mx)
        be.sync()
        return y
    finally:
        be.sync()
        for rk in ranks:
            rk.close()


def dead_rows(m):
    """m with the wavenumber rows min(k, nx - k) > nx // 4 zeroed (fftshift-ed grid): pruned per rank."""
    nx = m.shape[0]
    ks = np.fft.fftshift(np.arange(nx))
    m = m.copy()
    m[np.minimum(ks, nx - ks) > nx // 4, :] = 0.0
    return m


def band_masks(rng, nx, ns):
    """Three masks that are zero outside a frequency band: symmetric bands, a band on the positive frequencies only, a band
    touching DC and Nyquist."""
    f = np.arange(-(ns // 2), ns - ns // 2) / (ns / 2.0)                      # the mask's fftshift-ed frequency grid
    for keep in ((np.abs(f) >= 0.15) & (np.abs(f) <= 0.35), (f >= 0.2) & (f <= 0.5), (np.abs(f) <= 0.1) | (np.abs(f) >= 0.9)):
        yield rng.uniform(0.1, 1, (nx, ns)) * keep[None, :]


def live_columns(be, rk):
    info = (ctypes.c_int * 2)()
    assert be.lib.d4w_fkd_plan_live_columns(rk.h, info) == 0
    return tuple(info)


DESIGN_P8 = (1400., 1450., 3400., 3500., 0., 0., 0., 0.)
DESIGN_STEP, DESIGN_FS = 2.0419046878814697, 200.0


def design_dense(be, nx, ns):
    """The classic fan of d4w_design_mask_f32 as a dense float32 [nx, ns] mask on the host."""
    p8 = (ctypes.c_double * 8)(*DESIGN_P8)
    out = be.alloc(nx * ns)
    out.fill(np.nan)
    be.ok(be.lib.d4w_design_mask_f32(0, nx, ns, DESIGN_STEP, 1.0 / DESIGN_FS, p8, 0, 0, None, out.ptr, be.stream))
    dense = out.get().reshape(nx, ns)
    assert not np.isnan(dense).any()
    _intact(out)
    return dense


def design_setter(be):
    p8 = (ctypes.c_double * 8)(*DESIGN_P8)

    def setter(rk):
        be.ok(be.lib.d4w_fkd_set_mask_design_f32(rk.h, 0, DESIGN_STEP, 1.0 / DESIGN_FS, p8, 0, 0, None, be.stream))
    return setter
