// Per-channel power spectral density and energy of consecutive time chunks on MI355X (gfx950):
//   * Welch PSD of every chunk as the reference's tools.spec forms it with scipy.signal.welch
//     (tools.py:212-236): periodic Hann, each segment's own mean removed, nfft = nperseg,
//     scaling='density', one-sided, average='mean';
//   * sum of squares of every chunk (tools.energy_TimeDomain, tools.py:84-157).
// Both read the block once (4 B / sample) and write next to nothing: the
// spectrogram [segments x bins] of a chunk is never formed in HBM.  A workgroup owns one (row,
// chunk).  It stages the samples that a group of segments covers in LDS once (overlapping segments
// are not read twice), two real segments ride one complex transform z = s_a + i s_b of fft_lds.h,
// and |Z|^2 is summed per LDS position in float64: no untangling is needed for the average, since
// |S_a[k]|^2 + |S_b[k]|^2 = (|Z[k]|^2 + |Z[N-k]|^2) / 2.  k is folded with N - k once per chunk.
// The segment transform's tables (stage radices, positions, periodic Hann and its float64 sum of squares) are the row
// operators' plan of the same length (row_fft.h).
#include "row_fft.h"

namespace d4w {

constexpr int kWelchThreads = 256;
constexpr int kWelchMinSeg = 16, kWelchMaxSeg = 4096;
constexpr int kWelchTile = 4096;                               // complex LDS elements of a group of segment pairs
constexpr int kWelchMaxPairs = 16;

struct WelchDims {
    int ns, chunk, nchunks;
    int N, step, nseg;    // segment length, distance of segment starts, whole segments per chunk
    int nb;               // segment pairs transformed together
    int seg_cap;          // floats of the staged samples' LDS area (a multiple of 4)
    double scale;         // 1 / (fs sum(w^2) nseg)
};

// `len` floats from src to dst, dst[j] = src[j], with dst as far into its 16-byte LDS slot as src is into its own in
// memory: 16-byte loads and LDS stores wherever src allows them, single floats before and after (odd ns or chunk leave
// most chunk starts unaligned).  The caller synchronises.
__device__ __forceinline__ void welch_stage(const float* __restrict__ src, float* __restrict__ dst, int len, int tid) {
    const int pro = min((4 - (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3)) & 3, len);
    if (tid < pro) dst[tid] = src[tid];
    const int n4 = (len - pro) >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src + pro);
    float4* d4 = reinterpret_cast<float4*>(dst + pro);
    constexpr int kAhead = 4;                                       // 16-byte loads in flight per lane
    for (int i0 = tid; i0 < n4; i0 += kAhead * kWelchThreads) {
        float4 q[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            const int i = i0 + k * kWelchThreads;
            if (i < n4) q[k] = s4[i];
        }
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            const int i = i0 + k * kWelchThreads;
            if (i < n4) d4[i] = q[k];
        }
    }
    const int done = pro + 4 * n4;
    if (tid < len - done) dst[done + tid] = src[done + tid];
}

template <bool GENERIC>
__global__ __launch_bounds__(kWelchThreads) void welch_chunks(RowFftDev F, WelchDims d, const float* __restrict__ x,
                                                              float* __restrict__ pxx) {
    D4W_DYN_LDS(smem_raw);
    const int tid = threadIdx.x, N = d.N;
    float2* tile = reinterpret_cast<float2*>(smem_raw);               // [nb][N]
    double* accp = reinterpret_cast<double*>(tile + d.nb * N);        // [N] sum of |Z|^2 by LDS position, over the chunk
    float* segbuf = reinterpret_cast<float*>(accp + N);               // [seg_cap], 16-byte aligned
    float* win = segbuf + d.seg_cap;                                  // [N]
    Mean2* mean = reinterpret_cast<Mean2*>(win + N);                  // [2 nb] segment means as hi + lo
    const TwLds tw = tw_stage(F.ax, reinterpret_cast<float2*>(mean + 2 * d.nb), tid, kWelchThreads);
    for (int i = tid; i < N; i += kWelchThreads) win[i] = F.hann[i];
    const unsigned row = blockIdx.x / (unsigned)d.nchunks, j = blockIdx.x - row * (unsigned)d.nchunks;
    const float* xc = x + (size_t)row * d.ns + (size_t)j * d.chunk;
    const FDiv dn(N);
    for (int p = tid; p < N; p += kWelchThreads) accp[p] = 0.0;       // position p stays with thread p % 256: no barrier needed
    for (int s0 = 0; s0 < d.nseg; s0 += 2 * d.nb) {
        const int nst = min(2 * d.nb, d.nseg - s0);                   // segments of this group, in nbt transforms
        const int nbt = (nst + 1) >> 1;
        const float* src = xc + (size_t)s0 * d.step;
        float* seg = segbuf + (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3);
        welch_stage(src, seg, (nst - 1) * d.step + N, tid);
        __syncthreads();
        // detrend='constant': every segment's own mean, summed in float64 by one wave and kept as a two-float value, so
        // that a sample loses its segment's offset before anything is rounded to the float32 of the offset (a row
        // 1000 x its rms off zero is 4e-5 of the PSD maximum wrong in bins 0 and 1 with a float32 mean)
        for (int s = tid >> 6; s < nst; s += kWelchThreads / 64) {
            const float* sp = seg + s * d.step;
            double m = 0.0;
            for (int n = tid & 63; n < N; n += 64) m += (double)sp[n];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) m += __shfl_xor(m, off);
            if ((tid & 63) == 0) {
                m /= (double)N;
                Mean2 mm;
                mm.hi = (float)m;
                mm.lo = (float)(m - (double)mm.hi);
                mean[s] = mm;
            }
        }
        __syncthreads();
        for (int w = tid; w < nbt * N; w += kWelchThreads) {
            const int b = dn.div(w), n = w - b * N;
            const float wn = win[n];
            const float* sa = seg + 2 * b * d.step + n;
            float2 v = make_float2(demean(sa[0], mean[2 * b]) * wn, 0.f);
            if (2 * b + 1 < nst) v.y = demean(sa[d.step], mean[2 * b + 1]) * wn;   // an odd count: the last one rides alone
            tile[w] = v;
        }
        __syncthreads();
        lds_fft<false, false, GENERIC>(tile, F.ax, tw, 1, nbt, N, 1, 0, tid, kWelchThreads);
        for (int p = tid; p < N; p += kWelchThreads) {
            float s = 0.f;
            for (int b = 0; b < nbt; ++b) {
                const float2 z = tile[b * N + p];
                s = fmaf(z.x, z.x, fmaf(z.y, z.y, s));
            }
            accp[p] += (double)s;
        }
        __syncthreads();                                              // seg / tile are refilled by the next group
    }
    // one-sided density: sum over segments of 2 |S[k]|^2 = |Z[k]|^2 + |Z[N-k]|^2 summed over the transforms; DC and Nyquist
    // are not doubled and are their own mirror: |S|^2 = |Z|^2 there
    float* out = pxx + (size_t)blockIdx.x * (N / 2 + 1);
    for (int k = tid; k <= N / 2; k += kWelchThreads) {
        double v = accp[F.pos[k]];
        if (k != 0 && 2 * k != N) v += accp[F.pos[N - k]];
        out[k] = (float)(v * d.scale);
    }
}

// e[row][j] = sum of the squares of chunk j, in float64 (a drifting raw strain row loses its small chunks in a float32 sum)
__global__ __launch_bounds__(kWelchThreads) void chunk_energy(const float* __restrict__ x, int ns, int chunk, int nchunks,
                                                              float* __restrict__ e) {
    __shared__ double red[kWelchThreads / 64];
    const int tid = threadIdx.x;
    const unsigned row = blockIdx.x / (unsigned)nchunks, j = blockIdx.x - row * (unsigned)nchunks;
    const int start = (int)j * chunk, len = min(chunk, ns - start);
    const float* src = x + (size_t)row * ns + start;
    double s = 0.0;
    auto take = [&](float v) { s = fma((double)v, (double)v, s); };
    const int pro = min((4 - (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3)) & 3, len);
    if (tid < pro) take(src[tid]);
    const int n4 = (len - pro) >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src + pro);
    constexpr int kAhead = 4;                                       // 16-byte loads in flight per lane
    for (int i0 = tid; i0 < n4; i0 += kAhead * kWelchThreads) {
        float4 q[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            const int i = i0 + k * kWelchThreads;
            q[k] = (i < n4) ? s4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < kAhead; ++k) { take(q[k].x); take(q[k].y); take(q[k].z); take(q[k].w); }
    }
    const int done = pro + 4 * n4;
    if (tid < len - done) take(src[done + tid]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        double t = red[0];
        for (int w = 1; w < kWelchThreads / 64; ++w) t += red[w];
        e[blockIdx.x] = (float)t;
    }
}

}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_welch_bins(int nperseg) { return nperseg > 0 ? nperseg / 2 + 1 : 0; }

int d4w_welch_segments(int n, int nperseg, int noverlap) {
    if (nperseg < 1 || noverlap < 0 || noverlap >= nperseg || n < nperseg) return 0;
    return (n - noverlap) / (nperseg - noverlap);
}

int d4w_welch_supported(int nperseg) {
    if (nperseg < kWelchMinSeg || nperseg > kWelchMaxSeg || (nperseg & 1)) return 0;
    std::vector<int> rad;
    return factor_radices(nperseg, rad) ? 1 : 0;
}

int d4w_welch_f32(const float* x, int nx, int ns, int chunk, int nperseg, int noverlap, double fs, float* pxx,
                  void* stream) {
    if (!x || !pxx || nx < 1 || ns < 1) return fail(D4W_EINVAL, "bad argument");
    if (nperseg & 1) return fail(D4W_EINVAL, "nperseg = %d must be even", nperseg);
    if (nperseg < kWelchMinSeg || nperseg > kWelchMaxSeg)
        return fail(D4W_EINVAL, "nperseg = %d outside %d..%d", nperseg, kWelchMinSeg, kWelchMaxSeg);
    if (!d4w_welch_supported(nperseg))
        return fail(D4W_EINVAL, "nperseg = %d has a prime factor > 31: no segment transform", nperseg);
    if (noverlap < 0 || noverlap >= nperseg) return fail(D4W_EINVAL, "noverlap = %d outside 0..nperseg - 1 = %d", noverlap, nperseg - 1);
    if (chunk < nperseg || chunk > ns)
        return fail(D4W_EINVAL, "chunk = %d outside nperseg..ns = %d..%d", chunk, nperseg, ns);
    if (!(fs > 0.0)) return fail(D4W_EINVAL, "fs = %g must be positive", fs);
    const int nchunks = ns / chunk;
    if ((long long)nx * nchunks > 0x7FFFFFFFLL) return fail(D4W_EINVAL, "nx x chunks = %d x %d exceeds the grid limit", nx, nchunks);
    const RowFftHost* h = nullptr;
    int rc = row_fft_get(nperseg, &h);      // (never a Bluestein plan: d4w_welch_supported above)
    if (rc) return rc;
    WelchDims d;
    d.ns = ns; d.chunk = chunk; d.nchunks = nchunks;
    d.N = nperseg; d.step = nperseg - noverlap; d.nseg = d4w_welch_segments(chunk, nperseg, noverlap);
    d.nb = std::min(std::min(std::max(1, kWelchTile / nperseg), kWelchMaxPairs), (d.nseg + 1) / 2);
    // samples a group of 2 nb segments covers, + 3 for the start's place in its 16-byte slot
    d.seg_cap = (int)((((long long)(2 * d.nb - 1) * d.step + nperseg + 3) + 3) & ~3LL);
    d.scale = 1.0 / (fs * h->sumw2 * (double)d.nseg);
    const size_t lds = (size_t)d.nb * nperseg * sizeof(float2) + (size_t)nperseg * sizeof(double) + (size_t)d.seg_cap * sizeof(float) + (size_t)nperseg * sizeof(float)
                       + (size_t)2 * d.nb * sizeof(Mean2) + (size_t)(kTwLo + h->dev.ax.nhi) * sizeof(float2);
    const dim3 grid((unsigned)((long long)nx * nchunks));
    return with_flag(h->generic, [&](auto G) {
        constexpr auto kern = welch_chunks<decltype(G)::value>;
        allow_lds(kern, lds);
        D4W_LAUNCH(kern, grid, dim3(kWelchThreads), lds, stream, h->dev, d, x, pxx);
        return (int)D4W_OK;
    });
}

int d4w_chunk_energy_f32(const float* x, int nx, int ns, int chunk, float* e, void* stream) {
    if (!x || !e || nx < 1 || ns < 1) return fail(D4W_EINVAL, "bad argument");
    if (chunk < 1 || chunk > ns) return fail(D4W_EINVAL, "chunk = %d outside 1..ns = %d", chunk, ns);
    const int nchunks = (ns - 1) / chunk + 1;
    if ((long long)nx * nchunks > 0x7FFFFFFFLL) return fail(D4W_EINVAL, "nx x chunks = %d x %d exceeds the grid limit", nx, nchunks);
    D4W_LAUNCH(chunk_energy, dim3((unsigned)((long long)nx * nchunks)), dim3(kWelchThreads), 0, stream, x, ns, chunk, nchunks, e);
    return D4W_OK;
}

}  // extern "C"
