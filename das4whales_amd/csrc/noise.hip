// Row statistics on MI355X (gfx950): the median the spectrogram correlation divides by (detect.py:600; a radix select, not
// a reduction), np.quantile of every row (row_select.h) and the noise floor of every channel -- reference
// scripts/main_bathynoise.py:139, 183-194 (median and mean of |hilbert|, std, per channel) and :256-259 (mean square and
// mean envelope of a quiet window).  HBM-streaming work (DESIGN.md sections 3.4, 3.4a); no MFMA.
#include "analytic_row.h"
#include "row_select.h"

namespace d4w {

// ---------------------------------------------------------------------------------------------
// np.median of every row (detect.py:600 divides by the median of the sliced spectrogram):
// radix select on order-preserving keys in THREE sweeps of the row -- digits of 11, 11 and 10 bits with an LDS histogram of
// 2048 bins (8 per thread).  The sweeps are what the kernel costs: the detector's rows (13 bins x 1501 frames, 78 KB) do
// not stay in L2 between sweeps (FETCH_SIZE of the former 4 x 8-bit + 1 form: 3.4 GB for an 857-MB spectrogram,
// profiles/r04h/pmc_stream_11020x12000.txt; staging the row in LDS, a sampled one-sweep form and one wave per row were
// all slower, profiles/r04h/README.txt).  For an even count the upper middle value comes out of the last sweep as well: it
// is the lower one again when duplicates cover the next rank, else the next non-empty bin of the last histogram, else the
// smallest key above the selected 22-bit prefix, which the last sweep tracks.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned med_key(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float med_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

constexpr int kMedBins = 2048, kMedPer = kMedBins / kSpThreads;
__global__ __launch_bounds__(kSpThreads) void row_median(const float* __restrict__ v, size_t n,
                                                         float* __restrict__ med) {
    __shared__ unsigned hist[kMedBins];
    __shared__ unsigned wtot[kSpThreads / 64];
    __shared__ unsigned s_bin, s_k, s_excl, s_next, s_above;
    static_assert(kMedPer * kSpThreads == kMedBins, "whole bins per thread");
    const float* row = v + (size_t)blockIdx.x * n;
    const int tid = threadIdx.x;
    unsigned prefix = 0u, mask = 0u, kk = (unsigned)((n - 1) / 2);
    unsigned above = 0xFFFFFFFFu;                                  // smallest key beyond the selected prefix (last sweep)
    unsigned bin = 0u, excl_sel = 0u, h_sel = 0u;
    constexpr int kAhead = 8;
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = (pass == 0) ? 21 : (pass == 1) ? 10 : 0;
        const unsigned dmask = (pass == 2) ? 1023u : 2047u;
        for (int i = tid; i < kMedBins; i += kSpThreads) hist[i] = 0u;
        if (tid == 0) { s_next = 0xFFFFFFFFu; s_above = 0xFFFFFFFFu; }
        __syncthreads();
        // first sweep: every value takes part and the top digit (sign, exponent, two mantissa bits) of a row of magnitudes
        // falls into a handful of bins -- as LDS atomics a many-way same-address conflict per wave.  Four bins around the first
        // value's are counted in registers and added once per wave.
        const unsigned hot = (pass == 0) ? (med_key(row[0]) >> 21) - 1u : 0xFFFFF000u;
        unsigned priv[4] = {0u, 0u, 0u, 0u};
        for (size_t i0 = tid; i0 < n; i0 += (size_t)kAhead * kSpThreads) {
            float q[kAhead];
#pragma unroll
            for (int j = 0; j < kAhead; ++j) {
                const size_t i = i0 + (size_t)j * kSpThreads;
                q[j] = (i < n) ? row[i] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < kAhead; ++j) {
                if (i0 + (size_t)j * kSpThreads < n) {
                    const unsigned k = med_key(q[j]);
                    if ((k & mask) == prefix) {
                        const unsigned bq = (k >> shift) & dmask, d = bq - hot;
                        if (d < 4u) {
#pragma unroll
                            for (int t = 0; t < 4; ++t) priv[t] += (d == (unsigned)t) ? 1u : 0u;
                        } else {
                            atomicAdd(&hist[bq], 1u);
                        }
                    } else if (pass == 2 && (k & mask) > prefix) {
                        above = min(above, k);
                    }
                }
            }
        }
        if (pass == 0) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                unsigned c = priv[t];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
                if ((tid & 63) == 0 && c && hot + (unsigned)t < (unsigned)kMedBins) atomicAdd(&hist[hot + (unsigned)t], c);
            }
        }
        __syncthreads();
        // the bin holding rank kk: kMedPer bins per thread, inclusive scan of the threads' sums
        unsigned h[kMedPer], sum = 0u;
#pragma unroll
        for (int t = 0; t < kMedPer; ++t) { h[t] = hist[kMedPer * tid + t]; sum += h[t]; }
        unsigned incl = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned up = __shfl_up(incl, off);
            if ((tid & 63) >= off) incl += up;
        }
        if ((tid & 63) == 63) wtot[tid >> 6] = incl;
        __syncthreads();
        unsigned before = 0u;
        for (int w = 0; w < (tid >> 6); ++w) before += wtot[w];
        unsigned run = incl + before - sum;                        // keys in the bins before this thread's
#pragma unroll
        for (int t = 0; t < kMedPer; ++t) {
            if (kk >= run && kk < run + h[t]) {                   // exactly one (thread, t): the counts sum to more than kk
                s_bin = (unsigned)(kMedPer * tid + t);
                s_k = kk - run;
                s_excl = run;
            }
            run += h[t];
        }
        __syncthreads();
        bin = s_bin;
        if (pass == 2) {
            excl_sel = s_excl;
            h_sel = hist[bin];
            // the next non-empty bin of the last digit, and the smallest key beyond the prefix
#pragma unroll
            for (int t = 0; t < kMedPer; ++t) {
                const unsigned bq = (unsigned)(kMedPer * tid + t);
                if (bq > bin && h[t]) atomicMin(&s_next, bq);
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) above = min(above, __shfl_xor(above, off));
            if ((tid & 63) == 0) atomicMin(&s_above, above);
        }
        kk = s_k;
        prefix |= bin << shift;
        mask |= dmask << shift;
        __syncthreads();
    }
    if (tid == 0) {
        const unsigned a = prefix;
        unsigned b = a;
        if ((n & 1) == 0) {
            // rank (n - 1) / 2 is key a, the kk-th of its h_sel copies; rank n / 2 is a again unless that was the last copy
            (void)excl_sel;
            if (kk + 1 >= h_sel) b = (s_next != 0xFFFFFFFFu) ? ((prefix & ~1023u) | s_next) : s_above;
        }
        med[blockIdx.x] = (n & 1) ? med_unkey(a) : 0.5f * (med_unkey(a) + med_unkey(b));
    }
}

// np.quantile of every row, and its mean from the same sweep
__global__ __launch_bounds__(kSpThreads) void row_quantile(const float* __restrict__ v, size_t n, size_t ld, SelRanks R,
                                                           float* __restrict__ out, float* __restrict__ mean) {
    __shared__ double sel_raw[kSelLdsBytes / sizeof(double)];
    const SelLds S = sel_lds(reinterpret_cast<unsigned char*>(sel_raw));
    double sum = 0.0;
    row_select(v + (size_t)blockIdx.x * ld, n, R, S, threadIdx.x, kSpThreads, out ? out + (size_t)blockIdx.x * R.nq : nullptr,
               mean ? &sum : nullptr);
    if (mean && threadIdx.x == 0) mean[blockIdx.x] = (float)(sum / (double)n);
}

// mean(x^2) and np.std(x) of a row: every lane keeps sum x^2 and, shifted by the first sample it meets, sum d and sum d^2 in
// float64 (row_var's form); the lanes' (count, mean, M2) are merged pairwise, x^2 summed by the same butterfly.
// Three float64 operations per sample (they are what the one-read kernel pays for its moments): the lane's sum of squares
// follows from the shifted sums, sum x^2 = sum d^2 + 2 c sum d + n c^2.
struct MomLane { double c, s1, s2; unsigned cnt; };
__device__ __forceinline__ void mom_take(MomLane& a, float v) {
    const double d = (double)v - a.c;
    a.s1 += d;
    a.s2 = fma(d, d, a.s2);
    a.cnt += 1u;
}
// red: [4][kAnMaxThreads / 64] doubles of LDS.  One barrier; thread 0 writes.
__device__ __forceinline__ void mom_finish(const MomLane& l, double (*red)[kAnMaxThreads / 64], int tid, int nthr, int ns,
                                           float* __restrict__ mean_sq, float* __restrict__ sd) {
    const double cnt = (double)l.cnt;
    double m2 = l.cnt ? l.s2 - l.s1 * l.s1 / cnt : 0.0;
    if (m2 < 0.0) m2 = 0.0;                                        // (a NaN stays one)
    VarAcc a{cnt, l.cnt ? l.c + l.s1 / cnt : 0.0, m2};
    double sq = l.cnt ? l.s2 + 2.0 * l.c * l.s1 + cnt * l.c * l.c : 0.0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a = var_merge(a, VarAcc{__shfl_xor(a.n, off), __shfl_xor(a.mean, off), __shfl_xor(a.m2, off)});
        sq += __shfl_xor(sq, off);
    }
    if ((tid & 63) == 0) { red[0][tid / 64] = a.n; red[1][tid / 64] = a.mean; red[2][tid / 64] = a.m2; red[3][tid / 64] = sq; }
    __syncthreads();
    if (tid == 0) {
        VarAcc t{red[0][0], red[1][0], red[2][0]};
        double q = red[3][0];
        for (int w = 1; w < nthr / 64; ++w) {
            t = var_merge(t, VarAcc{red[0][w], red[1][w], red[2][w]});
            q += red[3][w];
        }
        if (mean_sq) mean_sq[blockIdx.x] = (float)(q / (double)ns);
        if (sd) sd[blockIdx.x] = (float)sqrt(t.m2 / (double)ns);
    }
}

__global__ __launch_bounds__(kSpThreads) void row_moments(const float* __restrict__ x, int ns, size_t ld,
                                                          float* __restrict__ mean_sq, float* __restrict__ sd) {
    __shared__ double red[4][kAnMaxThreads / 64];
    const float* row = x + (size_t)blockIdx.x * ld;
    const int tid = threadIdx.x;
    MomLane a{0.0, 0.0, 0.0, 0u};
    if ((ns & 3) == 0 && (reinterpret_cast<uintptr_t>(row) & 15) == 0) {
        const float4* r4 = reinterpret_cast<const float4*>(row);
        const int n4 = ns >> 2;
        if (tid < n4) a.c = (double)r4[tid].x;
        constexpr int kAhead = 4;
        for (int i0 = tid; i0 < n4; i0 += kAhead * kSpThreads) {
            float4 q[kAhead];
#pragma unroll
            for (int k = 0; k < kAhead; ++k) {
                const int i = i0 + k * kSpThreads;
                if (i < n4) q[k] = r4[i];
            }
#pragma unroll
            for (int k = 0; k < kAhead; ++k)
                if (i0 + k * kSpThreads < n4) { mom_take(a, q[k].x); mom_take(a, q[k].y); mom_take(a, q[k].z); mom_take(a, q[k].w); }
        }
    } else {
        if (tid < ns) a.c = (double)row[tid];
        for (int i = tid; i < ns; i += kSpThreads) mom_take(a, row[i]);
    }
    mom_finish(a, red, tid, kSpThreads, ns, mean_sq, sd);
}

// rows of a column window gathered into contiguous rows (the long-row transform reads whole rows)
__global__ __launch_bounds__(kSpThreads) void gather_rows(const float* __restrict__ x, int ns, size_t ld, float* __restrict__ y) {
    const float* row = x + (size_t)blockIdx.y * ld;
    float* out = y + (size_t)blockIdx.y * ns;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += gridDim.x * blockDim.x) out[i] = row[i];
}

// The one-read form: one workgroup per row stages the row (taking the moments of the samples as they pass), runs analytic_rows'
// transform - multiplier - inverse, leaves the ENVELOPE in the tile in place of the Hilbert values and runs the select and the
// envelope's sum over it in LDS; nothing of [nx, ns] size is written.  The second touch of the samples (the envelope's real
// part, as in analytic_rows) re-reads the row this workgroup has just staged.
//   PACKED: even ns, the tile holds ns / 2 pairs of Hilbert values, replaced pair by pair by the same lane.  al8 = 0 (a column
//     window whose rows are only 4-byte aligned): the pairs are read as two 4-byte loads, never as one 8-byte load.
//   plain (odd ns): the tile holds ns complex values and the envelope takes the first half of it; a chunk of envelopes is
//     formed, a barrier, then written -- chunk k lands on complex elements [k nthr / 2, (k + 1) nthr / 2), all read by then.
//   sel_off: where the select's scratch lies -- in the tile's unused part where that is large enough, else behind the twiddles.
template <bool PACKED, bool GENERIC>
__global__ __launch_bounds__(kAnMaxThreads) void noise_rows(RowFftDev F, const float* __restrict__ x, int ns, size_t ld,
                                                         int al8, int sel_off, SelRanks R, float* __restrict__ mean_sq,
                                                         float* __restrict__ sd, float* __restrict__ env_mean,
                                                         float* __restrict__ env_q) {
    D4W_DYN_LDS(smem_raw);
    __shared__ double red[4][kAnMaxThreads / 64];
    float2* tile = reinterpret_cast<float2*>(smem_raw);
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int L = F.ax.L;
    const float* xr = x + (size_t)blockIdx.x * ld;
    const bool want_env = env_mean || R.nq > 0;                      // uniform
    TwLds tw{};
    if (want_env) tw = tw_stage(row_tw_axis(F), tile + row_tile_elems(F), tid, nthr);
    MomLane a{0.0, 0.0, 0.0, 0u};
    auto pair_at = [&](int m) -> float2 {
        if (al8) return reinterpret_cast<const float2*>(xr)[m];
        return make_float2(xr[2 * m], xr[2 * m + 1]);
    };
    if (PACKED) {
        if (tid < L) a.c = (double)xr[2 * tid];
        an_pair_sweep(L, tid, nthr, pair_at, [&](int m, float2 q) {
            if (want_env) tile[m] = q;
            mom_take(a, q.x);
            mom_take(a, q.y);
        });
    } else {
        if (tid < L) a.c = (double)xr[tid];
        for (int n = tid; n < L; n += nthr) {
            const float v = xr[n];
            if (want_env) tile[n] = make_float2(v, 0.f);
            mom_take(a, v);
        }
    }
    mom_finish(a, red, tid, nthr, ns, mean_sq, sd);
    if (!want_env) return;
    lds_barrier();
    row_dft<false, GENERIC>(tile, F, tw, tid, nthr);
    an_multiplier<PACKED>(tile, F, tid, nthr);
    lds_barrier();
    row_dft<true, GENERIC>(tile, F, tw, tid, nthr);
    const float scale = 1.0f / (float)L;
    float* env = reinterpret_cast<float*>(tile);
    if (PACKED) {
        an_pair_sweep(L, tid, nthr, pair_at, [&](int m, float2 q) {
            const float2 h = tile[m];
            const float i0 = h.x * scale, i1 = h.y * scale;
            tile[m] = make_float2(sqrtf(fmaf(q.x, q.x, i0 * i0)), sqrtf(fmaf(q.y, q.y, i1 * i1)));
        });
    } else {
        for (int i0 = 0; i0 < ns; i0 += nthr) {
            const int i = i0 + tid;
            float v = 0.f;
            if (i < ns) {
                const float re = xr[i], im = tile[i].y * scale;
                v = sqrtf(fmaf(re, re, im * im));
            }
            lds_barrier();
            if (i < ns) env[i] = v;
        }
    }
    lds_barrier();
    const SelLds S = sel_lds(smem_raw + sel_off);
    double sum = 0.0;
    row_select(env, (size_t)ns, R, S, tid, nthr, env_q ? env_q + (size_t)blockIdx.x * R.nq : nullptr, env_mean ? &sum : nullptr);
    if (env_mean && tid == 0) env_mean[blockIdx.x] = (float)(sum / (double)ns);
}

}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_row_median_f32(const float* v, int nx, size_t per_row, float* med, void* stream) {
    if (!v || !med || nx < 1 || per_row < 1) return fail(D4W_EINVAL, "bad argument");
    D4W_LAUNCH(row_median, dim3(nx), dim3(kSpThreads), 0, stream, v, per_row, med);
    return D4W_OK;
}

int d4w_row_quantile_limits(int* max_q) {
    if (!max_q) return fail(D4W_EINVAL, "NULL argument");
    *max_q = kSelMaxQ;
    return D4W_OK;
}

// h = q (n - 1) in float64 like NumPy's virtual index; lo = floor(h), g = h - lo
static int sel_ranks(const double* q_host, int nq, size_t n, SelRanks* R) {
    if (nq < 0 || nq > kSelMaxQ) return fail(D4W_EINVAL, "nq = %d not in 0..%d", nq, kSelMaxQ);
    if (nq && !q_host) return fail(D4W_EINVAL, "NULL argument");
    memset(R, 0, sizeof(*R));
    R->nq = nq;
    for (int j = 0; j < nq; ++j) {
        const double q = q_host[j];
        if (!(q >= 0.0 && q <= 1.0)) return fail(D4W_EINVAL, "q[%d] = %g not in [0, 1]", j, q);
        const double h = (double)(n - 1) * q;
        double lo = floor(h);
        if (lo >= (double)(n - 1)) lo = (double)(n - 1);
        R->lo[j] = (unsigned)lo;
        R->g[j] = h - lo;
    }
    return D4W_OK;
}

int d4w_row_quantile_f32(const float* v, int nx, size_t per_row, size_t ld, const double* q_host, int nq, float* out,
                         void* stream) {
    if (!v || !out || nx < 1) return fail(D4W_EINVAL, "bad argument");
    if (per_row < 1 || per_row > 0x7FFFFFFFu || ld < per_row) return fail(D4W_EINVAL, "per_row = %zu (1 .. 2^31 - 1), ld = %zu >= per_row", per_row, ld);
    if (nq < 1) return fail(D4W_EINVAL, "nq = %d not in 1..%d", nq, kSelMaxQ);
    SelRanks R;
    int rc = sel_ranks(q_host, nq, per_row, &R);
    if (rc) return rc;
    D4W_LAUNCH(row_quantile, dim3(nx), dim3(kSpThreads), 0, stream, v, per_row, ld, R, out, (float*)nullptr);
    return D4W_OK;
}

// LDS of the one-read form for rows of ns samples (host arithmetic only): the transform tile of tile_elems values and its
// twiddles, plus the select's scratch unless the tile's part the envelope leaves free holds it.
static size_t noise_lds(int ns, int tile_elems, int* sel_off) {
    const size_t tile_bytes = row_tile_bytes(tile_elems);
    const size_t env_bytes = ((size_t)ns * sizeof(float) + 7) & ~(size_t)7;
    const size_t room = (size_t)tile_elems * sizeof(float2) - env_bytes;
    if (room >= kSelLdsBytes) { *sel_off = (int)env_bytes; return tile_bytes; }
    *sel_off = (int)tile_bytes;
    return tile_bytes + kSelLdsBytes;
}

int d4w_channel_noise_fits_lds(int ns) {
    if (ns < 2) return 0;
    const int elems = row_fft_tile_elems((ns % 2 == 0) ? ns / 2 : ns);
    if (row_tile_bytes(elems) > kSpLdsMax) return 0;
    int off = 0;
    return noise_lds(ns, elems, &off) <= kSpLdsMax ? 1 : 0;
}

constexpr int kNoiseSlab = 65535;      // rows per pass of the long-row form (d4w_analytic_long_f32's grid limit)

size_t d4w_channel_noise_ws_bytes(int nx, int ns) {
    if (nx < 1 || ns < 2) return 0;
    const int nb = std::min(nx, kNoiseSlab);
    // the envelope, the gathered rows of a column window, the long transform's own scratch
    return 2 * (size_t)nb * ns * sizeof(float) + d4w_analytic_long_ws_bytes(nb, ns);
}

int d4w_channel_noise_f32(const float* x, int nx, int ns, size_t ld, const double* q_host, int nq, float* mean_sq, float* sd,
                          float* env_mean, float* env_q, void* ws, int how, void* stream) {
    if (!x || nx < 1 || ns < 2 || ld < (size_t)ns) return fail(D4W_EINVAL, "bad argument");
    if (how < 0 || how > 2) return fail(D4W_EINVAL, "how = %d not in 0..2", how);
    SelRanks R;
    int rc = sel_ranks(q_host, nq, (size_t)ns, &R);
    if (rc) return rc;
    if (nq == 0) env_q = nullptr;
    if (!env_q) R.nq = 0;                                            // NULL like every other output: not formed
    const bool fits = d4w_channel_noise_fits_lds(ns) != 0;
    if (how == 1 && !fits) return fail(D4W_EINVAL, "rows of %d samples do not fit the one-read form (d4w_channel_noise_fits_lds)", ns);
    if (how == 0) how = fits ? 1 : 2;
    if (!mean_sq && !sd && !env_mean && !env_q) return D4W_OK;
    if (how == 1) {
        const bool packed = (ns % 2 == 0);
        const int L = packed ? ns / 2 : ns;
        const RowFftHost* h = nullptr;
        rc = row_fft_get(L, &h);
        if (rc) return rc;
        int sel_off = 0;
        const size_t lds = noise_lds(ns, h->dev.bs_L ? h->dev.bs_L : L, &sel_off);
        if (lds > kSpLdsMax) return fail(D4W_EINVAL, "rows of %d samples do not fit the one-read form", ns);
        // 8-byte row loads only where every row starts on 8 bytes: decided from the pointer and the pitch, not from ns
        const int al8 = ((reinterpret_cast<uintptr_t>(x) & 7) == 0 && (ld & 1) == 0) ? 1 : 0;
        const int threads = L >= 2048 ? kAnMaxThreads : kSpThreads;
        return with_flags(packed, h->generic, [&](auto P, auto G) {
            constexpr auto kern = noise_rows<decltype(P)::value, decltype(G)::value>;
            allow_lds(kern, lds);
            D4W_LAUNCH(kern, dim3(nx), dim3(threads), lds, stream, h->dev, x, ns, ld, al8, sel_off, R, mean_sq, sd, env_mean,
                       env_q);
            return (int)D4W_OK;
        });
    }
    const bool want_env = env_mean || env_q;
    if (want_env && !ws) return fail(D4W_EINVAL, "the long-row form needs the workspace of d4w_channel_noise_ws_bytes");
    for (int a = 0; a < nx; a += kNoiseSlab) {
        const int nb = std::min(nx - a, kNoiseSlab);
        const float* xb = x + (size_t)a * ld;
        if (mean_sq || sd)
            D4W_LAUNCH(row_moments, dim3(nb), dim3(kSpThreads), 0, stream, xb, ns, ld, mean_sq ? mean_sq + a : nullptr,
                       sd ? sd + a : nullptr);
        if (!want_env) continue;
        const int nws = std::min(nx, kNoiseSlab);
        float* env = (float*)ws;
        float* rows = env + (size_t)nws * ns;
        void* lws = rows + (size_t)nws * ns;
        if (ld != (size_t)ns) {
            D4W_LAUNCH(gather_rows, dim3(std::min(ceil_div(ns, kSpThreads), 64), nb), dim3(kSpThreads), 0, stream, xb, ns, ld, rows);
            xb = rows;
        }
        rc = d4w_analytic_long_f32(xb, env, nb, ns, kAnEnvelope, nullptr, 0.0, lws, stream);
        if (rc) return rc;
        D4W_LAUNCH(row_quantile, dim3(nb), dim3(kSpThreads), 0, stream, (const float*)env, (size_t)ns, (size_t)ns, R,
                   env_q ? env_q + (size_t)a * R.nq : nullptr, env_mean ? env_mean + a : nullptr);
    }
    return D4W_OK;
}

}  // extern "C"
