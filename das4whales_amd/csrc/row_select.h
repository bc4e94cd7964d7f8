// Exact order statistics of one row by a radix select on order-preserving keys (the keys of med_key in noise.hip: sign
// flipped, negative values complemented), written once for a row in global memory (d4w_row_quantile_f32, the long-row form of
// d4w_channel_noise_f32) and for a row that sits in LDS (the one-read form of d4w_channel_noise_f32): the row is a plain
// `const float*` either way and every function is inlined into its kernel, so the compiler sees which address space it is.
//
// One workgroup per row, 64 k threads with k dividing 32.  Sweeps of the row:
//   * the FIRST, shared by every requested rank: histogram of the top 11 key bits (kept in hist0), the NaN flag, and -- on
//     request -- the row's sum in float64 (fixed order: lane-strided partial sums, xor butterfly inside a wave, the waves in
//     order);
//   * per requested rank TWO more, digits of 11 and 10 bits below the bin hist0 puts the rank in.  The last one also yields the
//     NEXT order statistic (NumPy's "linear" quantile interpolates between ranks floor(h) and floor(h) + 1): the same key
//     again while copies remain, else the next non-empty bin of the last histogram, else the smallest key above the 22-bit
//     prefix, which that sweep tracks.
// 1 + 2 nq sweeps in all.  In LDS a sweep is cheap; over global memory a row of ordinary length is served by L2 after the
// first (profiles/noise/README.txt).  -0 and +0 share a key (+0); a NaN anywhere makes every result of the row NaN.
#pragma once
#include "d4w_internal.h"

namespace d4w {

constexpr int kSelBins = 2048;
constexpr int kSelMaxQ = 8;
constexpr int kSelMaxWaves = 16;

// the requested quantiles of a row of n values, formed on the host in float64 like NumPy: h = q (n - 1), lo = floor(h),
// g = h - lo  (lo = n - 1, g = 0 at q = 1)
struct SelRanks {
    int nq;
    unsigned lo[kSelMaxQ];
    double g[kSelMaxQ];
};

// LDS scratch of the select: 2 histograms, the wave totals of the scan, a few scalars, the waves' partial sums
struct SelLds {
    unsigned* hist0;
    unsigned* hist;
    unsigned* wtot;     // [kSelMaxWaves]
    unsigned* s;        // [8]: bin, rank inside it, its count, next bin, smallest key above, NaN flag
    double* red;        // [kSelMaxWaves]
};
constexpr size_t kSelLdsBytes = (2 * (size_t)kSelBins + kSelMaxWaves + 8) * sizeof(unsigned) + kSelMaxWaves * sizeof(double);

__device__ __forceinline__ SelLds sel_lds(unsigned char* p) {      // p: 8-byte aligned, kSelLdsBytes long
    SelLds S;
    S.red = reinterpret_cast<double*>(p);
    S.hist0 = reinterpret_cast<unsigned*>(S.red + kSelMaxWaves);
    S.hist = S.hist0 + kSelBins;
    S.wtot = S.hist + kSelBins;
    S.s = S.wtot + kSelMaxWaves;
    return S;
}

__device__ __forceinline__ unsigned sel_key(float v) {
    const unsigned b = (v == 0.f) ? 0u : __float_as_uint(v);      // -0 == +0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sel_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// The bin of `hist` that holds rank kk (kk < the histogram's total), the rank inside that bin and the bin's count.  Every thread
// of the workgroup calls it; two barriers inside.  The caller puts a barrier between two calls (a sweep always lies between them):
// the next call writes S.wtot and S.s[0 .. 2] again.
__device__ __forceinline__ void sel_locate(const unsigned* hist, unsigned kk, const SelLds& S, int tid, int nthr,
                                           unsigned& bin, unsigned& krem, unsigned& hsel) {
    const int per = kSelBins / nthr;
    unsigned sum = 0u;
    for (int t = 0; t < per; ++t) sum += hist[per * tid + t];
    unsigned incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned up = __shfl_up(incl, off);
        if ((tid & 63) >= off) incl += up;
    }
    if ((tid & 63) == 63) S.wtot[tid >> 6] = incl;
    __syncthreads();
    unsigned run = incl - sum;
    for (int w = 0; w < (tid >> 6); ++w) run += S.wtot[w];
    for (int t = 0; t < per; ++t) {
        const unsigned h = hist[per * tid + t];
        if (kk >= run && kk < run + h) {                           // exactly one (thread, t)
            S.s[0] = (unsigned)(per * tid + t);
            S.s[1] = kk - run;
            S.s[2] = h;
        }
        run += h;
    }
    __syncthreads();
    bin = S.s[0];
    krem = S.s[1];
    hsel = S.s[2];
}

// One sweep of the row.  PASS 0: every value, top digit into S.hist0 (four bins around the first value's counted in registers
// and added once per wave: a row of magnitudes puts most of its values into a handful of top-digit bins, a many-way
// same-address conflict as LDS atomics -- see row_median), NaN flag, optional sum.  PASS 1 / 2: the values under `prefix`,
// next digit into S.hist; PASS 2 also tracks the smallest key above the prefix.  Barriers before and after.
template <int PASS>
__device__ __forceinline__ void sel_sweep(const float* __restrict__ row, size_t n, unsigned prefix, unsigned mask,
                                          const SelLds& S, int tid, int nthr, double* sum_out) {
    constexpr int shift = (PASS == 0) ? 21 : (PASS == 1) ? 10 : 0;
    constexpr unsigned dmask = (PASS == 2) ? 1023u : 2047u;
    unsigned* hist = (PASS == 0) ? S.hist0 : S.hist;
    for (int i = tid; i < kSelBins; i += nthr) hist[i] = 0u;
    if (tid == 0) {
        S.s[3] = 0xFFFFFFFFu;
        S.s[4] = 0xFFFFFFFFu;
        if (PASS == 0) S.s[5] = 0u;
    }
    __syncthreads();
    const unsigned hot = (PASS == 0) ? (sel_key(row[0]) >> 21) - 1u : 0xFFFFF000u;
    unsigned priv[4] = {0u, 0u, 0u, 0u};
    unsigned above = 0xFFFFFFFFu;
    bool nan = false;
    double acc = 0.0;
    constexpr int kAhead = 8;
    for (size_t i0 = tid; i0 < n; i0 += (size_t)kAhead * nthr) {
        float q[kAhead];
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            const size_t i = i0 + (size_t)j * nthr;
            q[j] = (i < n) ? row[i] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            if (i0 + (size_t)j * nthr < n) {
                const unsigned k = sel_key(q[j]);
                if (PASS == 0) {
                    nan = nan || (q[j] != q[j]);
                    acc += (double)q[j];
                    const unsigned bq = k >> 21, d = bq - hot;
                    if (d < 4u) {
#pragma unroll
                        for (int t = 0; t < 4; ++t) priv[t] += (d == (unsigned)t) ? 1u : 0u;
                    } else {
                        atomicAdd(&hist[bq], 1u);
                    }
                } else if ((k & mask) == prefix) {
                    atomicAdd(&hist[(k >> shift) & dmask], 1u);
                } else if (PASS == 2 && (k & mask) > prefix) {
                    above = min(above, k);
                }
            }
        }
    }
    if (PASS == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            unsigned c = priv[t];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
            if ((tid & 63) == 0 && c && hot + (unsigned)t < (unsigned)kSelBins) atomicAdd(&hist[hot + (unsigned)t], c);
        }
        unsigned f = nan ? 1u : 0u;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) f |= __shfl_xor(f, off);
        if ((tid & 63) == 0 && f) atomicOr(&S.s[5], 1u);
        if (sum_out) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
            if ((tid & 63) == 0) S.red[tid >> 6] = acc;
        }
    }
    if (PASS == 2) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) above = min(above, __shfl_xor(above, off));
        if ((tid & 63) == 0) atomicMin(&S.s[4], above);
    }
    __syncthreads();
    if (PASS == 0 && sum_out) {
        double t = 0.0;
        for (int w = 0; w < nthr / 64; ++w) t += S.red[w];         // the waves in order
        *sum_out = t;
    }
}

// NumPy's lerp of the "linear" method (numpy/lib/_function_base_impl.py, _lerp) in float64, rounded once
__device__ __forceinline__ float sel_lerp(float a, float b, double g) {
    const double da = (double)a, d = (double)b - da;
    double r = da + d * g;
    if (g >= 0.5) r = (double)b - d * (1.0 - g);
    return (float)r;
}

// The quantiles R of row[0 .. n) -> out[0 .. R.nq) (thread 0 writes); *sum_out, if not NULL, = the row's float64 sum in every
// thread.  Every thread of the workgroup calls it; the row is not modified.
__device__ __forceinline__ void row_select(const float* __restrict__ row, size_t n, const SelRanks& R, const SelLds& S,
                                           int tid, int nthr, float* __restrict__ out, double* sum_out) {
    sel_sweep<0>(row, n, 0u, 0u, S, tid, nthr, sum_out);
    const bool has_nan = S.s[5] != 0u;                             // written by the first sweep alone
    for (int j = 0; j < R.nq; ++j) {
        if (has_nan) {                                             // uniform
            if (tid == 0) out[j] = __uint_as_float(0x7FC00000u);
            continue;
        }
        unsigned bin, kk, hsel;
        sel_locate(S.hist0, R.lo[j], S, tid, nthr, bin, kk, hsel);
        unsigned prefix = bin << 21, mask = 2047u << 21;
        sel_sweep<1>(row, n, prefix, mask, S, tid, nthr, nullptr);
        sel_locate(S.hist, kk, S, tid, nthr, bin, kk, hsel);
        prefix |= bin << 10;
        mask |= 2047u << 10;
        sel_sweep<2>(row, n, prefix, mask, S, tid, nthr, nullptr);
        sel_locate(S.hist, kk, S, tid, nthr, bin, kk, hsel);
        {
            const int per = kSelBins / nthr;                       // the next non-empty bin of the last digit
            for (int t = 0; t < per; ++t) {
                const unsigned bq = (unsigned)(per * tid + t);
                if (bq > bin && bq < 1024u && S.hist[bq]) atomicMin(&S.s[3], bq);
            }
        }
        __syncthreads();
        if (tid == 0) {
            const unsigned ka = prefix | bin;
            unsigned kb = ka;
            if ((size_t)R.lo[j] + 1 < n && kk + 1 >= hsel) kb = (S.s[3] != 0xFFFFFFFFu) ? (prefix | S.s[3]) : S.s[4];
            out[j] = sel_lerp(sel_unkey(ka), sel_unkey(kb), R.g[j]);
        }                                                          // (S.s[3], S.s[4] are next written by thread 0 itself)
    }
}

}  // namespace d4w
