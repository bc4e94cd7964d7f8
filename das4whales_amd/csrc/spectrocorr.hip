// Spectrogram x kernel correlation on MI355X (gfx950): reference detect.py:579-602 (xcorr2d) and :605-647 (xcorr).  The
// median it divides by is row_median of noise.hip.  HBM-streaming work; no MFMA.
#include "d4w_internal.h"

namespace d4w {

// ---------------------------------------------------------------------------------------------
// spectrogram x kernel correlation along time, summed over frequency:
//   raw[c][t] = sum_f sum_j S[c][f][t + j - off] K[f][j]   (S = 0 outside [0, nt)),  t < nout
//   zero_ends == 0:  out = max(raw, 0) / (med[c] * nk)     (detect.py:597-600: clipped, then divided)
//   zero_ends != 0:  out = max(raw / (med[c] * nk), 0), first and last value forced to 0
//                                                          (detect.py:632-645: divided, then clipped)
// The two differ when med[c] < 0 (a spectrogram in dB): the first form is then <= 0, the second >= 0.
// off = nk/2, nout = nt, zero_ends = 0 reproduces detect.xcorr2d (fftconvolve(S, flip(K, 1), 'same', axes=1));
// off = 0, nout = nt-nk+1, zero_ends = 1 reproduces detect.xcorr.
// ---------------------------------------------------------------------------------------------
constexpr int kScThreads = 128, kScPer = 4, kScTile = kScThreads * kScPer;      // 512 correlation lags per workgroup
constexpr int kScLdsFloats = 2560;          // a few strip rows at a time: a small footprint keeps ~30 waves on a CU
__host__ __device__ constexpr int sc_width(int nk) { return (kScTile + nk + 2 + 3) & ~3; }

// Four consecutive lags per lane: a lane reads its window of a strip row in 16-byte pieces (conflict-free) and every piece
// feeds 16 FMAs -- a quarter of the LDS reads of one lag per lane -- with the 7 kernel taps a piece meets as wave-uniform
// scalars; the strip itself is filled with eight global loads in flight per lane.
// The strip of the NEXT frequency rows is already in registers while this one is worked on (one exposed load latency per
// workgroup instead of one per chunk: the kernel was bound by those waits and by an integer division per staged sample, 0.44 ms
// for a 0.86-GB spectrogram at 11020 x 12000; round 5).
// FL strip rows of M pieces per lane and chunk (FL x M x kScThreads >= FL x width staged samples: 4 x 5 for kernels of up to
// ~120 frames, 2 x 10, 1 x 20 beyond), chosen by the host from the kernel's length.
template <int FL, int M>
__global__ __launch_bounds__(kScThreads) void spectro_corr(const float* __restrict__ S, int nf, int nt,
                                                           const float* __restrict__ K, int nk, int off, int nout,
                                                           const float* __restrict__ med, int zero_ends,
                                                           float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float strip[kScLdsFloats];
    static_assert(FL * M * kScThreads <= kScLdsFloats + FL * kScThreads, "a chunk fits the strip");
    const int tid = threadIdx.x;
    const int t0 = blockIdx.x * kScTile;
    const int width = sc_width(nk);
    constexpr int fchunk = FL;
    const float* Sc = S + (size_t)blockIdx.y * nf * nt;
    float acc[kScPer] = {0.f, 0.f, 0.f, 0.f};
    float q[FL][M];
    auto fetch = [&](int f0) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const int j = tid + m * kScThreads, sidx = t0 + j - off;
            const bool in = j < width && sidx >= 0 && sidx < nt;
#pragma unroll
            for (int fl = 0; fl < FL; ++fl) q[fl][m] = (in && f0 + fl < nf) ? Sc[(size_t)(f0 + fl) * nt + sidx] : 0.f;
        }
    };
    auto stash = [&](int f0) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const int j = tid + m * kScThreads;
#pragma unroll
            for (int fl = 0; fl < FL; ++fl)
                if (j < width && f0 + fl < nf) strip[fl * width + j] = q[fl][m];
        }
    };
    fetch(0);
    for (int f0 = 0; f0 < nf; f0 += fchunk) {
        const int fn = min(fchunk, nf - f0);
        stash(f0);
        __syncthreads();
        if (f0 + fchunk < nf) fetch(f0 + fchunk);                 // in flight during the products below
        for (int fl = 0; fl < fn; ++fl) {
            const float* kr = K + (size_t)(f0 + fl) * nk;
            const float4* sr4 = reinterpret_cast<const float4*>(strip + fl * width) + tid;
            for (int c = 0; 4 * c < nk + 3; ++c) {
                const float4 v4 = sr4[c];
                const float v[4] = {v4.x, v4.y, v4.z, v4.w};
                // sample e of the piece sits at lag offset 4 c + e: tap j = 4 c + e - q for lag q of this lane.  Taps outside
                // [0, nk) are skipped (wave-uniform branch), not multiplied by zero: a NaN next to the window stays out
#pragma unroll
                for (int d = 0; d < 7; ++d) {
                    const int j = 4 * c - 3 + d;
                    if (j >= 0 && j < nk) {
                        const float tap = kr[j];
#pragma unroll
                        for (int qq = 0; qq < kScPer; ++qq) {
                            const int e = d - 3 + qq;
                            if (e >= 0 && e < 4) acc[qq] = fmaf(v[e], tap, acc[qq]);
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int qq = 0; qq < kScPer; ++qq) {
        const int t = t0 + kScPer * tid + qq;
        if (t < nout) {
            // the two reference forms clip at different places, which shows once the median is negative (a dB spectrogram):
            // xcorr2d clips the raw sum and then divides, xcorr divides, zeroes its ends and then clips
            float v = acc[qq];
            if (!zero_ends && v < 0.f) v = 0.f;
            v /= med[blockIdx.y] * (float)nk;
            if (zero_ends) {
                if (t == 0 || t == nout - 1) v = 0.f;
                if (v < 0.f) v = 0.f;
            }
            out[(size_t)blockIdx.y * nout + t] = v;                  // NaN (0/0 on an all-zero row) passes through both forms
        }
    }
}

}  // namespace d4w

using namespace d4w;

extern "C" int d4w_spectrocorr_f32(const float* S, int nx, int nf, int nt, const float* K, int nk, int off, int nout,
                                   const float* med, int zero_ends, float* out, void* stream) {
    if (!S || !K || !med || !out || nx < 1 || nf < 1 || nt < 1 || nk < 1 || nout < 1)
        return fail(D4W_EINVAL, "bad argument");
    if (sc_width(nk) > kScLdsFloats) return fail(D4W_EINVAL, "kernel of %d frames is too long", nk);
    if (nx > 65535) return fail(D4W_EINVAL, "nx = %d exceeds the grid limit 65535", nx);
    const dim3 grid(ceil_div(nout, kScTile), nx);
    const int width = sc_width(nk);
    if (width <= 5 * kScThreads)
        D4W_LAUNCH((spectro_corr<4, 5>), grid, dim3(kScThreads), 0, stream, S, nf, nt, K, nk, off, nout, med, zero_ends, out);
    else if (width <= 10 * kScThreads)
        D4W_LAUNCH((spectro_corr<2, 10>), grid, dim3(kScThreads), 0, stream, S, nf, nt, K, nk, off, nout, med, zero_ends, out);
    else
        D4W_LAUNCH((spectro_corr<1, 20>), grid, dim3(kScThreads), 0, stream, S, nf, nt, K, nk, off, nout, med, zero_ends, out);
    return D4W_OK;
}
