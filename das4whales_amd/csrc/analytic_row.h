// What the kernels that form the analytic signal of a row inside one workgroup's LDS share (analytic.hip analytic_rows,
// noise.hip noise_rows): the output modes, the Hilbert multiplier on the transformed row, the staged sweep over the
// sample pairs of a packed row, and the one-sweep variance accumulator.
#pragma once
#include "row_fft.h"

namespace d4w {

//   mode 0: |z|                               (envelope, detect.py:192)
//   mode 1: imag(z) = H[x]
//   mode 2: 10 log10(|z|^2 / var[row])        (dsp.py:975)
//   mode 4: |z| / std[row]                    (improcess.trace2image before scaling, improcess.py:60)
//   mode 3: arg(z[i+1] conj(z[i])) * fscale   (diff(unwrap(angle z)) / 2 pi * fs, dsp.py:846-855),
//           ns - 1 outputs per row
enum { kAnEnvelope = 0, kAnHilbert = 1, kAnSnr = 2, kAnIfreq = 3, kAnEnvStd = 4 };

__device__ __forceinline__ float an_ifreq(float2 z0, float2 z1, float fscale) {
    const float2 p = c_mulc(z1, z0);
    return atan2f(p.y, p.x) * fscale;
}

// The Hilbert multiplier on the transformed row (analytic.hip): the packed form untangles the real spectrum, applies -i / +i and
// tangles again for the packed inverse; the plain form scales by scipy's h.
template <bool PACKED>
__device__ __forceinline__ void an_multiplier(float2* tile, const RowFftDev& F, int tid, int nthr) {
    const int L = F.ax.L;
    if (PACKED) {
        const int M = L;
        for (int f = tid; f <= M / 2; f += nthr) {
            const int g = (f == 0) ? 0 : M - f;
            const int pa = F.pos[f], pb = F.pos[g];
            const float2 a = tile[pa], bc = c_conj(tile[pb]);
            float2 out_a = make_float2(0.f, 0.f), out_b = make_float2(0.f, 0.f);
            if (f != 0) {
                const float2 w = F.wpack[f];
                const float2 E = c_scale(c_add(a, bc), 0.5f);
                const float2 O = c_mul_mi(c_scale(c_sub(a, bc), 0.5f));
                const float2 tO = c_mul(w, O);
                const float2 Yp = c_mul_mi(c_add(E, tO));             // -i X(f)
                const float2 Ym = c_mul_pi(c_sub(E, tO));             // +i X(f + M)  (negative frequency)
                const float2 S = c_scale(c_add(Yp, Ym), 0.5f);
                const float2 D = c_mul_pi(c_mulc(c_scale(c_sub(Yp, Ym), 0.5f), w));
                out_a = c_add(S, D);
                out_b = c_conj(c_sub(S, D));
            }
            tile[pa] = out_a;
            if (pb != pa) tile[pb] = out_b;
        }
    } else {
        const int half = (L + 1) / 2;                                 // first negative frequency
        for (int p = tid; p < L; p += nthr) {
            const int f = F.p2f[p];
            float h = (f < half) ? 2.f : 0.f;
            if (f == 0 || (2 * f == L)) h = 1.f;
            tile[p] = c_scale(tile[p], h);
        }
    }
}

// One sweep over the L sample pairs of a packed row: kAhead loads load(m) in flight per lane (the sweeps are latency-bound),
// then use(m, pair) for each of them.
template <typename Load, typename Use>
__device__ __forceinline__ void an_pair_sweep(int L, int tid, int nthr, Load load, Use use) {
    constexpr int kAhead = 8;
    for (int m0 = tid; m0 < L; m0 += kAhead * nthr) {
        float2 q[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            const int m = m0 + k * nthr;
            q[k] = (m < L) ? load(m) : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            const int m = m0 + k * nthr;
            if (m < L) use(m, q[k]);
        }
    }
}

// Variance of a row in ONE sweep (analytic.hip row_var): a lane's (count, mean, M2) triples are merged pairwise with the
// parallel update of Chan et al., M2 = M2a + M2b + delta^2 na nb / (na + nb), which has no cancellation at all.
struct VarAcc { double n, mean, m2; };
__device__ __forceinline__ VarAcc var_merge(VarAcc a, VarAcc b) {
    const double n = a.n + b.n;
    if (n == 0.0) return VarAcc{0.0, 0.0, 0.0};
    const double delta = b.mean - a.mean;
    return VarAcc{n, a.mean + delta * (b.n / n), a.m2 + b.m2 + delta * delta * (a.n * b.n / n)};
}

}  // namespace d4w
