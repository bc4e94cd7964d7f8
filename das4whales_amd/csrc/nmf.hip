// Window-normalised matched filter (NMF): the second pass that turns the correlograms of the matched filter (xcorr_mm.hip and
// its siblings, untouched) into correlation coefficients in [-1, 1] -- every lag divided by the energy of the data that lies
// under the template AT THAT LAG instead of by the row's loudest sample.  For a row x of ns samples, a
// template support of m taps h' (de-meaned over the support), the row's mean mu and A = max|x|:
//     x'[i]  = (x[i] - mu) / A                      i < ns   (the correlator's own normalised samples, float32)
//            = (head[i - ns] - mu) / A              ns <= i < ns + n_next  (the record's continuation), 0 beyond: zeros are data
//     S1[k]  = sum_{n < m} x'[k + n],   S2[k] = sum_{n < m} x'[k + n]^2
//     V[k]   = S2 - S1^2 / m  (center)  or  S2
//     y[k]  <- y[k] / (|h'| sqrt(V[k]))  where V[k] > floor^2 m,  0 elsewhere
//
// One workgroup = one tile of kNmfTile lags of one row, both templates: x is read ONCE for the pair (m0 != m1 allowed), every
// correlogram is read and written once with 16 bytes per lane (20 B per sample for a pair against the correlator's 12).
//
// Numerics.  The windowed sums are float64 and never a float32 running sum: on a row of offset 200 + ramp +-50 + unit noise
// S2 - S1^2 / m cancels six digits.  A float64 PREFIX over the tile would do for such rows but carries the rounding of
// everything since the tile's start into a window that may hold nothing (a dropout, a constant stretch: V must come out
// below floor^2 m = 1e-12 m there, while ulp(sum of a tile) is 1e-12 for m = 1).  So the sums SLIDE and are re-anchored:
//   1. the tile's samples plus the m - 1 halo are staged in LDS as float32 x', in runs of kNmfRun = 8 (one pad word per run:
//      lanes that own consecutive runs read words 9 apart -- odd, so the 32 lanes of a ds_read_b32 group hit 32 banks);
//   2. float64 sums (sum, sum of squares) of every run;
//   3. a thread owns the 8 lags of one run.  Its first window is the sum of the m / 8 WHOLE run sums it covers plus the
//      m % 8 samples behind them -- every term a part of the window itself, so the error is relative to what the window
//      holds --, then 7 slides  S1 += b - a,  S2 += b^2 - a^2  (b - a, a^2, b^2 exact in float64).  After 7 slides the error is
//      at most 7 ulp of the largest S2 of the run <= 4 m:  7 * 4 m * 2^-52 = 6e-15 m, 0.6 % of floor^2 m at the default floor.
// The final scale is float32: V rounded once, v_sqrt_f32, one product, one division.
#include "d4w_internal.h"
#include "mm_common.h"

namespace d4w {
namespace {

constexpr int kNmfThreads = 256, kNmfRun = 8, kNmfTile = kNmfThreads * kNmfRun;     // 2048 lags per workgroup
constexpr int kNmfMaxSupport = 7936;                                                // = d4w_xcorr_mm_max_support()

struct NmfArgs {
    const float* x;         // [nx][ns]
    const float* xnext;     // [nx][ld_next] or NULL: the head of the next file, read in place
    const double* mean;     // [nx] float64 row means (d4w_row_stats_f32)
    const float* maxabs;    // [nx] row maxima
    float* y0;              // [nx][ns] correlogram of template 0, normalised in place
    float* y1;              // ... of template 1 (NT == 2)
    float* rowmax0;         // [nx] or NULL: max over the lags of every normalised row (-inf from the host, mm_atomic_fmax)
    float* rowmax1;
    int nx, ns, ld_next, n_next, ntile, nr;       // nr: runs staged per tile
    int m0, m1;
    double cm0, cm1;        // 1 / m (center) or 0
    double thr0, thr1;      // floor^2 m; +inf for a template without shape (|h'| = 0): every lag 0
    float hn0, hn1;         // |h'|
};

__device__ __forceinline__ int nmf_at(int i) { return i + (i >> 3); }              // sample i of the stage, one pad word per run

template <int NT>
__global__ __launch_bounds__(kNmfThreads) void nmf_rows(NmfArgs P) {
    D4W_DYN_LDS(smem);
    const int tid = threadIdx.x;
    const int row = (int)(blockIdx.x / (unsigned)P.ntile);
    const int t0 = ((int)blockIdx.x - row * P.ntile) * kNmfTile;                    // first lag (= first sample) of the tile
    const int ns = P.ns;
    const int nlag = min(kNmfTile, ns - t0);
    const int mmax = (NT == 2) ? max(P.m0, P.m1) : P.m0;
    const int nrun = (nlag + mmax - 1 + kNmfRun - 1) / kNmfRun;                     // runs this tile needs, <= P.nr
    double* rs1 = reinterpret_cast<double*>(smem);
    double* rs2 = rs1 + P.nr;
    float* xs = reinterpret_cast<float*>(rs2 + P.nr);

    // ---- 1. stage the normalised samples: ((x - hi) - lo) g as the correlator forms them (xcorr_mm.hip), zeros beyond the data
    const Mean2 mu = mean2_load(P.mean, row);
    const float a = P.maxabs[row];
    const float g = (a > 0.f) ? 1.0f / a : 0.f;
    const float mlg = -mu.lo * g;
    const float* xr = P.x + (size_t)row * ns;
    const float* xn = P.xnext ? P.xnext + (size_t)row * P.ld_next : nullptr;
    const int n_data = ns + (xn ? P.n_next : 0);
    auto sample = [&](int gi) -> float {                                            // x' of sample gi of the row and its extension
        if (gi >= n_data) return 0.f;
        const float v = (gi < ns) ? xr[gi] : xn[gi - ns];
        return fmaf(v - mu.hi, g, mlg);
    };
    const bool x_al = (reinterpret_cast<uintptr_t>(xr + t0) & 15) == 0;
    for (int q = tid; q < nrun * (kNmfRun / 4); q += kNmfThreads) {                 // 16 bytes per lane inside the row
        const int i = 4 * q, gi = t0 + i;
        float s0, s1, s2, s3;
        if (x_al && gi + 4 <= ns) {
            const float4 v = *reinterpret_cast<const float4*>(xr + gi);
            s0 = fmaf(v.x - mu.hi, g, mlg); s1 = fmaf(v.y - mu.hi, g, mlg); s2 = fmaf(v.z - mu.hi, g, mlg); s3 = fmaf(v.w - mu.hi, g, mlg);
        } else {
            s0 = sample(gi); s1 = sample(gi + 1); s2 = sample(gi + 2); s3 = sample(gi + 3);
        }
        float* p = xs + nmf_at(i);                                                  // (4 | i: the four lie in one run)
        p[0] = s0; p[1] = s1; p[2] = s2; p[3] = s3;
    }
    __syncthreads();

    // ---- 2. float64 sums of every run
    for (int r = tid; r < nrun; r += kNmfThreads) {
        const float* p = xs + r * (kNmfRun + 1);
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int j = 0; j < kNmfRun; ++j) {
            const double v = (double)p[j];
            s1 += v;
            s2 = fma(v, v, s2);
        }
        rs1[r] = s1;
        rs2[r] = s2;
    }
    __syncthreads();

    // ---- 3. the thread's 8 lags: anchor from the run sums, slide, scale
    const int k0 = kNmfRun * tid;
    const bool active = k0 < nlag;
    const float* own = xs + tid * (kNmfRun + 1);
    auto one = [&](float* yrow, int m, double cm, double thr, float hn) -> float {
        float vmax = -INFINITY;
        if (!active) return vmax;
        float* yp = yrow + (size_t)row * ns + t0 + k0;
        const bool vec = k0 + kNmfRun <= nlag && (reinterpret_cast<uintptr_t>(yp) & 15) == 0;
        float c[kNmfRun];
        if (vec) {
            const float4 u = *reinterpret_cast<const float4*>(yp), w = *reinterpret_cast<const float4*>(yp + 4);
            c[0] = u.x; c[1] = u.y; c[2] = u.z; c[3] = u.w; c[4] = w.x; c[5] = w.y; c[6] = w.z; c[7] = w.w;
        } else {
#pragma unroll
            for (int j = 0; j < kNmfRun; ++j) c[j] = (k0 + j < nlag) ? yp[j] : 0.f;
        }
        const int q = m / kNmfRun, rem = m - q * kNmfRun;
        double S1 = 0.0, S2 = 0.0;
        for (int u = 0; u < q; ++u) {
            S1 += rs1[tid + u];
            S2 += rs2[tid + u];
        }
        const float* pr = xs + (tid + q) * (kNmfRun + 1);
        for (int j = 0; j < rem; ++j) {
            const double v = (double)pr[j];
            S1 += v;
            S2 = fma(v, v, S2);
        }
#pragma unroll
        for (int j = 0; j < kNmfRun; ++j) {
            const double V = fma(-S1 * cm, S1, S2);
            float o = 0.f;
            if (V > thr) o = c[j] / (hn * sqrtf((float)V));
            c[j] = o;
            if (k0 + j < nlag) vmax = fmaxf(vmax, o);
            if (j + 1 < kNmfRun && k0 + j + 1 < nlag) {                             // (no lag behind the row: nothing staged for it)
                const double va = (double)own[j], vb = (double)xs[nmf_at(k0 + j + m)];
                S1 += vb - va;
                S2 = fma(vb, vb, S2);
                S2 = fma(-va, va, S2);
            }
        }
        if (vec) {
            mm_store4(yp, c[0], c[1], c[2], c[3]);
            mm_store4(yp + 4, c[4], c[5], c[6], c[7]);
        } else {
#pragma unroll
            for (int j = 0; j < kNmfRun; ++j)
                if (k0 + j < nlag) yp[j] = c[j];
        }
        return vmax;
    };
    float v0 = one(P.y0, P.m0, P.cm0, P.thr0, P.hn0);
    float v1 = -INFINITY;
    if constexpr (NT == 2) v1 = one(P.y1, P.m1, P.cm1, P.thr1, P.hn1);

    // ---- the rows' maxima of the normalised values (detect.correlogram_max / Threshold): one atomic pair per wave
    if (P.rowmax0) {                                                                // (a kernel argument: every wave alike)
        for (int o = 32; o > 0; o >>= 1) {
            v0 = fmaxf(v0, __shfl_xor(v0, o));
            if constexpr (NT == 2) v1 = fmaxf(v1, __shfl_xor(v1, o));
        }
        if ((tid & 63) == 0 && kNmfTile / 4 * (tid >> 6) < nlag) {                  // the wave holds a lag of the row
            mm_atomic_fmax(P.rowmax0 + row, v0);
            if constexpr (NT == 2) mm_atomic_fmax(P.rowmax1 + row, v1);
        }
    }
}

template <int NT>
int nmf_launch(const NmfArgs& P, void* stream) {
    const size_t lds = (size_t)P.nr * (2 * sizeof(double) + (kNmfRun + 1) * sizeof(float));
    auto kern = nmf_rows<NT>;
    if (lds > 64 * 1024) D4W_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    D4W_LAUNCH(kern, dim3((unsigned)((long long)P.nx * P.ntile)), dim3(kNmfThreads), lds, stream, P);
    return D4W_OK;
}

}  // namespace
}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_nmf_max_support(void) { return kNmfMaxSupport; }

int d4w_nmf_tile(void) { return kNmfTile; }

int d4w_nmf_normalise_f32(const float* x, int nx, int ns, const float* xnext, int ld_next, int n_next, const double* mean,
                          const float* maxabs, int ntpl, int len0, int len1, double norm0, double norm1, int center, double floor,
                          float* y0, float* y1, float* rowmax0, float* rowmax1, void* stream) {
    if (!x || !y0 || !mean || !maxabs || nx < 1 || ns < 1) return fail(D4W_EINVAL, "bad argument (x, y0, mean and maxabs are needed; nx, ns >= 1)");
    if (ntpl < 1 || ntpl > 2 || (ntpl == 2 && !y1)) return fail(D4W_EINVAL, "ntpl = %d (1 or 2 correlograms per call)", ntpl);
    if (ntpl == 2 && ((rowmax0 == nullptr) != (rowmax1 == nullptr))) return fail(D4W_EINVAL, "rowmax0 and rowmax1 go together");
    if (xnext && (n_next < 0 || ld_next < n_next)) return fail(D4W_EINVAL, "a continuation needs 0 <= n_next <= ld_next");
    if (ntpl == 1) { len1 = len0; norm1 = norm0; }
    if (len0 < 1 || len1 < 1 || std::max(len0, len1) > kNmfMaxSupport)
        return fail(D4W_EINVAL, "template supports (%d, %d) must lie in 1..%d", len0, len1, kNmfMaxSupport);
    if (!(norm0 >= 0.0) || !(norm1 >= 0.0) || !std::isfinite(norm0) || !std::isfinite(norm1))
        return fail(D4W_EINVAL, "the templates' norms must be finite and >= 0");
    if (!(floor >= 0.0) || !std::isfinite(floor)) return fail(D4W_EINVAL, "floor must be finite and >= 0");
    if (center != 0 && center != 1) return fail(D4W_EINVAL, "center = %d (0 or 1)", center);
    NmfArgs P;
    P.x = x; P.xnext = (xnext && n_next > 0) ? xnext : nullptr; P.mean = mean; P.maxabs = maxabs;
    P.y0 = y0; P.y1 = (ntpl == 2) ? y1 : nullptr; P.rowmax0 = rowmax0; P.rowmax1 = (ntpl == 2) ? rowmax1 : nullptr;
    P.nx = nx; P.ns = ns; P.ld_next = ld_next; P.n_next = P.xnext ? n_next : 0;
    P.ntile = ceil_div(ns, kNmfTile);
    if ((long long)nx * P.ntile > 0x7FFFFFFFLL) return fail(D4W_EINVAL, "%d rows of %d samples: more tiles than one launch holds", nx, ns);
    P.nr = ceil_div(std::min(ns, kNmfTile) + std::max(len0, len1) - 1, kNmfRun);
    P.m0 = len0; P.m1 = len1;
    P.cm0 = center ? 1.0 / len0 : 0.0; P.cm1 = center ? 1.0 / len1 : 0.0;
    // a template without shape (|h'| = 0: one tap, a constant) correlates to 0 with everything: every lag 0, never 0 / 0
    P.thr0 = norm0 > 0.0 ? floor * floor * len0 : INFINITY; P.thr1 = norm1 > 0.0 ? floor * floor * len1 : INFINITY;
    P.hn0 = (float)norm0; P.hn1 = (float)norm1;
    if (rowmax0) {                                                  // -inf: the identity of the integer-atomic float max
        D4W_HIP(hipMemsetD32Async((hipDeviceptr_t)rowmax0, (int)0xFF800000u, (size_t)nx, (hipStream_t)stream));
        if (ntpl == 2) D4W_HIP(hipMemsetD32Async((hipDeviceptr_t)rowmax1, (int)0xFF800000u, (size_t)nx, (hipStream_t)stream));
    }
    return ntpl == 2 ? nmf_launch<2>(P, stream) : nmf_launch<1>(P, stream);
}

}  // extern "C"
