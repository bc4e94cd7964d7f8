// Analytic signal of every row on MI355X (gfx950), the transform running in one workgroup's LDS (row_fft.h) -- envelope,
// Hilbert transform, envelope SNR, instantaneous frequency: reference dsp.py:830-856 (instant_freq), dsp.py:956-976
// (snr_tr_array), detect.py:192,217 (pick_times_env / process_corr) -- and dsp.get_fx (dsp.py:18-38).
// HBM-streaming work; no MFMA.  Rows too long for LDS: analytic_long.hip.
#include "analytic_row.h"

namespace d4w {

// ---------------------------------------------------------------------------------------------
// analytic signal of every row  (scipy.signal.hilbert(x, axis=1) = ifft(fft(x) * h))
//
// Even ns (every shape the reference processes): the real row is read as M = ns/2 packed complex
// samples, one M-point FFT gives the half spectrum X(f) after the real-spectrum untangle, the
// Hilbert transform's spectrum is -i X(f) (0 < f < M; 0 at DC and Nyquist, scipy's h = 1 there
// belongs to the real part), and the packed inverse returns H[x] itself; z = x + i H[x].
// Odd ns: plain ns-point complex transform of (x, 0), times h, inverse.  The modes: analytic_row.h.
// ---------------------------------------------------------------------------------------------
template <bool PACKED, bool GENERIC>
__global__ __launch_bounds__(kAnMaxThreads) void analytic_rows(RowFftDev F, const float* __restrict__ x, int ns,
                                                            float* __restrict__ y, int mode,
                                                            const float* __restrict__ var, float fscale) {
    D4W_DYN_LDS(smem_raw);
    float2* tile = reinterpret_cast<float2*>(smem_raw);
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int L = F.ax.L;
    const TwLds tw = tw_stage(row_tw_axis(F), tile + row_tile_elems(F), tid, nthr);
    const float* xr = x + (size_t)blockIdx.x * ns;
    const float2* x2 = reinterpret_cast<const float2*>(xr);           // ns even: 8-byte aligned rows
    auto pair_at = [&](int m) -> float2 { return x2[m]; };
    if (PACKED) {
        an_pair_sweep(L, tid, nthr, pair_at, [&](int m, float2 q) { tile[m] = q; });
    } else {
        for (int n = tid; n < L; n += nthr) tile[n] = make_float2(xr[n], 0.f);
    }
    lds_barrier();
    row_dft<false, GENERIC>(tile, F, tw, tid, nthr);
    an_multiplier<PACKED>(tile, F, tid, nthr);
    lds_barrier();
    row_dft<true, GENERIC>(tile, F, tw, tid, nthr);
    const float scale = 1.0f / (float)L;
    auto zat = [&](int i) -> float2 {
        if (PACKED) {
            const float2 h = tile[i >> 1];
            return make_float2(xr[i], ((i & 1) ? h.y : h.x) * scale);
        }
        return make_float2(xr[i], tile[i].y * scale);                 // the real part of the analytic signal IS the sample: not its
    };                                                                // transformed-and-back copy (off by ~1e-7 max|x|: a row offset)
    if (mode == kAnIfreq) {
        float* yr = y + (size_t)blockIdx.x * (ns - 1);
        for (int i = tid; i < ns - 1; i += nthr) yr[i] = an_ifreq(zat(i), zat(i + 1), fscale);
        return;
    }
    float* yr = y + (size_t)blockIdx.x * ns;
    const float inv_var = (mode == kAnSnr || mode == kAnEnvStd) ? 1.0f / var[blockIdx.x] : 0.f;
    if (PACKED) {
        // two samples per lane: the pair of inputs again (8 bytes), the pair of Hilbert values from the tile, one 8-byte store
        float2* y2 = reinterpret_cast<float2*>(yr);
        auto val = [&](float re, float im) -> float {
            const float p = fmaf(re, re, im * im);
            if (mode == kAnEnvelope) return sqrtf(p);
            if (mode == kAnHilbert) return im;
            if (mode == kAnEnvStd) return sqrtf(p * inv_var);
            return 10.0f * log10f(p * inv_var);
        };
        an_pair_sweep(L, tid, nthr, pair_at, [&](int m, float2 q) {
            const float2 h = tile[m];
            y2[m] = make_float2(val(q.x, h.x * scale), val(q.y, h.y * scale));
        });
        return;
    }
    for (int i = tid; i < ns; i += nthr) {
        const float2 z = zat(i);
        float v;
        if (mode == kAnEnvelope) v = sqrtf(fmaf(z.x, z.x, z.y * z.y));
        else if (mode == kAnHilbert) v = z.y;
        else if (mode == kAnEnvStd) v = sqrtf(fmaf(z.x, z.x, z.y * z.y) * inv_var);
        else v = 10.0f * log10f(fmaf(z.x, z.x, z.y * z.y) * inv_var);
        yr[i] = v;
    }
}

// population variance of every row (np.std(x, axis=1)**2, dsp.py:975-976) in ONE sweep.  Every lane sums d = x - c and d^2 in
// float64 over its share of the row, c = the first sample it meets (its own shift: the shifted-data form is exact enough as
// long as the lane's ~ns / 256 samples are not many orders of magnitude closer to each other than to c); the lanes' (count,
// mean, M2) triples are then merged by var_merge.  Rounds 1-5 swept twice (mean, then centred squares: 2.2 ms per sweep of a
// 20 000 x 120 000 block -- the second sweep of a 480-KB row does not come out of L2).
__global__ __launch_bounds__(kSpThreads) void row_var(const float* __restrict__ x, int ns, float* __restrict__ var) {
    __shared__ double red[3][kSpThreads / 64];
    const float* row = x + (size_t)blockIdx.x * ns;
    const int tid = threadIdx.x;
    double s1 = 0.0, s2 = 0.0, c = 0.0, cnt = 0.0;
    auto take = [&](float v) {
        const double d = (double)v - c;
        s1 += d;
        s2 = fma(d, d, s2);
    };
    if ((ns & 3) == 0 && (reinterpret_cast<uintptr_t>(row) & 15) == 0) {
        const float4* r4 = reinterpret_cast<const float4*>(row);
        const int n4 = ns >> 2;
        if (tid < n4) c = (double)r4[tid].x;
        constexpr int kAhead = 4;                                   // 16-byte loads in flight per lane
        for (int i0 = tid; i0 < n4; i0 += kAhead * kSpThreads) {
            float4 q[kAhead];
#pragma unroll
            for (int k = 0; k < kAhead; ++k) {
                const int i = i0 + k * kSpThreads;
                if (i < n4) q[k] = r4[i];
            }
#pragma unroll
            for (int k = 0; k < kAhead; ++k)
                if (i0 + k * kSpThreads < n4) { take(q[k].x); take(q[k].y); take(q[k].z); take(q[k].w); cnt += 4.0; }
        }
    } else {
        if (tid < ns) c = (double)row[tid];
        for (int i = tid; i < ns; i += kSpThreads) { take(row[i]); cnt += 1.0; }
    }
    VarAcc a{cnt, cnt > 0.0 ? c + s1 / cnt : 0.0, cnt > 0.0 ? fmax(s2 - s1 * s1 / cnt, 0.0) : 0.0};
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        a = var_merge(a, VarAcc{__shfl_xor(a.n, off), __shfl_xor(a.mean, off), __shfl_xor(a.m2, off)});
    if ((tid & 63) == 0) { red[0][tid / 64] = a.n; red[1][tid / 64] = a.mean; red[2][tid / 64] = a.m2; }
    __syncthreads();
    if (tid == 0) {
        VarAcc t{red[0][0], red[1][0], red[2][0]};
        for (int w = 1; w < kSpThreads / 64; ++w) t = var_merge(t, VarAcc{red[0][w], red[1][w], red[2][w]});
        var[blockIdx.x] = (float)(t.m2 / (double)ns);
    }
}

// 10 log10(x^2 / var[row])   (dsp.py:976)
__global__ __launch_bounds__(kSpThreads) void snr_rows(const float* __restrict__ x, int ns,
                                                       const float* __restrict__ var, float* __restrict__ y) {
    const size_t base = (size_t)blockIdx.y * ns;
    const float inv_var = 1.0f / var[blockIdx.y];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += gridDim.x * blockDim.x) {
        const float v = x[base + i];
        y[base + i] = 10.0f * log10f(v * v * inv_var);
    }
}

// ---------------------------------------------------------------------------------------------
// dsp.get_fx: 2 |fftshift(fft(x, nfft), axes=1)| / nfft * 1e9   (dsp.py:35-37)
// np.fft.fft(x, nfft) crops or zero-pads the row to nfft samples.
// ---------------------------------------------------------------------------------------------
template <bool GENERIC>
__global__ __launch_bounds__(kSpThreads) void fx_rows(RowFftDev F, const float* __restrict__ x, int ns,
                                                      float* __restrict__ y) {
    D4W_DYN_LDS(smem_raw);
    float2* tile = reinterpret_cast<float2*>(smem_raw);
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int L = F.ax.L;
    const TwLds tw = tw_stage(row_tw_axis(F), tile + row_tile_elems(F), tid, nthr);
    const float* xr = x + (size_t)blockIdx.x * ns;
    for (int n = tid; n < L; n += nthr) tile[n] = make_float2(n < ns ? xr[n] : 0.f, 0.f);
    lds_barrier();
    row_dft<false, GENERIC>(tile, F, tw, tid, nthr);
    const float scale = (float)(2.0e9 / (double)L);
    float* yr = y + (size_t)blockIdx.x * L;
    const int sh = L / 2;                                             // fftshift: out[j] = F[(j - L//2) mod L]
    for (int j = tid; j < L; j += nthr) {
        int f = j - sh;
        if (f < 0) f += L;
        const float2 v = tile[F.pos[f]];
        yr[j] = sqrtf(fmaf(v.x, v.x, v.y * v.y)) * scale;
    }
}

}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_row_var_f32(const float* x, int nx, int ns, float* var, void* stream) {
    if (!x || !var || nx < 1 || ns < 1) return fail(D4W_EINVAL, "bad argument");
    D4W_LAUNCH(row_var, dim3(nx), dim3(kSpThreads), 0, stream, x, ns, var);
    return D4W_OK;
}

int d4w_analytic_row_fits_lds(int ns) {
    if (ns < 2) return 0;
    return row_tile_bytes(row_fft_tile_elems((ns % 2 == 0) ? ns / 2 : ns)) <= kSpLdsMax ? 1 : 0;
}

int d4w_analytic_f32(const float* x, float* y, int nx, int ns, int mode, const float* var, double fs,
                     void* stream) {
    if (!x || !y || nx < 1 || ns < 2) return fail(D4W_EINVAL, "bad argument");
    if (mode < 0 || mode > 4) return fail(D4W_EINVAL, "mode = %d not in 0..4", mode);
    if ((mode == kAnSnr || mode == kAnEnvStd) && !var) return fail(D4W_EINVAL, "modes 2 and 4 need the row variances");
    const bool packed = (ns % 2 == 0);
    const int L = packed ? ns / 2 : ns;
    const RowFftHost* h = nullptr;
    int rc = row_fft_get(L, &h);
    if (rc) return rc;
    const size_t lds = row_tile_lds(h->dev);
    if (lds > kSpLdsMax)
        return fail(D4W_EINVAL, "rows of %d samples exceed the single-workgroup transform (max %d even / %d odd)",
                    ns, (int)(2 * (kSpLdsMax / 8 - 512)), (int)(kSpLdsMax / 8 - 512));
    const float fscale = (float)(fs / (2.0 * M_PI));
    static const int an_env = [] { const char* v = getenv("D4W_AN_THREADS"); return v ? atoi(v) : 0; }();
    // long rows: 512 threads per row (three 48-KB tiles fit a CU either way: 24 waves instead of 12; 0.69 -> 0.56 ms at
    // 11020 x 12000)
    const int an_threads = (an_env >= 64 && an_env <= kAnMaxThreads && an_env % 64 == 0) ? an_env
                           : (L >= 2048 ? kAnMaxThreads : kSpThreads);
    return with_flags(packed, h->generic, [&](auto P, auto G) {
        constexpr auto kern = analytic_rows<decltype(P)::value, decltype(G)::value>;
        allow_lds(kern, lds);
        D4W_LAUNCH(kern, dim3(nx), dim3(an_threads), lds, stream, h->dev, x, ns, y, mode, var, fscale);
        return (int)D4W_OK;
    });
}

int d4w_snr_f32(const float* x, float* y, int nx, int ns, int env, float* var_ws, void* stream) {
    if (!x || !y || !var_ws || nx < 1 || ns < 2) return fail(D4W_EINVAL, "bad argument");
    int rc = d4w_row_var_f32(x, nx, ns, var_ws, stream);
    if (rc) return rc;
    if (env) return d4w_analytic_f32(x, y, nx, ns, kAnSnr, var_ws, 0.0, stream);
    if (nx > 65535) return fail(D4W_EINVAL, "nx = %d exceeds the grid limit 65535", nx);
    D4W_LAUNCH(snr_rows, dim3(std::min(ceil_div(ns, kSpThreads), 64), nx), dim3(kSpThreads), 0, stream, x, ns,
               (const float*)var_ws, y);
    return D4W_OK;
}

int d4w_fx_f32(const float* x, float* y, int nx, int ns, int nfft, void* stream) {
    if (!x || !y || nx < 1 || ns < 1 || nfft < 1) return fail(D4W_EINVAL, "bad argument");
    const RowFftHost* h = nullptr;
    int rc = row_fft_get(nfft, &h);
    if (rc) return rc;
    const size_t lds = row_tile_lds(h->dev);
    if (lds > kSpLdsMax) return fail(D4W_EINVAL, "nfft = %d exceeds the single-workgroup transform", nfft);
    return with_flag(h->generic, [&](auto G) {
        constexpr auto kern = fx_rows<decltype(G)::value>;
        allow_lds(kern, lds);
        D4W_LAUNCH(kern, dim3(nx), dim3(kSpThreads), lds, stream, h->dev, x, ns, y);
        return (int)D4W_OK;
    });
}

}  // extern "C"
