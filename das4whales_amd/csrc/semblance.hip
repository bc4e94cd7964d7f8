// Local slant-stack semblance (no reference counterpart): for every channel c and sample t the coherence of
// the 2M + 1 neighbouring channels along np trial moveouts, and the moveout that maximises it.  With the delay of trial j at
// neighbour m split on the host into k = floor(d) and a float32 fraction f, X(c, u) = x[c][u] inside the record and 0 outside,
// and the neighbours that are present (0 <= c + m < nx, w_m != 0) taken in increasing m:
//     xi      = v0 + f (v1 - v0),  v0 = X(c + m, tau + k),  v1 = X(c + m, tau + k + 1)        one fmaf
//     b(tau)  = sum_m w_m xi        e(tau) = sum_m w_m xi^2        W = sum_m w_m              one fmaf per term
//     N[t]    = sum_tau b^2,  E[t] = sum_tau e    over tau in [t - H, t + H] and [0, ns)
//     S_j     = N / (W E)  where W E > 0, else 0;     coh = max_j S_j,  idx = the smallest j that attains it
//
// One workgroup of 512 threads owns kSbTc = 4 output channels x kSbTs = 639 output samples; 256 threads work on one channel,
// two channels are in flight at a time (twice the waves over the same staged rectangle).
//   1. It stages the (4 + 2M) x (P3 + kmax - kmin + 1) input rectangle in LDS once (coalesced dword loads, zeros outside the
//      record), P3 = the beam samples the tile needs: its outputs, rounded up to whole threads, plus the 2H halo of the windows.
//   2. For every channel of the tile and every trial j, a thread forms the beam of kSbT = 3 CONSECUTIVE samples: per neighbour
//      it reads 4 words for 3 interpolated values.  Lanes are 3 words apart -- odd, so the 32 lanes of a ds_read_b32 group hit
//      32 banks -- and the neighbour's row and shift move all lanes alike.  Lane l of a wave loads k, f, w of neighbour l - M
//      once per trial and the loop fetches them with v_readlane: no memory latency inside it.
//   3. (b^2, e) go to LDS once as one float2 per beam sample, zero where tau lies outside the record (adding +0 changes no
//      rounding), and the same thread sums the windows of its 3 outputs from 2H + 3 ds_read_b64: the 2H - 1 terms the three
//      windows share are added once (two chains, even and odd terms), then the one or two terms at either end.  Every sum
//      only ever ADDS non-negative terms, in one fixed order: no running sum, no prefix difference, no atomics.
//   4. The maximum over j and its index stay in registers; the cube is written only when asked for.
// One more staged row holds zeros: a neighbour of weight 0 reads it, so that whatever its channel holds (NaNs of a dead
// channel included) stays out of the sums without a branch in the loop (w = 0 times a finite sample adds exactly nothing).
// LDS: (5 + 2M)(P3 + kmax - kmin + 1) + 4 P3 words, at most 145 048 B at the limits (M 16, H 64, |delay| 64); 80 640 B at
// M = 10, H = 25, |delay| < 3, two workgroups = 16 waves per compute unit.
#include <algorithm>

#include "d4w_internal.h"

namespace d4w {
namespace {

constexpr int kSbRow = 256, kSbPar = 2, kSbThreads = kSbRow * kSbPar;   // 256 threads per channel, two channels at a time
constexpr int kSbT = 3, kSbTc = 4, kSbTs = 639;                        // 639 + 2 * 64 = 767 <= 256 * 3 beam samples
constexpr int kSbMaxM = 16, kSbMaxNp = 64, kSbMaxH = 64, kSbMaxDelay = 64;
static_assert(kSbTs % kSbT == 0 && kSbTs + 2 * kSbMaxH <= kSbRow * kSbT && kSbTc % kSbPar == 0,
              "one beam pass covers a tile and its window halo");

struct SbShift { int k; float f; };                                     // one (j, m) of the delay table

struct SbArgs {
    const float* x;             // [nx][pitch]
    float* coh;                 // [nx][ns]
    uint8_t* idx;               // [nx][ns]
    float* cube;                // [np][nx][ns] or NULL
    long long pitch;
    int nx, ns, np, M, H, kmin, kmax, ntile_s;
};

// 8-byte LDS read that stays one ds_read_b64 (256 B/clk): paired into ds_read2_b64 by the compiler it runs at half that rate
__device__ __forceinline__ float2 sb_read2(const float2* p) {
#ifdef D4W_EMU
    return *p;
#else
    typedef float f2_t __attribute__((ext_vector_type(2)));
    typedef const volatile f2_t __attribute__((address_space(3))) * lds_f2_ptr;
    const f2_t v = *(lds_f2_ptr)(p);
    return make_float2(v.x, v.y);
#endif
}

__global__ __launch_bounds__(kSbThreads) void semblance_tile(SbArgs A, const SbShift* __restrict__ tab, const float* __restrict__ w) {
    D4W_DYN_LDS(smem);
    const int tid = threadIdx.x;
    const int tile_c = (int)(blockIdx.x / (unsigned)A.ntile_s);
    const int t0 = ((int)blockIdx.x - tile_c * A.ntile_s) * kSbTs;       // first output sample of the tile
    const int c0 = tile_c * kSbTc;
    const int M = A.M, H = A.H, ns = A.ns, nx = A.nx, n = 2 * M + 1;
    const int nts = min(kSbTs, ns - t0), ntc = min(kSbTc, nx - c0);
    const int P3 = kSbT * ((kSbT * ((nts + kSbT - 1) / kSbT) + 2 * H + kSbT - 1) / kSbT);      // beam samples formed, <= 768
    const int Wd = P3 + (A.kmax - A.kmin) + 1;                           // staged columns: sample t0 - H + kmin + q
    const int rows = ntc + 2 * M;                                        // staged rows: channel c0 - M + r
    float* xs = reinterpret_cast<float*>(smem);
    const int sub = tid & (kSbRow - 1);                                  // position along time
    const int par = __builtin_amdgcn_readfirstlane(tid / kSbRow);        // which of the two channels in flight (the same in a wave)
    float2* pe = reinterpret_cast<float2*>(xs + (((kSbTc + 2 * M + 1) * Wd + 1) & ~1)) + par * P3;      // (b^2, e) of the P3 beam samples

    // ---- 1. stage the input rectangle
    const int u0 = t0 - H + A.kmin;
    for (int r = 0; r < rows; ++r) {
        const int ch = c0 - M + r;
        const bool row_in = ch >= 0 && ch < nx;
        const float* xr = A.x + (size_t)(row_in ? ch : 0) * (size_t)A.pitch;
        float* dst = xs + r * Wd;
        for (int q = tid; q < Wd; q += kSbThreads) {
            const int u = u0 + q;
            dst[q] = (row_in && u >= 0 && u < ns) ? xr[u] : 0.f;
        }
    }
    for (int q = tid; q < Wd; q += kSbThreads) xs[(kSbTc + 2 * M) * Wd + q] = 0.f;          // the row of zeros
    __syncthreads();

    const int p0 = kSbT * sub;                                           // the thread's beam samples p0 .. p0 + 2 and outputs alike
    const bool beam_on = p0 < P3, out_on = p0 < nts;
#ifndef D4W_EMU
    const int lane = tid & 63;
    const float my_w = lane < n ? w[lane] : 0.f;
#endif
    bool in_rec[kSbT];
#pragma unroll
    for (int i = 0; i < kSbT; ++i) {
        const int tau = t0 - H + p0 + i;
        in_rec[i] = tau >= 0 && tau < ns;
    }
    for (int cl = par; cl < kSbTc; cl += kSbPar) {                       // (every thread makes every trip: the barriers inside)
        const int c = c0 + cl;
        const bool c_on = cl < ntc;
        const int off_zero = (kSbTc + M - cl) * Wd + A.kmin;             // the row of zeros: what a neighbour of weight 0 reads
        const int m_lo = max(-M, -c), m_hi = min(M, nx - 1 - c);         // the neighbours inside the cable
        float Wsum = 0.f;
        for (int m = m_lo; m <= m_hi; ++m) Wsum += w[m + M];             // (w = 0: absent, adds nothing)
        float best[kSbT];
        int arg[kSbT];
#pragma unroll
        for (int i = 0; i < kSbT; ++i) { best[i] = 0.f; arg[i] = 0; }
        for (int j = 0; j < A.np; ++j) {
            // ---- 2. the beam of three consecutive samples.  Lane l of every wave holds (row and sample shift, f) of neighbour
            // l - M for this trial, and w; the loop fetches them with v_readlane (no memory latency inside it)
#ifndef D4W_EMU
            int my_off = 0;
            float my_f = 0.f;
            if (lane < n) {
                const SbShift s = tab[j * n + lane];
                my_off = my_w == 0.f ? off_zero : (lane - M) * Wd + s.k;  // (absent: its samples, NaNs included, are not read)
                my_f = s.f;
            }
#endif
            if (beam_on && c_on) {
                float b[kSbT], e[kSbT];
#pragma unroll
                for (int i = 0; i < kSbT; ++i) { b[i] = 0.f; e[i] = 0.f; }
                const float* base = xs + (cl + M) * Wd + p0 - A.kmin;
                auto fetch = [&](int mm, float (&v)[kSbT + 1], float& fm, float& wm) {
#ifdef D4W_EMU
                    wm = w[mm]; fm = tab[j * n + mm].f;
                    const int off = wm == 0.f ? off_zero : (mm - M) * Wd + tab[j * n + mm].k;
#else
                    wm = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), mm));
                    fm = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_f), mm));
                    const int off = __builtin_amdgcn_readlane(my_off, mm);
#endif
#pragma unroll
                    for (int i = 0; i <= kSbT; ++i) v[i] = base[off + i];
                };
                auto accum = [&](const float (&v)[kSbT + 1], float fm, float wm) {
#pragma unroll
                    for (int i = 0; i < kSbT; ++i) {
                        const float xi = fmaf(fm, v[i + 1] - v[i], v[i]);
                        b[i] = fmaf(wm, xi, b[i]);
                        e[i] = fmaf(wm * xi, xi, e[i]);
                    }
                };
                int mm = m_lo + M;
                const int mm_hi = m_hi + M;
                for (; mm + 3 <= mm_hi; mm += 4) {                       // four neighbours' reads in flight, summed in order
                    float v0[kSbT + 1], v1[kSbT + 1], v2[kSbT + 1], v3[kSbT + 1], f0, f1, f2, f3, w0, w1, w2, w3;
                    fetch(mm, v0, f0, w0); fetch(mm + 1, v1, f1, w1); fetch(mm + 2, v2, f2, w2); fetch(mm + 3, v3, f3, w3);
                    accum(v0, f0, w0); accum(v1, f1, w1); accum(v2, f2, w2); accum(v3, f3, w3);
                }
                for (; mm <= mm_hi; ++mm) {
                    float v0[kSbT + 1], f0, w0;
                    fetch(mm, v0, f0, w0);
                    accum(v0, f0, w0);
                }
#pragma unroll
                for (int i = 0; i < kSbT; ++i) pe[p0 + i] = in_rec[i] ? make_float2(b[i] * b[i], e[i]) : make_float2(0.f, 0.f);
            }
            __syncthreads();
            // ---- 3. the windows of three consecutive outputs: terms q = 0 .. 2H + 2, output i sums q = i .. i + 2H
            if (out_on && c_on) {
                const float2* q = pe + p0;
                float N[kSbT], E[kSbT];
                if (H == 0) {
#pragma unroll
                    for (int i = 0; i < kSbT; ++i) { N[i] = q[i].x; E[i] = q[i].y; }
                } else {
                    float2 ca = q[2], cb = make_float2(0.f, 0.f);        // the shared terms 2 .. 2H: even ones, odd ones
                    for (int u = 3; u < 2 * H; u += 2) {
                        const float2 o = sb_read2(q + u), v = sb_read2(q + u + 1);
                        cb.x += o.x; cb.y += o.y;
                        ca.x += v.x; ca.y += v.y;
                    }
                    const float2 core = make_float2(ca.x + cb.x, ca.y + cb.y);
                    const float2 l0 = q[0], l1 = q[1], r0 = q[2 * H + 1], r1 = q[2 * H + 2];
                    N[0] = (l0.x + l1.x) + core.x;  E[0] = (l0.y + l1.y) + core.y;
                    N[1] = (l1.x + core.x) + r0.x;  E[1] = (l1.y + core.y) + r0.y;
                    N[2] = core.x + (r0.x + r1.x);  E[2] = core.y + (r0.y + r1.y);
                }
#pragma unroll
                for (int i = 0; i < kSbT; ++i) {
                    const float den = Wsum * E[i];
                    const float S = den > 0.f ? N[i] / den : 0.f;
                    if (S > best[i]) { best[i] = S; arg[i] = j; }
                    if (A.cube && p0 + i < nts) A.cube[((size_t)j * nx + c) * (size_t)ns + t0 + p0 + i] = S;
                }
            }
            __syncthreads();                                             // pe is rewritten by the next trial
        }
        if (out_on && c_on) {
            const size_t o = (size_t)c * ns + t0 + p0;
#pragma unroll
            for (int i = 0; i < kSbT; ++i)
                if (p0 + i < nts) { A.coh[o + i] = best[i]; A.idx[o + i] = (uint8_t)arg[i]; }
        }
    }
}

size_t sb_lds_bytes(int M, int H, int nts, int kmin, int kmax) {
    const int P3 = kSbT * ((kSbT * ceil_div(nts, kSbT) + 2 * H + kSbT - 1) / kSbT);
    const int Wd = P3 + (kmax - kmin) + 1;
    return (size_t)(((kSbTc + 2 * M + 1) * Wd + 1) & ~1) * sizeof(float) + (size_t)kSbPar * P3 * sizeof(float2);
}

}  // namespace
}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_semblance_limits(int* max_half_aperture, int* max_slownesses, int* max_half_window, int* max_abs_delay) {
    if (max_half_aperture) *max_half_aperture = kSbMaxM;
    if (max_slownesses) *max_slownesses = kSbMaxNp;
    if (max_half_window) *max_half_window = kSbMaxH;
    if (max_abs_delay) *max_abs_delay = kSbMaxDelay;
    return D4W_OK;
}

int d4w_semblance_tile(int* channels, int* samples) {
    if (channels) *channels = kSbTc;
    if (samples) *samples = kSbTs;
    return D4W_OK;
}

int d4w_semblance_f32(const float* x, int64_t pitch, int nx, int ns, const int32_t* k, const float* f, int np, int M, const float* w,
                      int H, float* coh, uint8_t* idx, float* cube, void* stream) {
    if (!x || !k || !f || !w || !coh || !idx) return fail(D4W_EINVAL, "bad argument (x, k, f, w, coh and idx are needed)");
    if (nx < 1 || ns < 1 || pitch < ns) return fail(D4W_EINVAL, "nx = %d, ns = %d, pitch = %lld (nx, ns >= 1, pitch >= ns)", nx, ns, (long long)pitch);
    if (M < 1 || M > kSbMaxM) return fail(D4W_EINVAL, "half aperture M = %d outside 1..%d", M, kSbMaxM);
    if (np < 1 || np > kSbMaxNp) return fail(D4W_EINVAL, "%d trial slownesses outside 1..%d", np, kSbMaxNp);
    if (H < 0 || H > kSbMaxH) return fail(D4W_EINVAL, "half window H = %d outside 0..%d", H, kSbMaxH);
    const int n = 2 * M + 1;
    for (int m = 0; m < n; ++m)
        if (!(w[m] >= 0.f) || !std::isfinite(w[m])) return fail(D4W_EINVAL, "weight %d is negative or not finite", m);
    if (!(w[M] > 0.f)) return fail(D4W_EINVAL, "the centre weight must be > 0");
    std::vector<unsigned char> host((size_t)np * n * sizeof(SbShift) + (size_t)n * sizeof(float));
    SbShift* tab = reinterpret_cast<SbShift*>(host.data());
    int kmin = 0, kmax = 0;
    for (int j = 0; j < np; ++j)
        for (int m = 0; m < n; ++m) {
            const int kk = k[j * n + m];
            const float ff = f[j * n + m];
            if (!(ff >= 0.f && ff < 1.f)) return fail(D4W_EINVAL, "fraction [%d][%d] = %g outside [0, 1)", j, m, (double)ff);
            if (kk < -kSbMaxDelay || kk > kSbMaxDelay || (kk == kSbMaxDelay && ff > 0.f))
                return fail(D4W_EINVAL, "delay [%d][%d] = %d + %g outside +-%d samples", j, m, kk, (double)ff, kSbMaxDelay);
            if (m == M && (kk != 0 || ff != 0.f)) return fail(D4W_EINVAL, "delay [%d][centre] must be 0", j);
            tab[j * n + m] = SbShift{kk, ff};
            kmin = std::min(kmin, kk);
            kmax = std::max(kmax, kk);
        }
    memcpy(host.data() + (size_t)np * n * sizeof(SbShift), w, (size_t)n * sizeof(float));
    SbArgs A;
    A.x = x; A.coh = coh; A.idx = idx; A.cube = cube; A.pitch = (long long)pitch;
    A.nx = nx; A.ns = ns; A.np = np; A.M = M; A.H = H; A.kmin = kmin; A.kmax = kmax;
    A.ntile_s = ceil_div(ns, kSbTs);
    const long long blocks = (long long)ceil_div(nx, kSbTc) * A.ntile_s;
    if (blocks > 0x7FFFFFFFLL) return fail(D4W_EINVAL, "%d x %d: more tiles than one launch holds", nx, ns);
    const size_t lds = sb_lds_bytes(M, H, std::min(ns, kSbTs), kmin, kmax);
    void* dtab = nullptr;
#ifdef D4W_EMU
    dtab = malloc(host.size());
    if (!dtab) return fail(D4W_ENOMEM, "out of memory");
    memcpy(dtab, host.data(), host.size());
#else
    // the table lives for this call only, in stream order (no workspace argument, no state between calls)
    D4W_HIP(hipMallocAsync(&dtab, host.size(), (hipStream_t)stream));
    hipError_t e = hipMemcpyAsync(dtab, host.data(), host.size(), hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e == hipSuccess && lds > 64 * 1024)
        e = hipFuncSetAttribute((const void*)semblance_tile, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
        (void)hipFreeAsync(dtab, (hipStream_t)stream);
        return fail(D4W_EHIP, "table upload failed: %s", hipGetErrorString(e));
    }
#endif
    const SbShift* d_tab = reinterpret_cast<const SbShift*>(dtab);
    const float* d_w = reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(dtab) + (size_t)np * n * sizeof(SbShift));
    hipLaunchKernelGGL(semblance_tile, dim3((unsigned)blocks), dim3(kSbThreads), lds, (hipStream_t)stream, A, d_tab, d_w);
#ifdef D4W_EMU
    free(dtab);
#else
    const hipError_t el = hipGetLastError();
    (void)hipFreeAsync(dtab, (hipStream_t)stream);
    if (el != hipSuccess) return fail(D4W_EHIP, "semblance launch failed: %s", hipGetErrorString(el));
#endif
    return D4W_OK;
}

}  // extern "C"
