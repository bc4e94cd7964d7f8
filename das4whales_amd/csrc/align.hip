// Arrival times refined against the beam on MI355X (gfx950): every channel correlated with the call's own waveform over a few
// lags around the predicted moveout, the lag of the largest coefficient and a parabola through its neighbours.  The step after
// beam.hip in dw.loc: locate -> beam -> re-pick against the beam -> relocate; beyond the reference, which has
// nothing of the kind.  xcorr_mm.hip and nmf.hip correlate every row with one shared template over all lags; this takes one
// template per call, one window per (call, channel) and 2M + 1 lags.
//
//   n0 = start[c] + r[c][ch]                              int64; start clamped to +-2^62 as in beam.hip, r = moveout_round(tau)
//   for m in [-M, M], valid iff 0 <= n0 + m and n0 + m + L <= ns + ns_next      (sample ns + i of a row is xnext[ch][i])
//     dot[m] = sum_j t[c][j] x[ch][n0 + m + j],   en[m] = sum_j x[ch][n0 + m + j]^2,   tn[c] = sum_j t[c][j]^2
//     rho[m] = dot / sqrtf(tn en), 0 where tn or en is 0, NaN where the lag is not valid (a NaN sample makes its lags NaN)
//   m* = the lag of the largest non-NaN rho, the smallest of equals;  coef = rho[m*]
//   delta = 0.5 (a - c) / ((a - 2 b) + c) clipped to +-0.5, in float64 from the float32 a, b, c = rho[m* - 1 .. m* + 1], where both
//     neighbours exist and are not NaN and the denominator is negative; else 0
//   Ti[c][ch] = ((double)(n0 + m*) + delta) / fs;  NaN with weights[ch] = 0, without a valid lag, or with coef < min_coef
//
// Sum order, a function of L alone.  dot[m] and en[m] are one chain each, from 0, over j = 0 .. L - 1 in increasing order, one
// fmaf per term.  tn is 64 interleaved chains (chain i takes j = i, i + 64, ... in increasing order, fmaf from 0), added
// pairwise at distances 32, 16, 8, 4, 2, 1.  Every product of a sample with a power of two is exact, so rho keeps its bits
// under a power-of-two scaling of x or of the template, and an entry depends on its own (call, channel) alone: run-to-run
// bit-identical, independent of the rest of the batch.
//
// align_pick: grid (ceil(nch / 4), ncalls), one wave of 64 threads for four channels of one call, 16 lanes per channel.  The
//   template goes into LDS once per workgroup (and tn with it); the 16 lanes of a channel stage its window of L + 2M samples
//   in 64-byte runs of the row, the four channels' loads in flight together (staging them one after the other, each by the
//   whole wave, cost 11 %: four dependent trips to memory per workgroup instead of one).  A window is classified once, as
//   beam_sum does it: wholly inside the block or wholly inside the next one is a plain copy from that row's pointer; across
//   the seam or an end of the record every sample is tested (what lies outside is staged as 0 and reaches invalid lags only).
//   Register window: a lane owns 4 consecutive lags (64 lags per channel and pass; passes for
//   2M + 1 > 64).  Per four taps a lane reads one 16-byte word of its window (it keeps the previous one: 8 consecutive samples
//   serve 4 taps x 4 lags) and one 16-byte broadcast word of the template: 8 floats per 16 terms where a lane per lag reads 20,
//   and as 16-byte reads a sixth of the LDS cycles; every chain still in increasing j.  The window rows start 64 words apart modulo 64, so the 16-byte reads of a lane group
//   fall on distinct banks.  Samples past a channel's window are never staged: they reach only lags beyond 2M, which are not
//   stored.  rho goes to LDS (and to the table when asked for); the pick reads those floats back: a scan per lane, a reduction
//   over the 16 lanes of the channel, and the first of them fits the parabola.  No atomics.  A channel of weight 0 is never
//   read.
//   Dynamic LDS: 4 (L4 + 4 Ws + 4 (2M + 1)) bytes, L4 = L rounded up to 4, Ws = 64 ceil((2M + 1) / 64) + L4 rounded up to 64:
//   10.4 KB at L = 400, M = 20 (15 workgroups per compute unit) and 96 KB at the limits L = 4096, M = 255 (one).
//   Compiler's report (gfx950, -Rpass-analysis=kernel-resource-usage): 61 VGPRs, 64 SGPRs, no scratch, 8 waves per SIMD by
//   registers; the plain form had 48 VGPRs and 67 SGPRs.
//
// Cost model: ncalls nch (2M + 1) L terms, two multiply-adds each; ncalls nch (L + 2M) words read from the block, mostly L2
//   hits across the calls.  The plain form (a wave per channel, a lane per lag, one LDS word per term) was built first and
//   measured: 1.78 ms for 64 calls at 11 020 channels, L = 400, M = 20, by its count bound by the LDS read rate; this form takes
//   1.10 ms, its LDS cycles are a sixth and the multiply-adds the same (profiles/align/).
#include "taps.h"

#ifndef D4W_EMU
#pragma clang fp contract(off)
#endif

namespace d4w {

constexpr int kAlignThreads = 64;                            // one wave
constexpr int kAlignChannels = 4;                            // channels per workgroup
constexpr int kAlignGroup = kAlignThreads / kAlignChannels;  // lanes per channel
constexpr int kAlignRun = 4;                                 // consecutive lags per lane
constexpr int kAlignPass = kAlignGroup * kAlignRun;          // lags per channel and pass
constexpr int kAlignMaxCalls = 65535;                        // grid limit
constexpr int kAlignMaxLength = 4096;                        // 20 s at 200 Hz
constexpr int kAlignMaxLag = 255;
constexpr int kAlignNone = 0x7fffffff;                       // "no lag yet" in the argmax

static inline int align_row_words(int L, int M) {            // a window row in LDS: every 16-byte read of a pass stays inside it
    return (kAlignPass * ceil_div(2 * M + 1, kAlignPass) + ((L + 3) & ~3) + 63) & ~63;
}

static inline size_t align_lds_bytes(int L, int M) {
    return sizeof(float) * ((size_t)((L + 3) & ~3) + (size_t)kAlignChannels * align_row_words(L, M) + (size_t)kAlignChannels * (2 * M + 1));
}

// grid (ceil(nch / 4), ncalls).  tmpl [ncalls][L]; r [ncalls][nch]; Ti, coef, lag [ncalls][nch]; rho [ncalls][nch][2M + 1];
// lag and rho each or NULL; Ws = align_row_words(L, M)
__global__ __launch_bounds__(kAlignThreads) void align_pick(const float* __restrict__ x, long long pitch, int nch, int ns,
                                                            const float* __restrict__ xn, long long pitchn, int nsn,
                                                            const float* __restrict__ tmpl, int L, const int* __restrict__ r,
                                                            const long long* __restrict__ start, int M, int Ws,
                                                            const float* __restrict__ weights, double fs, double min_coef, int subsample,
                                                            double* __restrict__ Ti, float* __restrict__ coef, int* __restrict__ lag,
                                                            float* __restrict__ rho) {
    D4W_DYN_LDS(smem);
    const int Wn = L + 2 * M, nl = 2 * M + 1, L4 = L & ~3;
    const int lane = threadIdx.x, kk = lane / kAlignGroup, g = lane % kAlignGroup;
    float* tl = reinterpret_cast<float*>(smem);              // the template, 16-byte aligned
    float* win = tl + ((L + 3) & ~3);                        // four window rows of Ws words
    float* rl = win + (size_t)kAlignChannels * Ws + (size_t)kk * nl;         // this lane's channel's rho
    const int c = blockIdx.y;
    const long long ch0 = (long long)blockIdx.x * kAlignChannels;
    const long long ntot = (long long)ns + (long long)nsn;
    const long long s0 = clamp_start(start[c]);
    const float qnan = __int_as_float(0x7fc00000);

    const float* __restrict__ t = tmpl + (size_t)c * (size_t)L;
    float tn = 0.f;
    for (int j = lane; j < L; j += kAlignThreads) {
        const float v = t[j];
        tl[j] = v;
        tn = fmaf(v, v, tn);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) tn += __shfl_xor(tn, s);

    // a channel: 0 = no such channel, 1 = no pick possible (weight 0, or no lag fits the record), 2 = live
    auto classify = [&](long long chl, long long& n0) {
        n0 = 0;
        if (chl >= nch) return 0;
        const float w = weights ? weights[chl] : 1.f;
        if (w == 0.f) return 1;
        n0 = s0 + (long long)r[(size_t)c * (size_t)nch + (size_t)chl];
        return max(-(long long)M, -n0) <= min((long long)M, ntot - L - n0) ? 2 : 1;
    };

    // the 16 lanes of a channel stage its window: the four channels' loads are in flight together
    long long n0;                                            // of this lane's channel
    const int state = classify(ch0 + kk, n0);
    const size_t e = (size_t)c * (size_t)nch + (size_t)(state ? ch0 + kk : 0);
    if (state == 2) {
        const size_t ch = (size_t)(ch0 + kk);
        float* __restrict__ wk = win + (size_t)kk * Ws;
        const long long lo = n0 - M, hi = n0 + M + L - 1;
        if (lo >= 0 && hi < (long long)ns) {
            const float* __restrict__ p = x + ch * (size_t)pitch + lo;
            for (int i = g; i < Wn; i += kAlignGroup) wk[i] = p[i];
        } else if (lo >= (long long)ns && hi < ntot) {
            const float* __restrict__ p = xn + ch * (size_t)pitchn + (lo - (long long)ns);
            for (int i = g; i < Wn; i += kAlignGroup) wk[i] = p[i];
        } else {                                             // across an end of the record or the seam: every sample is tested
            const float* __restrict__ row = x + ch * (size_t)pitch;
            const float* __restrict__ rown = xn ? xn + ch * (size_t)pitchn : nullptr;
            for (int i = g; i < Wn; i += kAlignGroup) {
                const long long q = lo + i;
                float v = 0.f;
                if (q >= 0 && q < ntot) v = q < (long long)ns ? row[q] : rown[q - (long long)ns];
                wk[i] = v;
            }
        }
    }
    const bool any = __any(state == 2);
    __syncthreads();

    if (any) {
        for (int b = 0; b < nl; b += kAlignPass) {
            const int li0 = b + kAlignRun * g;               // this lane's first lag of the pass
            const float4* __restrict__ wp = reinterpret_cast<const float4*>(win + (size_t)kk * Ws + li0);
            float dot[kAlignRun] = {0.f, 0.f, 0.f, 0.f}, en[kAlignRun] = {0.f, 0.f, 0.f, 0.f};
            float4 xa = lds_read4(wp);
            // taps j .. j + ntaps - 1 from the samples li0 + j .. li0 + j + 7: every chain in increasing j
            auto step = [&](int j, int ntaps) {
                const float4 tv = lds_read4(reinterpret_cast<const float4*>(tl + j));
                const float4 xb = lds_read4(wp + j / 4 + 1);
                const float w[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
                const float tt[4] = {tv.x, tv.y, tv.z, tv.w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (u < ntaps) {
#pragma unroll
                        for (int v = 0; v < kAlignRun; ++v) {
                            dot[v] = fmaf(tt[u], w[u + v], dot[v]);
                            en[v] = fmaf(w[u + v], w[u + v], en[v]);
                        }
                    }
                }
                xa = xb;
            };
            for (int j = 0; j < L4; j += 4) step(j, 4);
            if (L4 < L) step(L4, L - L4);
            if (state == 2) {
#pragma unroll
                for (int v = 0; v < kAlignRun; ++v) {
                    const int li = li0 + v;
                    if (li >= nl) continue;
                    const long long q = n0 + (li - M);
                    float val = qnan;
                    if (q >= 0 && q + L <= ntot) val = (tn == 0.f || en[v] == 0.f) ? 0.f : dot[v] / sqrtf(tn * en[v]);
                    rl[li] = val;
                    if (rho) rho[e * (size_t)nl + (size_t)li] = val;
                }
            }
        }
    }
    if (state == 1 && rho)
        for (int li = g; li < nl; li += kAlignGroup) rho[e * (size_t)nl + (size_t)li] = qnan;
    __syncthreads();

    float bv = 0.f;
    int bi = kAlignNone;
    if (state == 2) {
        for (int li = g; li < nl; li += kAlignGroup) {       // increasing lags: of equal values the first stays
            const float v = rl[li];
            if (v == v && (bi == kAlignNone || v > bv)) {
                bv = v;
                bi = li;
            }
        }
    }
#pragma unroll
    for (int s = kAlignGroup / 2; s >= 1; s >>= 1) {         // within the 16 lanes of a channel
        const float ov = __shfl_xor(bv, s);
        const int oi = __shfl_xor(bi, s);
        if (oi != kAlignNone && (bi == kAlignNone || ov > bv || (ov == bv && oi < bi))) {
            bv = ov;
            bi = oi;
        }
    }
    if (g != 0 || state == 0) return;
    if (bi == kAlignNone) {                                  // weight 0, no valid lag, or every rho NaN
        Ti[e] = (double)qnan;
        coef[e] = qnan;
        if (lag) lag[e] = 0;
        return;
    }
    double delta = 0.0;
    if (subsample && bi > 0 && bi < nl - 1) {
        const float a = rl[bi - 1], cc = rl[bi + 1];
        if (a == a && cc == cc) {
            const double den = ((double)a - 2.0 * (double)bv) + (double)cc;
            if (den < 0.0) {
                delta = 0.5 * ((double)a - (double)cc) / den;
                if (delta < -0.5) delta = -0.5;
                if (delta > 0.5) delta = 0.5;
            }
        }
    }
    const int m = bi - M;
    coef[e] = bv;
    if (lag) lag[e] = m;
    Ti[e] = (double)bv < min_coef ? (double)qnan : ((double)(n0 + m) + delta) / fs;
}

}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_align_limits(int* max_calls, int* max_length, int* max_lag, int* channels) {
    if (!max_calls || !max_length || !max_lag || !channels) return fail(D4W_EINVAL, "bad argument");
    *max_calls = kAlignMaxCalls;
    *max_length = kAlignMaxLength;
    *max_lag = kAlignMaxLag;
    *channels = kAlignChannels;
    return D4W_OK;
}

int d4w_align_f32(const float* x, int64_t pitch, int nch, int ns, const float* xnext, int64_t pitch_next, int ns_next, const float* tmpl,
                  int length, const int32_t* r, const int64_t* start, int ncalls, int max_lag, const float* weights, double fs, double min_coef,
                  int subsample, double* Ti, float* coef, int32_t* lag, float* rho, void* stream) {
    if (!x || !tmpl || !r || !start || !Ti || !coef) return fail(D4W_EINVAL, "bad argument");
    if (ncalls < 1 || ncalls > kAlignMaxCalls) return fail(D4W_EINVAL, "align: %d calls, a launch takes 1 .. %d", ncalls, kAlignMaxCalls);
    if (length < 1 || length > kAlignMaxLength) return fail(D4W_EINVAL, "align: the template length %d is outside 1 .. %d", length, kAlignMaxLength);
    if (max_lag < 0 || max_lag > kAlignMaxLag) return fail(D4W_EINVAL, "align: max_lag %d is outside 0 .. %d", max_lag, kAlignMaxLag);
    if (!positive_finite(fs)) return fail(D4W_EINVAL, "align: fs must be positive and finite");
    if (!std::isfinite(min_coef)) return fail(D4W_EINVAL, "align: min_coef must be finite");
    const int rc = check_record("align", nch, ns, pitch, xnext, ns_next, pitch_next);
    if (rc) return rc;
    if (nch > (1 << 30)) return fail(D4W_EINVAL, "align: %d channels, a launch takes 1 .. %d", nch, 1 << 30);
    const size_t lds = align_lds_bytes(length, max_lag);
    // above 64 KiB a kernel has to opt into its dynamic LDS size; a refused opt-in is this call's error, before any launch
    if (lds > 64 * 1024) D4W_HIP(hipFuncSetAttribute((const void*)align_pick, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    D4W_LAUNCH(align_pick, dim3(ceil_div(nch, kAlignChannels), ncalls), dim3(kAlignThreads), lds, stream, x, (long long)pitch, nch, ns, xnext,
               (long long)pitch_next, xnext ? ns_next : 0, tmpl, length, (const int*)r, (const long long*)start, max_lag,
               align_row_words(length, max_lag), weights, fs, min_coef, subsample != 0, Ti, coef, (int*)lag, rho);
    return D4W_OK;
}

}  // extern "C"
