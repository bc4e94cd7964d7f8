// The transpose of the beam on MI355X (gfx950): the waveform of a located call put back on every channel along the call's
// moveout, fitted to what the channel recorded, and subtracted from the block.  The step of dw.loc that writes the block
// (DESIGN.md 3.9g), the CLEAN step of array processing: after it a second pass over the residual sees the call that lay 20 dB
// under the first; beyond the reference, which has nothing of the kind.  beam.hip sums the channels into one waveform per
// call; this takes that waveform b_c [L] and goes the other way.
//
//   q0 = start[c] + k[c][ch] (orders 1, 3) or start[c] + r[c][ch] (order 0)      int64; start clamped to +-2^62 as in beam.hip
//   l_m, kLo <= m <= kHi: the unweighted float32 coefficients of the fraction f[c][ch], taps.h's delay_taps with w = 1
//   image of the beam on the channel, the exact transpose of beam_sum's taps:
//     g[c][ch](n) = sum_m l_m b_c[n - q0 - m],  b_c[j] = 0 outside 0 <= j < L
//     float32: t = l_lo b, then t = fmaf(l_m, b, t) over the further taps in increasing m        (project_image, one text)
//   support n in [q0 + kLo, q0 + L - 1 + kHi], W = L + order samples; the record is ns + ns_next samples (sample ns + i of a
//   row is xnext[ch][i]); the window is valid iff the support lies wholly inside the record.
//
// Fit (project_fit): over the support, num = sum x g, den = sum g g, xx = sum x x, then
//     amp = num / den (one correctly rounded division; 0 where den = 0)          the least-squares amplitude of the image
//     coef = num / sqrtf(den xx) (0 where den or xx is 0)                         align.hip's form
//   An invalid window gives NaN in both and is not read; a NaN sample in the window gives NaN in both (also over a zero
//   beam); a channel of weight 0 is never read and gives NaN; a non-zero weight scales nothing.  Every fit is against the
//   block as given, independent of the other calls.
//   Sum order, levels.hip's, a function of W alone: term i of the support goes to chain i mod 64, one fmaf per term from 0 in
//   increasing i; the chains are added pairwise at distances 32, 16, 8, 4, 2, 1.  Nothing depends on q0, the pitch, the seam
//   or the batch, and a product with a power of two is exact: run-to-run bit-identical, amp scales by 2^k and coef keeps its
//   bits under a scaling of the channel by 2^k.
//   grid (ceil(nch / 4), ncalls), one wave for four channels of one call, 16 lanes per channel, lane g owning the chains
//   g, g + 16, g + 32, g + 48 (level_sum's shape: the 16 lanes of a channel read 64-byte runs of the row, four runs and four
//   channels in flight).  The beam (L words per call, shared by every workgroup of the call) goes through LDS in pieces of
//   1024 terms of the support (a multiple of 64: the chains keep their order), each with its `order` samples of history and
//   zeros outside [0, L), so that a tap is one LDS read without a test (4.1 KB per workgroup).  Read from L1 / L2 with a
//   test per tap instead, the fit took 0.340 / 0.371 / 0.420 ms (order 0 / 1 / 3) against 0.263 / 0.278 / 0.281 ms at 64
//   calls x 11 020 channels x L = 400.  No atomics, no workspace.
//
// Subtraction (project_subtract), a gather: a thread owns eight samples of one channel and walks the calls,
//     y = x, then for c = 0, 1, ... where amp[c][ch] is finite and non-zero, the window is valid and n lies in its support:
//     y = fmaf(-amp[c][ch], g[c][ch](n), y)
//   in increasing c: no atomics, run-to-run bit-identical, independent of the launch geometry.  grid (nch x tiles of 2048
//   samples of the record), 256 threads, lanes along consecutive samples.  The calls are tested 256 at a time, one per
//   thread (a usable amplitude, a valid window, a support that meets the tile); the waves publish their ballots through LDS
//   and every thread walks the set bits in increasing call order, so that a call that misses the tile costs nobody a
//   dependent load (walked one after the other by the whole workgroup, 64 calls cost 2.09 ms out of place where this form
//   costs 0.76 ms).  The beam's taps come from L1 / L2, tested.  Out of place every sample of y and ynext is written (a copy
//   where no call reaches).  In place (y = x) a sample is read when the first call reaches it and stored only then: a tile
//   that no support meets is neither read nor written.
//
// Compiler's report (gfx950, -Rpass-analysis=kernel-resource-usage): project_fit order 0 / 1 / 3: 65 / 48 / 48 VGPRs, 4108
//   bytes of LDS, no scratch, 7 / 8 / 8 waves per SIMD; project_subtract: 50 .. 64 VGPRs, 32 bytes of LDS, no scratch, 8
//   waves per SIMD in all six forms.
//
// Cost model.  Fit: ncalls nch W words of x read once from HBM (pieces of rows, as levels.hip streams them), L words of the
//   beam per workgroup from L2 (a quarter of a word per term), order + 1 LDS reads and three fmaf per term: the expectation
//   is level_sum's rate over the same samples.  Subtraction out of place: the block read and written once, a copy, plus the
//   terms under the supports at about the fit's rate; in place: the samples under the supports read and written, twice the
//   fit's bytes.  Measurements and where they stand against the models: DESIGN.md 3.9g, profiles/project/.
#include "taps.h"

#ifndef D4W_EMU
#pragma clang fp contract(off)
#endif

namespace d4w {

constexpr int kProjThreads = 64;                             // the fit: one wave
constexpr int kProjChannels = 4;                             // channels per workgroup of the fit (level_sum's shape)
constexpr int kProjGroup = kProjThreads / kProjChannels;     // lanes per channel
constexpr int kProjSlots = 64 / kProjGroup;                  // chains per lane
constexpr int kProjMaxCalls = 65535;                         // grid limit
constexpr int kProjMaxLength = 1 << 30;                      // of the beam
constexpr int kProjChunk = 1024;                             // terms of a support per LDS piece of the beam: a multiple of 64
constexpr int kSubThreads = 256;
constexpr int kSubCpt = 8;                                   // samples per thread
constexpr int kSubTile = kSubThreads * kSubCpt;              // samples per workgroup

// sample i of the image's support: g = sum_t l[t] b[i - t], t = 0 .. ORDER (tap m = kLo + t); at(j) = b[j], 0 outside [0, L)
template <int ORDER, typename At>
__device__ __forceinline__ float project_image(At at, const float (&l)[ORDER + 1], int i) {
    float t = l[0] * at(i);
#pragma unroll
    for (int m = 1; m <= ORDER; ++m) t = fmaf(l[m], at(i - m), t);
    return t;
}

// the first sample of the support of (call, channel) e; whether the window is valid
template <int ORDER>
__device__ __forceinline__ bool project_support(const long long* __restrict__ start, int c, const int* __restrict__ kr, size_t e, int W,
                                                long long ntot, long long& lo) {
    constexpr int kLo = ORDER == 3 ? -1 : 0;
    lo = clamp_start(start[c]) + (long long)kr[e] + kLo;
    return lo >= 0 && lo + W <= ntot;
}

// one trip of a lane of the fit: the terms i = j + 16 s, s < 4, of its four chains
template <int ORDER, bool SEAM, typename At>
__device__ __forceinline__ void project_trip(const LevelWindow& w, At at, const float (&l)[ORDER + 1], int j, float (&num)[kProjSlots],
                                             float (&den)[kProjSlots], float (&xx)[kProjSlots]) {
    float v[kProjSlots];
#pragma unroll
    for (int s = 0; s < kProjSlots; ++s) {
        const int i = j + kProjGroup * s;
        v[s] = 0.f;
        if (i < w.len) v[s] = (!SEAM || i < w.split) ? w.pa[i] : w.pb[i - w.split];
    }
#pragma unroll
    for (int s = 0; s < kProjSlots; ++s) {
        const int i = j + kProjGroup * s;
        if (i < w.len) {
            const float g = project_image<ORDER>(at, l, i);
            num[s] = fmaf(v[s], g, num[s]);
            den[s] = fmaf(g, g, den[s]);
            xx[s] = fmaf(v[s], v[s], xx[s]);
        }
    }
}

// grid (ceil(nch / 4), ncalls).  kr, fr, amp, coef [ncalls][nch]; beam [ncalls][L]
template <int ORDER>
__global__ __launch_bounds__(kProjThreads) void project_fit(const float* __restrict__ x, long long pitch, int nch, int ns,
                                                            const float* __restrict__ xn, long long pitchn, int nsn,
                                                            const int* __restrict__ kr, const float* __restrict__ fr,
                                                            const float* __restrict__ beam, int L, const long long* __restrict__ start,
                                                            const float* __restrict__ weights, float* __restrict__ amp,
                                                            float* __restrict__ coef) {
    __shared__ float sb[kProjChunk + 3];                     // sb[u] = b[base + u - ORDER], 0 outside [0, L)
    const int lane = threadIdx.x, kk = lane / kProjGroup, g = lane % kProjGroup;
    const int c = blockIdx.y, W = L + ORDER;
    const long long chl = (long long)blockIdx.x * kProjChannels + kk;
    const long long ntot = (long long)ns + (long long)nsn;
    const float qnan = __int_as_float(0x7fc00000);

    const bool there = chl < nch;
    const bool live = there && (weights ? weights[chl] != 0.f : true);
    LevelWindow w{nullptr, nullptr, 0, 0};
    float l[ORDER + 1];
#pragma unroll
    for (int m = 0; m <= ORDER; ++m) l[m] = 0.f;
    if (live) {
        const size_t ch = (size_t)chl, e = (size_t)c * (size_t)nch + ch;
        long long lo;
        if (project_support<ORDER>(start, c, kr, e, W, ntot, lo))
            w = level_window(x + ch * (size_t)pitch, xn ? xn + ch * (size_t)pitchn : nullptr, lo, W, (long long)ns, ntot);
        delay_taps<ORDER>(1.f, ORDER == 0 ? 0.f : fr[e], l);
    }
    const float* __restrict__ b = beam + (size_t)c * (size_t)L;

    float num[kProjSlots], den[kProjSlots], xx[kProjSlots];
#pragma unroll
    for (int s = 0; s < kProjSlots; ++s) num[s] = den[s] = xx[s] = 0.f;
    // the support in pieces of kProjChunk terms (a multiple of 64: the chains keep their order), the beam under a piece in LDS
    // with its ORDER samples of history, so that a tap is one LDS read without a test.  Uniform in the wave: W is.
    if (__any(w.len != 0)) {
        for (int base = 0; base < W; base += kProjChunk) {
            if (base) __syncthreads();
            const int nu = min(kProjChunk, W - base) + ORDER;
            for (int u = lane; u < nu; u += kProjThreads) {
                const int jj = base + u - ORDER;
                sb[u] = (jj >= 0 && jj < L) ? b[jj] : 0.f;
            }
            __syncthreads();
            auto at = [&](int i) { return sb[i - base + ORDER]; };
            const int end = min(w.len, base + kProjChunk);
            if (w.split == w.len) {
                for (int j = base + g; j < end; j += 64) project_trip<ORDER, false>(w, at, l, j, num, den, xx);
            } else {
                for (int j = base + g; j < end; j += 64) project_trip<ORDER, true>(w, at, l, j, num, den, xx);
            }
        }
    }

    // chains i and i + 32, then i and i + 16, inside the lane; 8, 4, 2, 1 across the 16 lanes of the channel
#pragma unroll
    for (int d = kProjSlots / 2; d >= 1; d >>= 1) {
#pragma unroll
        for (int s = 0; s < d; ++s) {
            num[s] += num[s + d];
            den[s] += den[s + d];
            xx[s] += xx[s + d];
        }
    }
    float sn = num[0], sd = den[0], sx = xx[0];
#pragma unroll
    for (int s = kProjGroup / 2; s >= 1; s >>= 1) {
        sn += __shfl_xor(sn, s);
        sd += __shfl_xor(sd, s);
        sx += __shfl_xor(sx, s);
    }
    if (g != 0 || !there) return;
    const size_t e = (size_t)c * (size_t)nch + (size_t)chl;
    float a = qnan, r = qnan;
    if (w.len && sx == sx) {                                 // xx is NaN iff a sample of the window is
        a = sd == 0.f ? 0.f : sn / sd;
        r = (sd == 0.f || sx == 0.f) ? 0.f : sn / sqrtf(sd * sx);
    }
    amp[e] = a;
    coef[e] = r;
}

// grid (nch x ntiles).  src / srcn: the block and the next block as given (INPLACE: the same memory as y / yn)
template <int ORDER, bool INPLACE>
__global__ __launch_bounds__(kSubThreads) void project_subtract(const float* src, long long pitch, int nch, int ns, const float* srcn,
                                                                long long pitchn, int nsn, const int* __restrict__ kr,
                                                                const float* __restrict__ fr, const float* __restrict__ beam, int L,
                                                                const long long* __restrict__ start, const float* __restrict__ amp,
                                                                int ncalls, float* y, long long pitchy, float* yn, long long pitchyn,
                                                                int ntiles) {
    __shared__ unsigned long long takes[kSubThreads / 64];   // per wave: which of its 64 calls take part in the tile
    const int tid = threadIdx.x, W = L + ORDER;
    const size_t ch = blockIdx.x / (unsigned)ntiles;
    const long long n0 = (long long)(blockIdx.x % (unsigned)ntiles) * kSubTile;
    const long long ntot = (long long)ns + (long long)nsn;
    auto load = [&](long long n) { return n < (long long)ns ? src[ch * (size_t)pitch + (size_t)n] : srcn[ch * (size_t)pitchn + (size_t)(n - (long long)ns)]; };

    float v[kSubCpt];
    unsigned hit = 0;                                        // bit j: sample j of the thread lies under a subtracted support
#pragma unroll
    for (int j = 0; j < kSubCpt; ++j) {
        const long long n = n0 + tid + j * kSubThreads;
        v[j] = 0.f;
        if (!INPLACE && n < ntot) v[j] = load(n);            // in place a sample is read when its first call reaches it
    }
    // the calls, kSubThreads at a time: thread t tests call c0 + t (a usable amplitude, a valid window, a support that meets
    // the tile), the waves publish their ballots, and every thread walks the set bits in increasing call order
    for (int c0 = 0; c0 < ncalls; c0 += kSubThreads) {
        bool mine = false;
        if (c0 + tid < ncalls) {
            const size_t e = (size_t)(c0 + tid) * (size_t)nch + ch;
            const float a = amp[e];
            long long lo;
            mine = a == a && a != 0.f && fabsf(a) != __int_as_float(0x7f800000) && project_support<ORDER>(start, c0 + tid, kr, e, W, ntot, lo) &&
                   lo < n0 + kSubTile && lo + W > n0;
        }
        const unsigned long long ballot = __ballot(mine);
        if (c0) __syncthreads();                             // everybody has read the last round's ballots
        if ((tid & 63) == 0) takes[tid >> 6] = ballot;
        __syncthreads();
        for (int wv = 0; wv < kSubThreads / 64; ++wv) {
            unsigned long long m = takes[wv];
            while (m) {
                const int c = c0 + 64 * wv + __popcll((m & (0ull - m)) - 1ull);      // the lowest set bit
                m &= m - 1ull;
                const size_t e = (size_t)c * (size_t)nch + ch;
                const float a = amp[e];
                long long lo;
                project_support<ORDER>(start, c, kr, e, W, ntot, lo);
                float l[ORDER + 1];
                delay_taps<ORDER>(1.f, ORDER == 0 ? 0.f : fr[e], l);
                const float* __restrict__ b = beam + (size_t)c * (size_t)L;
                auto at = [&](int i) { return (i >= 0 && i < L) ? b[i] : 0.f; };
#pragma unroll
                for (int j = 0; j < kSubCpt; ++j) {
                    const long long n = n0 + tid + j * kSubThreads, i = n - lo;
                    if (i >= 0 && i < (long long)W) {
                        if (INPLACE && !(hit >> j & 1u)) v[j] = load(n);
                        v[j] = fmaf(-a, project_image<ORDER>(at, l, (int)i), v[j]);
                        hit |= 1u << j;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kSubCpt; ++j) {
        const long long n = n0 + tid + j * kSubThreads;
        if (n >= ntot || (INPLACE && !(hit >> j & 1u))) continue;
        if (n < (long long)ns) y[ch * (size_t)pitchy + (size_t)n] = v[j];
        else yn[ch * (size_t)pitchyn + (size_t)(n - (long long)ns)] = v[j];
    }
}

// the checks the two entry points share
static int project_check(const char* who, int nch, int ns, long long pitch, const float* xnext, int ns_next, long long pitch_next, int ncalls,
                         int length, int order) {
    if (ncalls < 0 || ncalls > kProjMaxCalls) return fail(D4W_EINVAL, "%s: %d calls, a launch takes 0 .. %d", who, ncalls, kProjMaxCalls);
    if (length < 1 || length > kProjMaxLength) return fail(D4W_EINVAL, "%s: the length %d is outside 1 .. %d", who, length, kProjMaxLength);
    if (order != 0 && order != 1 && order != 3) return fail(D4W_EINVAL, "%s: order %d is none of 0, 1, 3", who, order);
    const int rc = check_record(who, nch, ns, pitch, xnext, ns_next, pitch_next);
    if (rc) return rc;
    if (nch > (1 << 30)) return fail(D4W_EINVAL, "%s: %d channels, a launch takes 1 .. %d", who, nch, 1 << 30);
    return D4W_OK;
}

template <int ORDER>
static int project_subtract_launch(const float* x, long long pitch, int nch, int ns, const float* xn, long long pitchn, int nsn, const int32_t* kr,
                                   const float* fr, const float* beam, int L, const int64_t* start, const float* amp, int ncalls, float* y,
                                   long long pitchy, float* yn, long long pitchyn, int ntiles, void* stream) {
    const dim3 grid((unsigned)((long long)nch * ntiles));
    if (y == x)
        D4W_LAUNCH((project_subtract<ORDER, true>), grid, dim3(kSubThreads), 0, stream, x, pitch, nch, ns, xn, pitchn, nsn, (const int*)kr, fr, beam, L,
                   (const long long*)start, amp, ncalls, y, pitchy, yn, pitchyn, ntiles);
    else
        D4W_LAUNCH((project_subtract<ORDER, false>), grid, dim3(kSubThreads), 0, stream, x, pitch, nch, ns, xn, pitchn, nsn, (const int*)kr, fr, beam, L,
                   (const long long*)start, amp, ncalls, y, pitchy, yn, pitchyn, ntiles);
    return D4W_OK;
}

}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_project_limits(int* max_calls, int* max_length, int* channels) {
    if (!max_calls || !max_length || !channels) return fail(D4W_EINVAL, "bad argument");
    *max_calls = kProjMaxCalls;
    *max_length = kProjMaxLength;
    *channels = kProjChannels;
    return D4W_OK;
}

int d4w_project_f32(const float* x, int64_t pitch, int nch, int ns, const float* xnext, int64_t pitch_next, int ns_next, const int32_t* k_or_r,
                    const float* f, const float* beam, int length, const int64_t* start, int ncalls, int order, const float* weights, float* amp,
                    float* coef, void* stream) {
    const int rc = project_check("project", nch, ns, pitch, xnext, ns_next, pitch_next, ncalls, length, order);
    if (rc) return rc;
    if (ncalls == 0) return D4W_OK;
    if (!x || !k_or_r || !beam || !start || !amp || !coef) return fail(D4W_EINVAL, "bad argument");
    if (order != 0 && !f) return fail(D4W_EINVAL, "project: order %d needs the fractions f", order);
    const dim3 grid(ceil_div(nch, kProjChannels), ncalls);
    const int nsn = xnext ? ns_next : 0;
    if (order == 0)
        D4W_LAUNCH((project_fit<0>), grid, dim3(kProjThreads), 0, stream, x, (long long)pitch, nch, ns, xnext, (long long)pitch_next, nsn,
                   (const int*)k_or_r, f, beam, length, (const long long*)start, weights, amp, coef);
    else if (order == 1)
        D4W_LAUNCH((project_fit<1>), grid, dim3(kProjThreads), 0, stream, x, (long long)pitch, nch, ns, xnext, (long long)pitch_next, nsn,
                   (const int*)k_or_r, f, beam, length, (const long long*)start, weights, amp, coef);
    else
        D4W_LAUNCH((project_fit<3>), grid, dim3(kProjThreads), 0, stream, x, (long long)pitch, nch, ns, xnext, (long long)pitch_next, nsn,
                   (const int*)k_or_r, f, beam, length, (const long long*)start, weights, amp, coef);
    return D4W_OK;
}

int d4w_project_subtract_f32(const float* x, int64_t pitch, int nch, int ns, const float* xnext, int64_t pitch_next, int ns_next,
                             const int32_t* k_or_r, const float* f, const float* beam, int length, const int64_t* start, const float* amp, int ncalls,
                             int order, float* y, int64_t pitch_y, float* ynext, int64_t pitch_ynext, void* stream) {
    int rc = project_check("project_subtract", nch, ns, pitch, xnext, ns_next, pitch_next, ncalls, length, order);
    if (rc) return rc;
    if (!x || !y) return fail(D4W_EINVAL, "bad argument");
    if (pitch_y < ns) return fail(D4W_EINVAL, "project_subtract: the row pitch %lld of y is below the %d samples of a row", (long long)pitch_y, ns);
    if ((xnext == nullptr) != (ynext == nullptr)) return fail(D4W_EINVAL, "project_subtract: xnext and ynext come together");
    if (xnext && pitch_ynext < ns_next)
        return fail(D4W_EINVAL, "project_subtract: the row pitch %lld of ynext is below the %d samples of a row", (long long)pitch_ynext, ns_next);
    const bool inplace = y == x;
    if (inplace ? (pitch_y != pitch || (xnext && (ynext != xnext || pitch_ynext != pitch_next))) : (xnext && ynext == xnext))
        return fail(D4W_EINVAL, "project_subtract: in place means y = x and ynext = xnext with their pitches, out of place neither");
    if (ncalls > 0 && (!k_or_r || !beam || !start || !amp)) return fail(D4W_EINVAL, "bad argument");
    if (ncalls > 0 && order != 0 && !f) return fail(D4W_EINVAL, "project_subtract: order %d needs the fractions f", order);
    const int nsn = xnext ? ns_next : 0;
    const long long ntiles = ((long long)ns + nsn + kSubTile - 1) / kSubTile;
    if ((long long)nch * ntiles > 0x7fffffffll)
        return fail(D4W_EINVAL, "project_subtract: %d channels x %lld tiles of %d samples are more than one launch takes", nch, ntiles, kSubTile);
    if (ncalls == 0 && inplace) return D4W_OK;               // nothing to subtract, nothing to copy
    if (order == 0)
        return project_subtract_launch<0>(x, pitch, nch, ns, xnext, pitch_next, nsn, k_or_r, f, beam, length, start, amp, ncalls, y, pitch_y, ynext,
                                          pitch_ynext, (int)ntiles, stream);
    if (order == 1)
        return project_subtract_launch<1>(x, pitch, nch, ns, xnext, pitch_next, nsn, k_or_r, f, beam, length, start, amp, ncalls, y, pitch_y, ynext,
                                          pitch_ynext, (int)ntiles, stream);
    return project_subtract_launch<3>(x, pitch, nch, ns, xnext, pitch_next, nsn, k_or_r, f, beam, length, start, amp, ncalls, y, pitch_y, ynext,
                                      pitch_ynext, (int)ntiles, stream);
}

}  // extern "C"
