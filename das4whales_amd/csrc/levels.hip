// Received level of located calls per channel on MI355X (gfx950): the energy of the strain in a window that follows the
// call's travel time, the energy in a noise window just before the call arrives, and the largest sample of the signal
// window.  The step after the position in dw.loc: SNR against range, the detection range of the cable, a
// transmission-loss fit; beyond the reference, whose only level measure (dsp.snr_tr_array) is a whole-block ratio that knows
// nothing of a call's moveout.  beam.hip sums the channels into one waveform per call; this keeps them apart.
//
//   n0 = start[c] + r[c][ch]                        int64; start clamped to +-2^62 as in beam.hip / align.hip, r = moveout_round(tau)
//   signal window  S = [n0, n0 + L)                 L >= 1
//   noise window   Q = [n0 - gap - N, n0 - gap)     N >= 0, gap >= 0; N = 0: no noise window
//   the record is ns + ns_next samples (sample ns + i of a row is xnext[ch][i]); a window is valid iff it lies wholly inside it
//     es = sum_{j<L} x[ch][n0 + j]^2               signal[c][ch] = es / (float)L     one correctly rounded division
//     eq = sum_{j<N} x[ch][n0 - gap - N + j]^2     noise[c][ch]  = eq / (float)N
//     peak[c][ch] = max_{j<L} |x[ch][n0 + j]|      exact
//   An invalid window gives NaN (noise is all NaN with N = 0); a NaN sample makes its window's mean square NaN, and peak is
//   NaN wherever signal is.  A channel with weights[ch] = 0 is never read and its three outputs are NaN; a non-zero weight
//   scales nothing, it is a mask.
//
// Sum order, a function of the window length alone.  64 interleaved chains: chain i takes j = i, i + 64, ... in increasing
// order, one fmaf(v, v, acc) per term from 0; the chains are added pairwise at distances 32, 16, 8, 4, 2, 1 (the order
// align.hip uses for tn).  Nothing in it depends on n0, on the address of the window, on the pitch, on where the seam falls
// or on the rest of the batch, and every product with a power of two is exact: run-to-run bit-identical, signal and noise
// scale by 4^k and peak by 2^k under a scaling of x by 2^k.
//
// level_sum: grid (ceil(nch / 4), ncalls), one wave of 64 threads for four channels of one call, 16 lanes per channel, so
//   that a window of a few tens of samples still occupies its lanes.  Lane g of a channel owns the chains g, g + 16, g + 32,
//   g + 48 in four registers: per trip it reads the samples j + g + 16 s, s < 4 -- the 16 lanes of a channel read 64-byte
//   runs of the row, four runs and the four channels in flight together -- and the chain sum starts inside the lane
//   (distance 32: registers 0 + 2 and 1 + 3; distance 16: 0 + 1) and ends in four shuffles within the 16 lanes.  A window is
//   described once, as beam_sum and align_pick classify theirs: sample i of it is pa[i] for i < split and pb[i - split] after,
//   with split = the window's length when it lies wholly in the block or wholly in the next one (a plain loop through one
//   row pointer) and less only across the seam, where every sample is tested.  An invalid window is not read at all.  When
//   both windows of a channel are plain, one loop issues the loads of both (they are gap samples apart); otherwise each
//   runs by itself.  No LDS, no atomics, no workspace.
//   Compiler's report (gfx950, -Rpass-analysis=kernel-resource-usage): 39 VGPRs, 44 SGPRs, no scratch, no LDS, 8 waves per
//   SIMD by registers.
//
// Cost model: ncalls nch (L + N) words read, one fmaf each: the reads are everything.  Inside a call nothing is read twice,
//   and across calls the L2 (4 MiB per XCD against 35 MB per call at 11 020 channels x 800 samples) holds next to nothing, so
//   the expectation is the rate at which pieces of rows stream from HBM.  Measured for 64 calls at 11 020 channels,
//   L = N = 400 (2.26 GB): 0.339 ms, 6.7 TB/s, against 0.368 + 0.037 ms for the order-0 beam over the same samples; with 1, 2,
//   8 or 16 channels per wave instead of 4 (the same sum order) the call took 0.545, 0.401, 0.457, 0.580 ms against 0.382
//   (profiles/levels/).
#include "taps.h"

#ifndef D4W_EMU
#pragma clang fp contract(off)
#endif

namespace d4w {

constexpr int kLevelThreads = 64;                            // one wave
constexpr int kLevelChannels = 4;                            // channels per workgroup: a power of two up to 64 (1 ... 16 were timed)
constexpr int kLevelGroup = kLevelThreads / kLevelChannels;  // lanes per channel
constexpr int kLevelSlots = 64 / kLevelGroup;                // chains per lane
constexpr int kLevelMaxCalls = 65535;                        // grid limit
constexpr int kLevelMaxLength = 1 << 30;                     // of L and of N + gap

// LevelWindow, level_window: taps.h (project.hip describes its windows the same way)

// one trip of a lane: the terms i = j + 16 s, s < 4, of its four chains (j = the lane's place among the 16 of its channel + 64 k)
template <bool SEAM>
__device__ __forceinline__ void level_trip(const LevelWindow& w, int j, float (&acc)[kLevelSlots], float& pk) {
    float v[kLevelSlots];
#pragma unroll
    for (int s = 0; s < kLevelSlots; ++s) {
        const int i = j + kLevelGroup * s;
        v[s] = 0.f;
        if (i < w.len) v[s] = (!SEAM || i < w.split) ? w.pa[i] : w.pb[i - w.split];
    }
#pragma unroll
    for (int s = 0; s < kLevelSlots; ++s) {
        if (j + kLevelGroup * s < w.len) {
            acc[s] = fmaf(v[s], v[s], acc[s]);
            pk = fmaxf(pk, fabsf(v[s]));
        }
    }
}

// grid (ceil(nch / 4), ncalls).  r, signal, noise, peak [ncalls][nch]; noise or NULL
__global__ __launch_bounds__(kLevelThreads) void level_sum(const float* __restrict__ x, long long pitch, int nch, int ns,
                                                           const float* __restrict__ xn, long long pitchn, int nsn,
                                                           const int* __restrict__ r, const long long* __restrict__ start, int L, int gap, int N,
                                                           const float* __restrict__ weights, float* __restrict__ signal,
                                                           float* __restrict__ noise, float* __restrict__ peak) {
    const int lane = threadIdx.x, kk = lane / kLevelGroup, g = lane % kLevelGroup;
    const int c = blockIdx.y;
    const long long chl = (long long)blockIdx.x * kLevelChannels + kk;
    const long long ntot = (long long)ns + (long long)nsn;
    const long long s0 = clamp_start(start[c]);
    const float qnan = __int_as_float(0x7fc00000);

    const bool there = chl < nch;
    const bool live = there && (weights ? weights[chl] != 0.f : true);
    LevelWindow ws{nullptr, nullptr, 0, 0}, wq{nullptr, nullptr, 0, 0};
    if (live) {
        const size_t ch = (size_t)chl;
        const long long n0 = s0 + (long long)r[(size_t)c * (size_t)nch + ch];
        const float* row = x + ch * (size_t)pitch;
        const float* rown = xn ? xn + ch * (size_t)pitchn : nullptr;
        ws = level_window(row, rown, n0, L, (long long)ns, ntot);
        wq = level_window(row, rown, n0 - gap - N, N, (long long)ns, ntot);
    }

    float es[kLevelSlots], eq[kLevelSlots];
#pragma unroll
    for (int s = 0; s < kLevelSlots; ++s) es[s] = eq[s] = 0.f;
    float pk = 0.f, pq = 0.f;
    if (ws.len && wq.len && ws.split == ws.len && wq.split == wq.len) {      // both plain: the loads of both in flight together
        const int both = min(ws.len, wq.len);
        int j = g;
        for (; j < both; j += 64) {
            level_trip<false>(ws, j, es, pk);
            level_trip<false>(wq, j, eq, pq);
        }
        for (int i = j; i < ws.len; i += 64) level_trip<false>(ws, i, es, pk);
        for (int i = j; i < wq.len; i += 64) level_trip<false>(wq, i, eq, pq);
    } else {
        if (ws.split == ws.len) {
            for (int j = g; j < ws.len; j += 64) level_trip<false>(ws, j, es, pk);
        } else {
            for (int j = g; j < ws.len; j += 64) level_trip<true>(ws, j, es, pk);
        }
        if (wq.split == wq.len) {
            for (int j = g; j < wq.len; j += 64) level_trip<false>(wq, j, eq, pq);
        } else {
            for (int j = g; j < wq.len; j += 64) level_trip<true>(wq, j, eq, pq);
        }
    }

    // chains i and i + 32, then i and i + 16, inside the lane; 8, 4, 2, 1 across the 16 lanes of the channel
#pragma unroll
    for (int d = kLevelSlots / 2; d >= 1; d >>= 1) {
#pragma unroll
        for (int s = 0; s < d; ++s) {
            es[s] += es[s + d];
            eq[s] += eq[s + d];
        }
    }
    float a = es[0], b = eq[0];
#pragma unroll
    for (int s = kLevelGroup / 2; s >= 1; s >>= 1) {
        a += __shfl_xor(a, s);
        b += __shfl_xor(b, s);
        pk = fmaxf(pk, __shfl_xor(pk, s));
    }
    if (g != 0 || !there) return;
    const size_t e = (size_t)c * (size_t)nch + (size_t)chl;
    const float sig = ws.len ? a / (float)L : qnan;
    signal[e] = sig;
    peak[e] = sig != sig ? qnan : pk;
    if (noise) noise[e] = wq.len ? b / (float)N : qnan;
}

}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_level_limits(int* max_calls, int* max_length, int* channels) {
    if (!max_calls || !max_length || !channels) return fail(D4W_EINVAL, "bad argument");
    *max_calls = kLevelMaxCalls;
    *max_length = kLevelMaxLength;
    *channels = kLevelChannels;
    return D4W_OK;
}

int d4w_level_f32(const float* x, int64_t pitch, int nch, int ns, const float* xnext, int64_t pitch_next, int ns_next, const int32_t* r,
                  const int64_t* start, int ncalls, int length, int gap, int noise_length, const float* weights, float* signal, float* noise,
                  float* peak, void* stream) {
    if (ncalls < 0 || ncalls > kLevelMaxCalls) return fail(D4W_EINVAL, "level: %d calls, a launch takes 0 .. %d", ncalls, kLevelMaxCalls);
    if (length < 1 || length > kLevelMaxLength) return fail(D4W_EINVAL, "level: the length %d is outside 1 .. %d", length, kLevelMaxLength);
    if (noise_length < 0 || gap < 0 || (long long)noise_length + (long long)gap > (long long)kLevelMaxLength)
        return fail(D4W_EINVAL, "level: noise_length %d and gap %d must be >= 0 and add up to at most %d", noise_length, gap, kLevelMaxLength);
    const int rc = check_record("level", nch, ns, pitch, xnext, ns_next, pitch_next);
    if (rc) return rc;
    if (nch > (1 << 30)) return fail(D4W_EINVAL, "level: %d channels, a launch takes 1 .. %d", nch, 1 << 30);
    if (ncalls == 0) return D4W_OK;
    if (!x || !r || !start || !signal || !peak) return fail(D4W_EINVAL, "bad argument");
    if (noise_length > 0 && !noise) return fail(D4W_EINVAL, "level: a noise window of %d samples without a noise output", noise_length);
    D4W_LAUNCH(level_sum, dim3(ceil_div(nch, kLevelChannels), ncalls), dim3(kLevelThreads), 0, stream, x, (long long)pitch, nch, ns, xnext,
               (long long)pitch_next, xnext ? ns_next : 0, (const int*)r, (const long long*)start, length, gap, noise_length, weights, signal,
               noise, peak);
    return D4W_OK;
}

}  // extern "C"
