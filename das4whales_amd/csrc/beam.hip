// Delay-and-sum beam of the strain toward located calls on MI355X (gfx950): the waveform of a call with the array's gain, the
// channels advanced by their travel times from the source and summed.  The last step of dw.loc; beyond the
// reference, which has nothing of the kind.  stack.hip sums envelopes along integer delays over a grid of nodes; this sums the
// strain itself along fractional delays toward a few arbitrary positions and keeps the trace.
//
//   tau[c][ch] = |cable[ch] - pos[c]| (1 / c0) fs                          float64, moveout.h's moveout_samples
//   r = floor(tau + 0.5)   or   k = floor(tau), f = float32(tau - k) in [0, 1)        moveout_round, moveout_split
//   beam[c][j] = sum over ch, increasing, of w[ch] v(ch, start[c] + j + delay[c][ch]),           0 <= j < nt
//     order 0: v = x[n + r]                       one fmaf(w, x, acc) per term: a stack_grid term
//     order 1: q = n + k, v = (1 - f) x[q] + f x[q + 1]
//     order 3: four-point Lagrange on x[q - 1 .. q + 2]
//   over the channels with w[ch] != 0 whose taps all lie inside the record [0, ns + ns_next): sample ns + i of a row is
//   xnext[ch][i] (the next file of the same cable).
//
// Arithmetic.  The interpolation coefficients are formed in float32 from f and multiplied by the weight once per (call,
// channel); a term of order 1 or 3 is t = c0 x0, t = fmaf(c_m, x_m, t) over its further taps, acc += t, so that the chain of
// the channel sum has one rounding per channel whatever the order.  One thread owns an element for a run of channels; the sum
// is float32, in increasing channel order, no atomics.  The channels are split in fixed segments of kBeamSegment = 128 (a
// single call at a file's length is a dozen column tiles only: 12 x 87 workgroups at 11 020 channels): each segment is summed
// from 0, and beam_reduce adds the segment partials in increasing segment order, the weight sums of normalize beside them.
// The segment is a constant of the source, so an element has one defined sequence of roundings: run-to-run bit-identical,
// independent of the other calls of the batch, exact under a power-of-two scaling of x, and with nch <= 128, order 0 and no
// normalize the same bits as stack_grid's column at that node: r and stack.hip's table are the same two functions of moveout.h.
//
// beam_sum<ORDER, NORM>: grid (ceil(nt / 1024), segments, ncalls), 256 threads; a thread owns columns col0 + tid + 256 j,
//   j < 4, lanes along consecutive samples: the reads are coalesced, unaligned.  The delay, the fraction and the weight of a
//   (call, channel) are wave-uniform (scalar loads), the coefficients a handful of vector instructions per channel.  Per
//   channel the tile's span of samples is classified once: wholly inside x or wholly inside xnext takes the plain loop on
//   that row's pointer (no range test, no selection between the blocks); wholly outside the record adds nothing; a span that
//   crosses an end of the record or the seam between the blocks takes the loop that tests every term.
//   Direct reads from global memory: an order-3 term reads four words that its neighbouring lanes read as well, from L1/L2.
//   Compiler's report (gfx950): order 0 / 1 / 3 use 20 / 24 / 31 VGPRs (normalize: 27 / 31 / 40), 8 waves per SIMD, no LDS, no
//   scratch.
// beam_reduce<NORM>: one thread per element, partials [segment][call][nt] read coalesced.
// beam_delays: one thread per (call, channel).
//
// Cost model: ncalls nch nt words read from the block, order + 1 words from cache and as many multiply-adds per term, and
//   2 ncalls nt ceil(nch / 128) words of partials written and read back (under 2 % of the reads).  Measured with segments
//   of 256 / 128 / 64 channels at 11 020 x 12 000: one call of order 0 takes 0.60 / 0.38 / 0.30 ms (two, four or eight
//   workgroups per compute unit), 64 calls 4.90 / 4.94 / 5.35 ms, and the workspace of 64 calls is 0.27 / 0.54 / 1.06 GB.
#include "taps.h"

#ifndef D4W_EMU
#pragma clang fp contract(off)
#endif

namespace d4w {

constexpr int kBeamThreads = 256;
constexpr int kBeamCpt = 4;                                   // columns per thread
constexpr int kBeamTile = kBeamThreads * kBeamCpt;            // columns per workgroup
// kBeamSegment, the channels one thread sums from 0: taps.h (coherence.hip sums in the same segments)
constexpr int kBeamMaxCalls = 65535;                          // grid limit
constexpr int kBeamMaxLength = kMoveoutDelayMax;              // a beam is no longer than the longest delay

// grid (ceil(nch / 256), min(ncalls, 65535)); pos [ncalls][3]; k, f, r [ncalls][nch], each or NULL
__global__ __launch_bounds__(kBeamThreads) void beam_delays(const double* __restrict__ cable, int nch, double inv_c0, double fs,
                                                            const double* __restrict__ pos, int ncalls, int* __restrict__ k,
                                                            float* __restrict__ f, int* __restrict__ r) {
    const int ch = blockIdx.x * kBeamThreads + threadIdx.x;
    if (ch >= nch) return;
    const double cx = cable[3 * (size_t)ch], cy = cable[3 * (size_t)ch + 1], cz = cable[3 * (size_t)ch + 2];
    for (int c = blockIdx.y; c < ncalls; c += gridDim.y) {
        const double tau = moveout_samples(cx, cy, cz, pos[3 * (size_t)c], pos[3 * (size_t)c + 1], pos[3 * (size_t)c + 2], inv_c0, fs);
        const size_t e = (size_t)c * (size_t)nch + ch;
        if (r) r[e] = moveout_round(tau);
        if (k) {
            int kk;
            float ff;
            moveout_split(tau, kk, ff);
            k[e] = kk;
            f[e] = ff;
        }
    }
}

// grid (ceil(nt / 1024), segments, ncalls).  nseg == 1: out = beam [ncalls][nt], finished; else out = partial sums and wout =
// partial weight sums, both [nseg][ncalls][nt]
template <int ORDER, bool NORM>
__global__ __launch_bounds__(kBeamThreads) void beam_sum(const float* __restrict__ x, long long pitch, int nch, int ns,
                                                         const float* __restrict__ xn, long long pitchn, int nsn,
                                                         const int* __restrict__ kr, const float* __restrict__ fr,
                                                         const float* __restrict__ weights, const long long* __restrict__ start,
                                                         int ncalls, int nt, int nseg, float* __restrict__ out, float* __restrict__ wout) {
    constexpr int kTaps = ORDER + 1, kLo = ORDER == 3 ? -1 : 0, kHi = ORDER == 3 ? 2 : ORDER;
    const int tid = threadIdx.x, seg = blockIdx.y, c = blockIdx.z;
    const long long col0 = (long long)blockIdx.x * kBeamTile;
    const long long b0 = clamp_start(start[c]) + col0;        // the sample of column col0 at delay 0
    const long long ntot = (long long)ns + (long long)nsn;
    const int ch0 = seg * kBeamSegment, ch1 = min(nch, ch0 + kBeamSegment);

    float acc[kBeamCpt], wsum[NORM ? kBeamCpt : 1];
#pragma unroll
    for (int j = 0; j < kBeamCpt; ++j) {
        acc[j] = 0.f;
        if constexpr (NORM) wsum[j] = 0.f;
    }

    for (int ch = ch0; ch < ch1; ++ch) {
        const float w = weights ? weights[ch] : 1.f;         // wave-uniform, like the delay and the fraction
        if (w == 0.f) continue;                              // a channel of weight 0 is not read at all
        const size_t e = (size_t)c * (size_t)nch + ch;
        const long long q0 = b0 + kr[e];
        const long long lo = q0 + kLo, hi = q0 + (kBeamTile - 1) + kHi;
        if (hi < 0 || lo >= ntot) continue;                  // the whole span lies outside the record

        float l[kTaps];                                      // weight x interpolation coefficient (taps.h)
        delay_taps<ORDER>(w, ORDER == 0 ? 0.f : fr[e], l);

        // the terms of this channel on a row pointer p = &row[q0]: every tap lies inside that block
        auto plain = [&](const float* __restrict__ p) {
#pragma unroll
            for (int j = 0; j < kBeamCpt; ++j) {
                const float* __restrict__ pj = p + tid + j * kBeamThreads;
                if constexpr (ORDER == 0) {
                    acc[j] = fmaf(l[0], pj[0], acc[j]);
                } else {
                    float t = l[0] * pj[kLo];
#pragma unroll
                    for (int m = 1; m < kTaps; ++m) t = fmaf(l[m], pj[kLo + m], t);
                    acc[j] += t;
                }
                if constexpr (NORM) wsum[j] += w;
            }
        };

        if (lo >= 0 && hi < (long long)ns) {
            plain(x + (size_t)ch * (size_t)pitch + q0);
        } else if (lo >= (long long)ns && hi < ntot) {
            plain(xn + (size_t)ch * (size_t)pitchn + (q0 - (long long)ns));
        } else {                                             // across an end of the record or the seam: every term is tested
            const float* __restrict__ row = x + (size_t)ch * (size_t)pitch;
            const float* __restrict__ rown = xn ? xn + (size_t)ch * (size_t)pitchn : nullptr;
            auto at = [&](long long i) { return i < (long long)ns ? row[i] : rown[i - (long long)ns]; };
#pragma unroll
            for (int j = 0; j < kBeamCpt; ++j) {
                const long long q = q0 + tid + j * kBeamThreads;
                if (q + kLo < 0 || q + kHi >= ntot) continue;
                if constexpr (ORDER == 0) {
                    acc[j] = fmaf(l[0], at(q), acc[j]);
                } else {
                    float t = l[0] * at(q + kLo);
#pragma unroll
                    for (int m = 1; m < kTaps; ++m) t = fmaf(l[m], at(q + kLo + m), t);
                    acc[j] += t;
                }
                if constexpr (NORM) wsum[j] += w;
            }
        }
    }

#pragma unroll
    for (int j = 0; j < kBeamCpt; ++j) {
        const long long col = col0 + tid + j * kBeamThreads;
        if (col >= nt) continue;
        if (nseg == 1) {
            float v = acc[j];
            if constexpr (NORM) v = wsum[j] != 0.f ? v / wsum[j] : 0.f;
            out[(size_t)c * (size_t)nt + (size_t)col] = v;
        } else {
            const size_t o = ((size_t)seg * (size_t)ncalls + c) * (size_t)nt + (size_t)col;
            out[o] = acc[j];
            if constexpr (NORM) wout[o] = wsum[j];
        }
    }
}

// grid (ceil(nt / 256), min(ncalls, 65535)).  part, wpart [nseg][ncalls][nt]
template <bool NORM>
__global__ __launch_bounds__(kBeamThreads) void beam_reduce(const float* __restrict__ part, const float* __restrict__ wpart, int nseg,
                                                            int ncalls, int nt, float* __restrict__ beam) {
    const long long col = (long long)blockIdx.x * kBeamThreads + threadIdx.x;
    if (col >= nt) return;
    for (int c = blockIdx.y; c < ncalls; c += gridDim.y) {
        const size_t o = (size_t)c * (size_t)nt + (size_t)col, step = (size_t)ncalls * (size_t)nt;
        float v = part[o], ws = NORM ? wpart[o] : 0.f;
        for (int s = 1; s < nseg; ++s) {                     // increasing segment order
            v += part[o + (size_t)s * step];
            if constexpr (NORM) ws += wpart[o + (size_t)s * step];
        }
        if constexpr (NORM) v = ws != 0.f ? v / ws : 0.f;
        beam[o] = v;
    }
}

static int beam_check_shape(const char* who, int nch, int ncalls, int length) {
    if (nch < 1 || nch > 65535 * kBeamSegment) return fail(D4W_EINVAL, "%s: %d channels, a launch takes 1 .. %d", who, nch, 65535 * kBeamSegment);
    if (ncalls < 1 || ncalls > kBeamMaxCalls) return fail(D4W_EINVAL, "%s: %d calls, a launch takes 1 .. %d", who, ncalls, kBeamMaxCalls);
    if (length < 1 || length > kBeamMaxLength) return fail(D4W_EINVAL, "%s: the length %d is outside 1 .. %d", who, length, kBeamMaxLength);
    return D4W_OK;
}

static size_t beam_part_words(int nch, int ncalls, int length) {
    const int nseg = ceil_div(nch, kBeamSegment);
    return nseg > 1 ? (size_t)nseg * (size_t)ncalls * (size_t)length : 0;
}

template <int ORDER>
static int beam_launch(const float* x, long long pitch, int nch, int ns, const float* xn, long long pitchn, int nsn, const int32_t* kr,
                       const float* fr, const float* weights, const int64_t* start, int ncalls, int nt, int normalize, float* beam, float* part,
                       float* wpart, void* stream) {
    const int nseg = ceil_div(nch, kBeamSegment);
    const dim3 grid(ceil_div(nt, kBeamTile), nseg, ncalls);
    float* out = nseg == 1 ? beam : part;
    if (normalize)
        D4W_LAUNCH((beam_sum<ORDER, true>), grid, dim3(kBeamThreads), 0, stream, x, pitch, nch, ns, xn, pitchn, nsn, (const int*)kr, fr, weights,
                   (const long long*)start, ncalls, nt, nseg, out, wpart);
    else
        D4W_LAUNCH((beam_sum<ORDER, false>), grid, dim3(kBeamThreads), 0, stream, x, pitch, nch, ns, xn, pitchn, nsn, (const int*)kr, fr, weights,
                   (const long long*)start, ncalls, nt, nseg, out, wpart);
    if (nseg > 1) {
        const dim3 rgrid(ceil_div(nt, kBeamThreads), min(ncalls, 65535));
        if (normalize)
            D4W_LAUNCH((beam_reduce<true>), rgrid, dim3(kBeamThreads), 0, stream, (const float*)part, (const float*)wpart, nseg, ncalls, nt, beam);
        else
            D4W_LAUNCH((beam_reduce<false>), rgrid, dim3(kBeamThreads), 0, stream, (const float*)part, (const float*)wpart, nseg, ncalls, nt, beam);
    }
    return D4W_OK;
}

}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_beam_limits(int* max_calls, int* max_length, int* segment) {
    if (!max_calls || !max_length || !segment) return fail(D4W_EINVAL, "bad argument");
    *max_calls = kBeamMaxCalls;
    *max_length = kBeamMaxLength;
    *segment = kBeamSegment;
    return D4W_OK;
}

int d4w_beam_tile(int* samples) {
    if (!samples) return fail(D4W_EINVAL, "bad argument");
    *samples = kBeamTile;
    return D4W_OK;
}

int d4w_beam_delays(const double* cable_pos, int nch, double c0, double fs, const double* pos, int ncalls, int32_t* k, float* f, int32_t* r,
                    void* stream) {
    if (!cable_pos || !pos) return fail(D4W_EINVAL, "bad argument");
    if ((k == nullptr) != (f == nullptr)) return fail(D4W_EINVAL, "beam_delays: k and f come together");
    if (!k && !r) return fail(D4W_EINVAL, "beam_delays: neither (k, f) nor r is asked for");
    if (nch < 1) return fail(D4W_EINVAL, "beam_delays: %d channels", nch);
    if (ncalls < 1 || ncalls > kBeamMaxCalls) return fail(D4W_EINVAL, "beam_delays: %d calls, a launch takes 1 .. %d", ncalls, kBeamMaxCalls);
    if (!positive_finite(fs) || !positive_finite(c0)) return fail(D4W_EINVAL, "beam_delays: fs and c0 must be positive and finite");
    D4W_LAUNCH(beam_delays, dim3(ceil_div(nch, kBeamThreads), min(ncalls, 65535)), dim3(kBeamThreads), 0, stream, cable_pos, nch, 1.0 / c0, fs, pos,
               ncalls, (int*)k, f, (int*)r);
    return D4W_OK;
}

int d4w_beam_ws_bytes(int nch, int ncalls, int length, size_t* bytes) {
    if (!bytes) return fail(D4W_EINVAL, "bad argument");
    const int rc = beam_check_shape("beam_ws_bytes", nch, ncalls, length);
    if (rc) return rc;
    *bytes = 2 * beam_part_words(nch, ncalls, length) * sizeof(float);
    return D4W_OK;
}

int d4w_beamform_f32(const float* x, int64_t pitch, int nch, int ns, const float* xnext, int64_t pitch_next, int ns_next, const int32_t* k_or_r,
                     const float* f, const float* weights, const int64_t* start, int ncalls, int length, int order, int normalize, float* beam,
                     void* ws, void* stream) {
    if (!x || !k_or_r || !start || !beam) return fail(D4W_EINVAL, "bad argument");
    if (order != 0 && order != 1 && order != 3) return fail(D4W_EINVAL, "beamform: order %d is none of 0, 1, 3", order);
    if (order != 0 && !f) return fail(D4W_EINVAL, "beamform: order %d needs the fractions f", order);
    int rc = beam_check_shape("beamform", nch, ncalls, length);
    if (rc) return rc;
    rc = check_record("beamform", nch, ns, pitch, xnext, ns_next, pitch_next);
    if (rc) return rc;
    const size_t words = beam_part_words(nch, ncalls, length);
    if (words && !ws) return fail(D4W_EINVAL, "beamform: %d channels are more than one segment of %d and need the workspace", nch, kBeamSegment);
    float* part = (float*)ws;
    float* wpart = part ? part + words : nullptr;
    const int nsn = xnext ? ns_next : 0;
    if (order == 0) return beam_launch<0>(x, pitch, nch, ns, xnext, pitch_next, nsn, k_or_r, f, weights, start, ncalls, length, normalize, beam, part, wpart, stream);
    if (order == 1) return beam_launch<1>(x, pitch, nch, ns, xnext, pitch_next, nsn, k_or_r, f, weights, start, ncalls, length, normalize, beam, part, wpart, stream);
    return beam_launch<3>(x, pitch, nch, ns, xnext, pitch_next, nsn, k_or_r, f, weights, start, ncalls, length, normalize, beam, part, wpart, stream);
}

}  // extern "C"
