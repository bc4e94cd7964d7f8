// Coherence of located calls along their moveout on MI355X (gfx950): the windowed semblance of the beam (Neidell-Taner) and
// the phase coherence of the analytic signal across the channels, the weight of a phase-weighted stack.  The amplitude-free
// answer to "did anything coherent arrive from the position the solver returned" (DESIGN.md 3.9h); beyond the reference,
// which has nothing of the kind.  semblance.hip gives it for straight moveouts over a few neighbouring channels; this reads
// the gather of beam.hip, the record along the travel times of moveout.h toward a few arbitrary positions.
//
//   For call c, channel ch of weight w = weights[ch] >= 0 and beam sample j, n = start[c] + j:
//   v(ch, j) = the record at n + delay[c][ch], interpolated as beam.hip does for order 0, 1, 3 (taps.h's delay_taps);
//   h(ch, j) = the same interpolation of the imaginary block (the Hilbert transform of the record), where one is given.
//   A term exists iff all of its taps lie inside the record [0, ns + ns_next); a channel of weight 0 is not read.
//   Over the contributing channels, in increasing order:
//     b[c][j] = sum w v        e[c][j] = sum w v^2        W[c][j] = sum w
//     pr = sum w v / a         pi = sum w h / a           a = sqrt(v^2 + h^2); a term with a = 0 adds nothing to pr, pi
//   semblance[c][j] = sum_tau b^2 / sum_tau (W e),  tau over [j - H, j + H] clipped to [0, nt);  0 where the denominator is 0
//   phase[c][j]     = sqrt(pr^2 + pi^2) / W;  0 where W is 0
//   Both lie in [0, 1] (Cauchy-Schwarz per tau with w >= 0), up to the roundings below.
//
// Arithmetic, float32 throughout.  t = w v is beam.hip's term: the coefficients times the weight once per (call, channel),
// t = c0 x0, t = fmaf(c_m, x_m, t), and b takes it exactly as beam_sum does (order 0: one fmaf(w, x, b); else b += t), in the
// same segments of kBeamSegment = 128 channels with contraction off: the b plane is d4w_beamform_f32(normalize = 0) bit for
// bit.  e = fmaf(t (1 / w), t, e) with 1 / w formed once per channel; W += w.  th = w h by the same chain on the imaginary
// block, a2 = fmaf(t, t, th th), and for a2 >= 2^-126 (below it, where the squares underflow, the term counts as a = 0)
// r = w rsqrt(a2), pr = fmaf(t, r, pr), pi = fmaf(th, r, pi): v_rsq_f32, one ulp.  Segment partials are added in increasing
// order; q = b b and d = W e per tau; the window sums add their 2H + 1 terms in increasing tau from 0 (a tau outside
// [0, nt) adds +0, which changes no bit): no running sums, no atomics.  So the results are run-to-run bit-identical and
// independent of the other calls of the batch, and semblance keeps its bits under a power-of-two scaling of the record
// (b, t scale by 2^k, q and d by 4^k, exactly, absent underflow).  Non-finite samples under a non-zero weight leave the
// elements they touch unspecified.
//
// coh_sum<ORDER, PHASE>: beam_sum's grid and walk -- (ceil(nt / 1024), segments, ncalls), 256 threads, a thread owns columns
//   col0 + tid + 256 j, j < 4, lanes along consecutive samples; delay, fraction, weight and 1 / w wave-uniform; per channel the
//   tile's span is classified once as inside x, inside xnext, outside, or crossing (every term tested).  3 accumulators per
//   column, 5 with PHASE; partial planes to the workspace [plane][segment][call][nt], planes b, e, W (, pr, pi).
//   Four columns per thread as in beam_sum: 12 (20) accumulators and the taps in flight stay below the 64 VGPRs that still
//   give 8 waves per SIMD in all forms but one, and with direct coalesced reads there is nothing to stage: no LDS.
//   Compiler's report (gfx950, -Rpass-analysis=kernel-resource-usage), order 0 / 1 / 3: semblance only 35 / 39 / 50 VGPRs, 8
//   waves per SIMD; with phase 56 / 58 / 76 VGPRs, 8 / 8 / 6 waves per SIMD (order 3 holds eight taps of four columns); no
//   LDS, no scratch in any form (beam_sum: 20 - 40 VGPRs).
// coh_finish<PHASE>: grid (ceil(nt / 256), ncalls), 256 threads, one column each.  Adds the segment partials for the tile's
//   256 columns and a halo of H on either side, q and d into an LDS tile of 2 (256 + 2 H) words (6 KiB at the largest H = 256:
//   no limit on residency), writes beam, wsum and phase for its own columns, and after one barrier every thread sums its
//   window from LDS: lanes read consecutive words, conflict-free ds_read_b32.  The halo re-reads the partials 1 + 2 H / 256
//   times; they are under 3 % of coh_sum's reads.  Measured with tiles of 1024 / 256 columns at 11 020 x 12 000, order 0,
//   H = 100: the whole call 0.458 / 0.385 ms for one call (12 / 47 workgroups walk 87 segments each) and 5.14 / 5.10 ms for 64.
//   Re-reading q and d per tau through L2 instead of the LDS tile was not built.  24 VGPRs (30 with phase), no scratch.
// coh_peak: one workgroup of 256 per call; a thread keeps the largest value and its smallest index over columns lo + tid +
//   256 i, then a tree over LDS at distances 128 ... 1, ties to the smaller index: the first maximum, whatever the order.
//
// Cost model: ncalls nch nt words read from the block (twice with the imaginary block), order + 1 words from cache per term
//   and block, and planes ncalls nt ceil(nch / 128) words of partials written, read back (1 + 2 H / 256) times.
//   Measured: DESIGN.md 3.9h, profiles/coherence/.
#include "taps.h"

#ifndef D4W_EMU
#pragma clang fp contract(off)
#endif

namespace d4w {

constexpr int kCohThreads = 256;
constexpr int kCohCpt = 4;                                    // columns per thread
constexpr int kCohTile = kCohThreads * kCohCpt;               // columns per workgroup: beam_sum's tile
constexpr int kCohFinishTile = kCohThreads;                    // columns per workgroup of coh_finish, one per thread
constexpr int kCohSegment = kBeamSegment;                     // taps.h: the b plane is the beam bit for bit
constexpr int kCohMaxCalls = 65535;                           // grid limit
constexpr int kCohMaxLength = kMoveoutDelayMax;
constexpr int kCohMaxHalf = 256;                              // H: 2 H + 1 roundings per window sum (the derived bound stays under 1e-4)
constexpr float kCohTiny = 1.17549435e-38f;                   // 2^-126: below it v^2 + h^2 has underflowed, the term has no phase

__device__ __forceinline__ float coh_rsqrt(float a) {
#ifdef D4W_EMU
    return 1.0f / sqrtf(a);
#else
    return __builtin_amdgcn_rsqf(a);
#endif
}

// grid (ceil(nt / 1024), segments, ncalls).  part [planes][nseg][ncalls][nt], planes = 3 (b, e, W) or 5 (, pr, pi)
template <int ORDER, bool PHASE>
__global__ __launch_bounds__(kCohThreads) void coh_sum(const float* __restrict__ x, long long pitch, int nch, int ns,
                                                       const float* __restrict__ xn, long long pitchn, int nsn,
                                                       const float* __restrict__ y, long long pitchy, const float* __restrict__ yn,
                                                       long long pitchyn, const int* __restrict__ kr, const float* __restrict__ fr,
                                                       const float* __restrict__ weights, const long long* __restrict__ start, int ncalls,
                                                       int nt, int nseg, float* __restrict__ part) {
    constexpr int kTaps = ORDER + 1, kLo = ORDER == 3 ? -1 : 0, kHi = ORDER == 3 ? 2 : ORDER;
    constexpr int kP = PHASE ? kCohCpt : 1;
    const int tid = threadIdx.x, seg = blockIdx.y, c = blockIdx.z;
    const long long col0 = (long long)blockIdx.x * kCohTile;
    const long long b0 = clamp_start(start[c]) + col0;        // the sample of column col0 at delay 0
    const long long ntot = (long long)ns + (long long)nsn;
    const int ch0 = seg * kCohSegment, ch1 = min(nch, ch0 + kCohSegment);

    float b[kCohCpt], e[kCohCpt], wsum[kCohCpt], pr[kP], pi[kP];
#pragma unroll
    for (int j = 0; j < kCohCpt; ++j) {
        b[j] = e[j] = wsum[j] = 0.f;
        if constexpr (PHASE) pr[j] = pi[j] = 0.f;
    }

    for (int ch = ch0; ch < ch1; ++ch) {
        const float w = weights ? weights[ch] : 1.f;         // wave-uniform, like the delay and the fraction
        if (w == 0.f) continue;                              // a channel of weight 0 is not read at all
        const size_t el = (size_t)c * (size_t)nch + ch;
        const long long q0 = b0 + kr[el];
        const long long lo = q0 + kLo, hi = q0 + (kCohTile - 1) + kHi;
        if (hi < 0 || lo >= ntot) continue;                  // the whole span lies outside the record

        float l[kTaps];                                      // weight x interpolation coefficient (taps.h)
        delay_taps<ORDER>(w, ORDER == 0 ? 0.f : fr[el], l);
        const float iw = 1.f / w;

        // one term: re(m), im(m) = the sample of tap kLo + m of this column in the real and the imaginary block
        auto term = [&](int j, auto&& re, auto&& im) {
            float t;
            if constexpr (ORDER == 0) {
                const float v = re(0);
                b[j] = fmaf(l[0], v, b[j]);                  // beam_sum's order-0 term
                t = l[0] * v;
            } else {
                t = l[0] * re(0);
#pragma unroll
                for (int m = 1; m < kTaps; ++m) t = fmaf(l[m], re(m), t);
                b[j] += t;                                   // beam_sum's chain
            }
            e[j] = fmaf(t * iw, t, e[j]);
            wsum[j] += w;
            if constexpr (PHASE) {
                float th = l[0] * im(0);
#pragma unroll
                for (int m = 1; m < kTaps; ++m) th = fmaf(l[m], im(m), th);
                const float a2 = fmaf(t, t, th * th);
                if (a2 >= kCohTiny) {
                    const float r = w * coh_rsqrt(a2);
                    pr[j] = fmaf(t, r, pr[j]);
                    pi[j] = fmaf(th, r, pi[j]);
                }
            }
        };

        // every tap of every column inside one block: p = &row[q0] there, pi_ the same place of the imaginary block
        auto plain = [&](const float* __restrict__ p, const float* __restrict__ pim) {
#pragma unroll
            for (int j = 0; j < kCohCpt; ++j) {
                const float* __restrict__ pj = p + tid + j * kCohThreads;
                const float* __restrict__ qj = PHASE ? pim + tid + j * kCohThreads : nullptr;
                term(j, [&](int m) { return pj[kLo + m]; }, [&](int m) { return qj[kLo + m]; });
            }
        };

        if (lo >= 0 && hi < (long long)ns) {
            plain(x + (size_t)ch * (size_t)pitch + q0, PHASE ? y + (size_t)ch * (size_t)pitchy + q0 : nullptr);
        } else if (lo >= (long long)ns && hi < ntot) {
            plain(xn + (size_t)ch * (size_t)pitchn + (q0 - (long long)ns),
                  PHASE ? yn + (size_t)ch * (size_t)pitchyn + (q0 - (long long)ns) : nullptr);
        } else {                                             // across an end of the record or the seam: every term is tested
            const float* __restrict__ row = x + (size_t)ch * (size_t)pitch;
            const float* __restrict__ rown = xn ? xn + (size_t)ch * (size_t)pitchn : nullptr;
            const float* __restrict__ rowy = PHASE ? y + (size_t)ch * (size_t)pitchy : nullptr;
            const float* __restrict__ rowyn = PHASE && yn ? yn + (size_t)ch * (size_t)pitchyn : nullptr;
#pragma unroll
            for (int j = 0; j < kCohCpt; ++j) {
                const long long q = q0 + tid + j * kCohThreads;
                if (q + kLo < 0 || q + kHi >= ntot) continue;
                term(j, [&](int m) { const long long i = q + kLo + m; return i < (long long)ns ? row[i] : rown[i - (long long)ns]; },
                     [&](int m) { const long long i = q + kLo + m; return i < (long long)ns ? rowy[i] : rowyn[i - (long long)ns]; });
            }
        }
    }

    const size_t step = (size_t)ncalls * (size_t)nt, plane = (size_t)nseg * step;
#pragma unroll
    for (int j = 0; j < kCohCpt; ++j) {
        const long long col = col0 + tid + j * kCohThreads;
        if (col >= nt) continue;
        const size_t o = (size_t)seg * step + (size_t)c * (size_t)nt + (size_t)col;
        part[o] = b[j];
        part[plane + o] = e[j];
        part[2 * plane + o] = wsum[j];
        if constexpr (PHASE) {
            part[3 * plane + o] = pr[j];
            part[4 * plane + o] = pi[j];
        }
    }
}

// grid (ceil(nt / 256), ncalls), dynamic LDS 2 (256 + 2 H) floats.  phase (PHASE only), wsum: or NULL
template <bool PHASE>
__global__ __launch_bounds__(kCohThreads) void coh_finish(const float* __restrict__ part, int nseg, int ncalls, int nt, int H,
                                                          float* __restrict__ beam, float* __restrict__ semb, float* __restrict__ phase,
                                                          float* __restrict__ wout) {
    D4W_DYN_LDS(smem);
    const int span = kCohFinishTile + 2 * H;
    float* q = reinterpret_cast<float*>(smem);
    float* d = q + span;
    const int tid = threadIdx.x, c = blockIdx.y;
    const long long col0 = (long long)blockIdx.x * kCohFinishTile;
    const size_t step = (size_t)ncalls * (size_t)nt, plane = (size_t)nseg * step;

    for (int i = tid; i < span; i += kCohThreads) {
        const long long col = col0 - H + i;
        float qq = 0.f, dd = 0.f;
        if (col >= 0 && col < nt) {
            const size_t o = (size_t)c * (size_t)nt + (size_t)col;
            float b = part[o], e = part[plane + o], w = part[2 * plane + o];
            for (int s = 1; s < nseg; ++s) {                 // increasing segment order, as beam_reduce
                b += part[o + (size_t)s * step];
                e += part[plane + o + (size_t)s * step];
                w += part[2 * plane + o + (size_t)s * step];
            }
            qq = b * b;
            dd = w * e;
            if (i >= H && i < H + kCohFinishTile) {          // the tile's own columns
                beam[o] = b;
                if (wout) wout[o] = w;
                if constexpr (PHASE) {
                    float pr = part[3 * plane + o], pi = part[4 * plane + o];
                    for (int s = 1; s < nseg; ++s) {
                        pr += part[3 * plane + o + (size_t)s * step];
                        pi += part[4 * plane + o + (size_t)s * step];
                    }
                    phase[o] = w != 0.f ? sqrtf(fmaf(pr, pr, pi * pi)) / w : 0.f;
                }
            }
        }
        q[i] = qq;
        d[i] = dd;
    }
    __syncthreads();
    const long long col = col0 + tid;                        // the window of column col0 + tid is q[tid .. tid + 2 H]
    if (col >= nt) return;
    float sq = 0.f, sd = 0.f;
    for (int t = 0; t <= 2 * H; ++t) {                       // increasing tau
        sq += q[tid + t];
        sd += d[tid + t];
    }
    semb[(size_t)c * (size_t)nt + (size_t)col] = sd != 0.f ? sq / sd : 0.f;
}

// grid (ncalls).  semb [ncalls][nt]; peak, index [ncalls]: the largest value over [lo, hi) and the smallest column that has it
__global__ __launch_bounds__(kCohThreads) void coh_peak(const float* __restrict__ semb, int nt, int lo, int hi, float* __restrict__ peak,
                                                        int* __restrict__ index) {
    __shared__ float sv[kCohThreads];
    __shared__ int si[kCohThreads];
    const int tid = threadIdx.x, c = blockIdx.x;
    const float* __restrict__ row = semb + (size_t)c * (size_t)nt;
    float best = -1.f;                                       // below every semblance; a NaN is never taken
    int at = hi;
    for (int j = lo + tid; j < hi; j += kCohThreads) {
        const float v = row[j];
        if (v > best) {
            best = v;
            at = j;
        }
    }
    sv[tid] = best;
    si[tid] = at;
    __syncthreads();
    for (int s = kCohThreads / 2; s >= 1; s >>= 1) {
        if (tid < s) {
            const float v = sv[tid + s];
            const int k = si[tid + s];
            if (v > sv[tid] || (v == sv[tid] && k < si[tid])) {
                sv[tid] = v;
                si[tid] = k;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const bool none = si[0] >= hi;                       // nothing but NaN in the range
        peak[c] = none ? __int_as_float(0x7fc00000) : sv[0];
        index[c] = none ? -1 : si[0];
    }
}

static int coh_check_shape(const char* who, int nch, int ncalls, int length) {
    if (nch < 1 || nch > 65535 * kCohSegment) return fail(D4W_EINVAL, "%s: %d channels, a launch takes 1 .. %d", who, nch, 65535 * kCohSegment);
    if (ncalls < 1 || ncalls > kCohMaxCalls) return fail(D4W_EINVAL, "%s: %d calls, a launch takes 1 .. %d", who, ncalls, kCohMaxCalls);
    if (length < 1 || length > kCohMaxLength) return fail(D4W_EINVAL, "%s: the length %d is outside 1 .. %d", who, length, kCohMaxLength);
    return D4W_OK;
}

static size_t coh_plane_words(int nch, int ncalls, int length) {
    return (size_t)ceil_div(nch, kCohSegment) * (size_t)ncalls * (size_t)length;
}

template <int ORDER>
static int coh_launch(const float* x, long long pitch, int nch, int ns, const float* xn, long long pitchn, int nsn, const float* y,
                      long long pitchy, const float* yn, long long pitchyn, const int32_t* kr, const float* fr, const float* weights,
                      const int64_t* start, int ncalls, int nt, int H, float* beam, float* semb, float* phase, float* wsum, float* part,
                      void* stream) {
    const int nseg = ceil_div(nch, kCohSegment);
    const dim3 grid(ceil_div(nt, kCohTile), nseg, ncalls), fgrid(ceil_div(nt, kCohFinishTile), ncalls);
    const size_t lds = 2 * (size_t)(kCohFinishTile + 2 * H) * sizeof(float);
    if (y) {
        D4W_LAUNCH((coh_sum<ORDER, true>), grid, dim3(kCohThreads), 0, stream, x, pitch, nch, ns, xn, pitchn, nsn, y, pitchy, yn, pitchyn,
                   (const int*)kr, fr, weights, (const long long*)start, ncalls, nt, nseg, part);
        D4W_LAUNCH((coh_finish<true>), fgrid, dim3(kCohThreads), lds, stream, (const float*)part, nseg, ncalls, nt, H, beam, semb, phase, wsum);
    } else {
        D4W_LAUNCH((coh_sum<ORDER, false>), grid, dim3(kCohThreads), 0, stream, x, pitch, nch, ns, xn, pitchn, nsn, y, pitchy, yn, pitchyn,
                   (const int*)kr, fr, weights, (const long long*)start, ncalls, nt, nseg, part);
        D4W_LAUNCH((coh_finish<false>), fgrid, dim3(kCohThreads), lds, stream, (const float*)part, nseg, ncalls, nt, H, beam, semb, phase, wsum);
    }
    return D4W_OK;
}

}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_coherence_limits(int* max_calls, int* max_length, int* max_half_window, int* segment) {
    if (!max_calls || !max_length || !max_half_window || !segment) return fail(D4W_EINVAL, "bad argument");
    *max_calls = kCohMaxCalls;
    *max_length = kCohMaxLength;
    *max_half_window = kCohMaxHalf;
    *segment = kCohSegment;
    return D4W_OK;
}

int d4w_coherence_ws_bytes(int nch, int ncalls, int length, int phase, size_t* bytes) {
    if (!bytes) return fail(D4W_EINVAL, "bad argument");
    const int rc = coh_check_shape("coherence_ws_bytes", nch, ncalls, length);
    if (rc) return rc;
    *bytes = (phase ? 5 : 3) * coh_plane_words(nch, ncalls, length) * sizeof(float);
    return D4W_OK;
}

int d4w_coherence_f32(const float* x, int64_t pitch, int nch, int ns, const float* xnext, int64_t pitch_next, int ns_next, const float* ximag,
                      int64_t pitch_imag, const float* ximag_next, int64_t pitch_imag_next, const int32_t* k_or_r, const float* f,
                      const float* weights, const int64_t* start, int ncalls, int length, int order, int half_window, float* beam,
                      float* semblance, float* phase, float* wsum, void* ws, void* stream) {
    if (!x || !k_or_r || !start || !beam || !semblance || !ws) return fail(D4W_EINVAL, "bad argument");
    if (order != 0 && order != 1 && order != 3) return fail(D4W_EINVAL, "coherence: order %d is none of 0, 1, 3", order);
    if (order != 0 && !f) return fail(D4W_EINVAL, "coherence: order %d needs the fractions f", order);
    if (half_window < 0 || half_window > kCohMaxHalf)
        return fail(D4W_EINVAL, "coherence: the half window %d is outside 0 .. %d", half_window, kCohMaxHalf);
    int rc = coh_check_shape("coherence", nch, ncalls, length);
    if (rc) return rc;
    rc = check_record("coherence", nch, ns, pitch, xnext, ns_next, pitch_next);
    if (rc) return rc;
    if ((ximag == nullptr) != (phase == nullptr)) return fail(D4W_EINVAL, "coherence: the imaginary block and the phase output come together");
    if (ximag) {
        if (pitch_imag < ns) return fail(D4W_EINVAL, "coherence: the row pitch %lld of the imaginary block is below the %d samples of a row",
                                         (long long)pitch_imag, ns);
        if ((ximag_next == nullptr) != (xnext == nullptr))
            return fail(D4W_EINVAL, "coherence: a next imaginary block is given if and only if a next block is");
        if (ximag_next && pitch_imag_next < ns_next)
            return fail(D4W_EINVAL, "coherence: the row pitch %lld of the next imaginary block is below the %d samples of a row",
                        (long long)pitch_imag_next, ns_next);
    } else if (ximag_next) {
        return fail(D4W_EINVAL, "coherence: a next imaginary block without an imaginary block");
    }
    if (weights) {                                           // one small copy to the host: finite and >= 0, before any launch
        std::vector<float> w((size_t)nch);
        D4W_HIP(hipMemcpyAsync(w.data(), weights, (size_t)nch * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
        D4W_HIP(hipStreamSynchronize((hipStream_t)stream));
        for (int ch = 0; ch < nch; ++ch)
            if (!(std::isfinite(w[ch]) && w[ch] >= 0.f)) return fail(D4W_EINVAL, "coherence: weights[%d] = %g is not finite and >= 0", ch, (double)w[ch]);
    }
    const int nsn = xnext ? ns_next : 0;
    float* part = (float*)ws;
#define D4W_COH_ARGS                                                                                                                         \
    x, pitch, nch, ns, xnext, pitch_next, nsn, ximag, pitch_imag, ximag_next, pitch_imag_next, k_or_r, f, weights, start, ncalls, length,   \
        half_window, beam, semblance, phase, wsum, part, stream
    if (order == 0) return coh_launch<0>(D4W_COH_ARGS);
    if (order == 1) return coh_launch<1>(D4W_COH_ARGS);
    return coh_launch<3>(D4W_COH_ARGS);
#undef D4W_COH_ARGS
}

int d4w_coherence_peak_f32(const float* semblance, int ncalls, int length, int lo, int hi, float* peak, int32_t* index, void* stream) {
    if (!semblance || !peak || !index) return fail(D4W_EINVAL, "bad argument");
    if (ncalls < 1 || ncalls > kCohMaxCalls) return fail(D4W_EINVAL, "coherence_peak: %d calls, a launch takes 1 .. %d", ncalls, kCohMaxCalls);
    if (length < 1 || length > kCohMaxLength) return fail(D4W_EINVAL, "coherence_peak: the length %d is outside 1 .. %d", length, kCohMaxLength);
    if (lo < 0 || hi <= lo || hi > length) return fail(D4W_EINVAL, "coherence_peak: the range [%d, %d) is not inside [0, %d)", lo, hi, length);
    D4W_LAUNCH(coh_peak, dim3(ncalls), dim3(kCohThreads), 0, stream, semblance, length, lo, hi, peak, (int*)index);
    return D4W_OK;
}

}  // extern "C"
