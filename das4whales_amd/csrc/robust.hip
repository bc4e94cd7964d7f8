// Robust weighted relocation on MI355X (gfx950): iteratively reweighted least squares (IRLS) around loc.hip's damped
// Gauss-Newton, batched over calls.  Beyond the reference, which has one unweighted solver; DESIGN.md 3.9e.
//
//   used(c, ch)  iff Ti[c][ch] is not NaN and weights[c][ch] > 0 (a NaN, zero or negative weight: not used).  An unused
//                channel's Ti and cable row are never read into a sum and may hold anything.
//   iteration j = 0 .. Nbiter - 1 at the iterate n, g and R exactly loc_common.h's loc_row, the travel time R / c0:
//     r  = Ti - (n3 + R / c0)
//     q  = 1 when loss = l2 or j < warmup; else with s = scale when one is given, else 1.4826 median |r| over the used
//          channels (the exact median: for an even count (a + b) * 0.5 of the two middle order statistics); s not > 0: q = 1;
//          else u = |r| / (tuning s):  huber q = 1 (u <= 1), 1 / u;   bisquare q = (1 - u^2)^2 (u < 1), 0
//     w  = weights q;  A = sum w g g^T + 1e-5 I;  b = sum w g r;  dn = A^-1 b (loc_solve_spd);  n += 0.7 dn (j < 4), dn after
//   final pass at the returned n, q as an iteration j >= warmup forms it: sum w g g^T without lambda, sum w r^2, sum w, the used
//   count, s, and q and r per channel.
//
// robust_solve<FIXZ, RES>: ONE workgroup (256 threads) per call, the whole iteration inside the kernel, as loc_solve.  A plain
//   robust iteration is two sweeps over the channels and a selection between them:
//   sweep 1  every thread strides over the channels (ch = tid, tid + 256, ...), computes |r| and keeps its bit pattern as a
//            64-bit key (non-negative doubles order like their unsigned integers) at keys[ch]: in LDS while the call's channels
//            fit (RES, nch <= 16 384: 8 nch bytes of dynamic LDS, 88 KB at 11 020 channels), else in a row of a global
//            workspace.  A thread reads back only the keys it wrote itself.  With them the used count m and the smallest and
//            largest key (wave shuffles, four partials through LDS).
//   select   the order statistic of rank (m - 1) / 2 by a radix select on the keys, most significant digit first, 8 bits per
//            pass: the bits that the smallest and the largest key share are skipped (the sign, most of the exponent); per pass
//            the keys that still match the prefix are counted into 256 LDS bins with integer atomics (counts do not depend on
//            the order of arrival), thread t owns bin t, an inclusive scan over the bins (wave shuffles, four wave totals) finds
//            the bin that holds the rank.  Once at most 256 keys match the prefix they are gathered, one per thread, and ranked
//            against each other (a count of the smaller and of the equal ones), which replaces the remaining passes: at 11 020
//            channels two digit passes, not seven.  All keys equal: no pass.  The second middle statistic of an even m is the same value
//            when the last bin holds another key past the rank, else the smallest key above it (one more sweep of the keys).
//   sweep 2  loc_solve's sweep with w: s[q] = fma(w g_i, g_k, s[q]), fma(w g_i, r, .), fma(w r, r, .), sum w, the used count.
//            w = 1.0 multiplies exactly, so with loss = l2 and no weights the sums, their wave / LDS reduction order and the
//            solve are loc_solve's, and n, the history, G^T G, the residual sum and the count equal its bits.
//   With a given scale, loss = l2 or j < warmup there is no sweep 1.  Every sum has a fixed order, the select is integer work:
//   run-to-run bit-identical, independent of the other calls of the batch.
#include "loc_common.h"

#ifndef D4W_EMU
#pragma clang fp contract(off)
#endif

namespace d4w {

constexpr int kRobustSums = 17;                  // 10 + 4 + 3 (free z); 6 + 3 + 3 with fix_z
constexpr int kRobustResident = 16384;           // channels whose keys stay in LDS: 128 KB of the compute unit's 160
constexpr int kRobustDigitBits = 8;              // one bin per thread
constexpr int kRobustBins = 1 << kRobustDigitBits;
constexpr unsigned long long kRobustUnused = ~0ull;      // above every key: |r| has no sign bit
constexpr double kRobustMad = 1.4826;            // median absolute deviation -> standard deviation of a normal distribution
enum { kRobustL2 = 0, kRobustHuber = 1, kRobustBisquare = 2 };
static_assert(kRobustBins == kLocThreads, "thread t owns bin t");

__device__ __forceinline__ unsigned long long robust_key(double a) {
    unsigned long long k;
    memcpy(&k, &a, 8);
    return k;
}
__device__ __forceinline__ double robust_value(unsigned long long k) {
    double a;
    memcpy(&a, &k, 8);
    return a;
}

// The arrival time, weight and cable row of kRobustUnroll of a thread's channels (base, base + 256, ...), loaded before any of
// them is used: at one workgroup per compute unit nothing else hides the latency of these loads.  Past the last channel the
// loads go to channel 0 and the entry reads as unused.
constexpr int kRobustUnroll = 4;
struct RobustRows {
    double tt[kRobustUnroll], w0[kRobustUnroll], cx[kRobustUnroll], cy[kRobustUnroll], cz[kRobustUnroll];
    __device__ __forceinline__ void load(const double* __restrict__ t, const double* __restrict__ wt, const double* __restrict__ cable, int base,
                                         int nch) {
#pragma unroll
        for (int u = 0; u < kRobustUnroll; ++u) {
            const int ch = base + u * kLocThreads;
            const size_t c = ch < nch ? (size_t)ch : 0;
            tt[u] = t[c];
            w0[u] = wt ? wt[c] : 1.0;
            cx[u] = cable[3 * c];
            cy[u] = cable[3 * c + 1];
            cz[u] = cable[3 * c + 2];
            if (ch >= nch) tt[u] = NAN;
        }
    }
    __device__ __forceinline__ bool used(int u) const { return tt[u] == tt[u] && w0[u] > 0.0; }
};

// the robust weight of |r| = ar with cs = tuning s; formed = (s > 0)
__device__ __forceinline__ double robust_q(int loss, bool formed, double ar, double cs) {
    if (!formed) return 1.0;
    const double u = ar / cs;
    if (loss == kRobustHuber) return u <= 1.0 ? 1.0 : 1.0 / u;
    const double v = 1.0 - u * u;
    return u < 1.0 ? v * v : 0.0;
}

// The median of the m >= 1 used keys among keys[0 .. nch) (unused entries hold kRobustUnused), kmin and kmax the smallest and
// largest used key.  Called by every thread of the workgroup with the same arguments; every thread returns the same value.
// hist [256], wtot [4], sel [4], cand [256], ncand [1]: LDS.
__device__ __forceinline__ double robust_median(const unsigned long long* keys, int nch, int m, unsigned long long kmin,
                                                unsigned long long kmax, int* hist, int* wtot, unsigned long long* sel,
                                                unsigned long long* cand, int* ncand) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (kmin == kmax) return robust_value(kmin);
    int top = 63 - __builtin_clzll(kmin ^ kmax);             // the highest bit in which two used keys differ; <= 62
    unsigned long long mask = ~0ull << (top + 1), prefix = kmin & mask;
    int k = (m - 1) / 2, cnt = m;                            // the rank among the keys that match the prefix, and their number
    while (top >= 0) {
        if (cnt <= kRobustBins) {
            // At most one candidate per thread is left: they are gathered (in an order that does not matter: only values are
            // compared) and thread i ranks candidate i against all of them, which replaces the remaining digit passes.
            if (tid == 0) *ncand = 0;
            __syncthreads();
#pragma unroll 4
            for (int ch = tid; ch < nch; ch += kLocThreads) {
                const unsigned long long key = keys[ch];
                if ((key & mask) == prefix) {
                    const int slot = atomicAdd(ncand, 1);
                    if (slot < kRobustBins) cand[slot] = key;       // always: cnt keys match
                }
            }
            __syncthreads();
            if (tid < cnt) {
                const unsigned long long mine = cand[tid];
                int lt = 0, eq = 0;
                for (int i = 0; i < cnt; ++i) {
                    const unsigned long long o = cand[i];
                    lt += o < mine;
                    eq += o == mine;
                }
                if (lt <= k && k < lt + eq) {                // the threads that hold this value all write the same words
                    sel[0] = mine;
                    sel[1] = (unsigned long long)(k - lt);
                    sel[2] = (unsigned long long)eq;
                }
            }
            __syncthreads();
            prefix = sel[0];
            k = (int)sel[1];
            cnt = (int)sel[2];
            break;
        }
        const int shift = top >= kRobustDigitBits ? top - (kRobustDigitBits - 1) : 0;
        const unsigned dmask = (1u << (top - shift + 1)) - 1u;
        hist[tid] = 0;
        __syncthreads();
#pragma unroll 4
        for (int ch = tid; ch < nch; ch += kLocThreads) {
            const unsigned long long key = keys[ch];
            if ((key & mask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & dmask], 1);
        }
        __syncthreads();
        const int c = hist[tid];
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        for (int w = 0; w < wave; ++w) incl += wtot[w];
        const int excl = incl - c;
        if (excl <= k && k < incl) {                         // one thread: the bins partition the matching keys
            sel[0] = (unsigned long long)tid;
            sel[1] = (unsigned long long)(k - excl);
            sel[2] = (unsigned long long)c;
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        k = (int)sel[1];
        cnt = (int)sel[2];
        mask |= (unsigned long long)dmask << shift;
        top = shift - 1;
    }
    const double a = robust_value(prefix);                   // cnt keys equal it, the rank is the k-th of them
    if ((m & 1) || k + 1 < cnt) return (a + a) * 0.5;
    unsigned long long b = kRobustUnused;                    // the smallest key above a: rank m / 2
    for (int ch = tid; ch < nch; ch += kLocThreads) {
        const unsigned long long key = keys[ch];
        if (key > prefix && key < b) b = key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = __shfl_down(b, o);
        if (v < b) b = v;
    }
    __syncthreads();                                         // sel was read above by every thread
    if (lane == 0) sel[wave] = b;
    __syncthreads();
    b = sel[0];
    for (int w = 1; w < kLocWaves; ++w) b = sel[w] < b ? sel[w] : b;
    __syncthreads();
    return (a + robust_value(b)) * 0.5;
}

// grid = ncalls.  weights NULL, [nch] (wpitch = 0) or [ncalls][nch] (wpitch = nch); scale = 0: from the median.
// hist [ncalls][nbiter][4], out_n [ncalls][4], gtg [ncalls][NP][NP], ssr, wsum_out, scale_out [ncalls], nused [ncalls],
// q_out, r_out [ncalls][nch]; wsum_out, scale_out, q_out, r_out each or NULL.  ws [ncalls][nch] keys when !RES.
template <bool FIXZ, bool RES>
__global__ __launch_bounds__(kLocThreads) void robust_solve(const double* __restrict__ cable, int nch, const double* __restrict__ Ti,
                                                            const double* __restrict__ weights, long long wpitch, double c0, int nbiter,
                                                            int warmup, int loss, double tuning, double scale,
                                                            const double* __restrict__ first_guess, double* __restrict__ hist,
                                                            double* __restrict__ out_n, double* __restrict__ gtg, double* __restrict__ ssr,
                                                            double* __restrict__ wsum_out, int* __restrict__ nused,
                                                            double* __restrict__ scale_out, double* __restrict__ q_out,
                                                            double* __restrict__ r_out, unsigned long long* __restrict__ ws) {
    constexpr int NP = FIXZ ? 3 : 4;
    constexpr int NT = NP * (NP + 1) / 2;
    constexpr int NS = NT + NP + 3;              // + sum w r^2 + used count + sum w
    D4W_DYN_LDS(smem);
    __shared__ double wsum[kLocWaves * kRobustSums];
    __shared__ double n_sh[4];
    __shared__ int bins[kRobustBins];
    __shared__ int wtot[kLocWaves];
    __shared__ unsigned long long sel[kLocWaves];
    __shared__ unsigned long long kred[2 * kLocWaves];
    __shared__ int mred[kLocWaves];
    __shared__ unsigned long long cand[kRobustBins];
    __shared__ int ncand;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t call = blockIdx.x;
    const double* __restrict__ t = Ti + call * (size_t)nch;
    const double* __restrict__ wt = weights ? weights + call * (size_t)wpitch : nullptr;
    unsigned long long* keys = RES ? reinterpret_cast<unsigned long long*>(smem) : ws + call * (size_t)nch;

    if (first_guess) {
        if (tid < 4) n_sh[tid] = first_guess[call * 4 + tid];
    } else {                                     // loc.py:86, the minimum over the used channels
        double m = INFINITY;
        for (int ch = tid; ch < nch; ch += kLocThreads) {
            const double v = t[ch];
            if (v == v && (!wt || wt[ch] > 0.0)) m = fmin(m, v);
        }
        m = loc_wave_min(m);
        if (lane == 0) wsum[wave] = m;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kLocWaves; ++w) m = fmin(m, wsum[w]);
            n_sh[0] = 40000.0;
            n_sh[1] = 23000.0;
            n_sh[2] = -60.0;
            n_sh[3] = m;
        }
    }
    __syncthreads();

    for (int j = 0; j <= nbiter; ++j) {
        const double n0 = n_sh[0], n1 = n_sh[1], n2 = n_sh[2], n3 = n_sh[3];
        const bool last = j == nbiter;
        const bool robust = loss != kRobustL2 && (last || j >= warmup);
        double sc = NAN;                         // the scale of this pass; NaN where q is not formed
        if (robust) {
            if (scale > 0.0) {
                sc = scale;
            } else {                             // sweep 1: the keys of |r|, their count and range
                int m = 0;
                unsigned long long kmin = kRobustUnused, kmax = 0ull;
                for (int base = tid; base < nch; base += kRobustUnroll * kLocThreads) {
                    RobustRows in;
                    in.load(t, wt, cable, base, nch);
#pragma unroll
                    for (int u = 0; u < kRobustUnroll; ++u) {
                        const int ch = base + u * kLocThreads;
                        if (ch >= nch) break;
                        unsigned long long key = kRobustUnused;
                        if (in.used(u)) {
                            const double R = moveout_dist(n0, n1, n2, in.cx[u], in.cy[u], in.cz[u]);
                            key = robust_key(fabs(in.tt[u] - (n3 + R / c0)));
                            kmin = key < kmin ? key : kmin;
                            kmax = key > kmax ? key : kmax;
                            ++m;
                        }
                        keys[ch] = key;
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const unsigned long long a = __shfl_down(kmin, o), b = __shfl_down(kmax, o);
                    m += __shfl_down(m, o);
                    kmin = a < kmin ? a : kmin;
                    kmax = b > kmax ? b : kmax;
                }
                if (lane == 0) {
                    kred[wave] = kmin;
                    kred[kLocWaves + wave] = kmax;
                    mred[wave] = m;
                }
                __syncthreads();
                m = mred[0];
                kmin = kred[0];
                kmax = kred[kLocWaves];
                for (int w = 1; w < kLocWaves; ++w) {
                    m += mred[w];
                    kmin = kred[w] < kmin ? kred[w] : kmin;
                    kmax = kred[kLocWaves + w] > kmax ? kred[kLocWaves + w] : kmax;
                }
                __syncthreads();                 // kred and mred are free for the next pass
                if (m > 0) sc = kRobustMad * robust_median(keys, nch, m, kmin, kmax, bins, wtot, sel, cand, &ncand);
            }
        }
        const bool formed = sc > 0.0;
        const double cs = tuning * sc;

        double s[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) s[i] = 0.0;
        for (int base = tid; base < nch; base += kRobustUnroll * kLocThreads) {
            RobustRows in;
            in.load(t, wt, cable, base, nch);
#pragma unroll
            for (int u = 0; u < kRobustUnroll; ++u) {        // in channel order: the chains of loc_solve
                const int ch = base + u * kLocThreads;
                if (ch >= nch) break;
                if (!in.used(u)) {
                    if (last) {
                        if (q_out) q_out[call * (size_t)nch + ch] = NAN;
                        if (r_out) r_out[call * (size_t)nch + ch] = NAN;
                    }
                    continue;
                }
                double g[4], R;
                loc_row(n0, n1, n2, in.cx[u], in.cy[u], in.cz[u], c0, g[0], g[1], g[2], R);
                if (FIXZ) g[2] = 1.0; else g[3] = 1.0;
                const double dt = in.tt[u] - (n3 + R / c0);
                const double qq = robust ? robust_q(loss, formed, fabs(dt), cs) : 1.0;
                const double w = in.w0[u] * qq;
                if (last) {
                    if (q_out) q_out[call * (size_t)nch + ch] = qq;
                    if (r_out) r_out[call * (size_t)nch + ch] = dt;
                }
                int q = 0;
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    const double wg = w * g[i];
#pragma unroll
                    for (int k = i; k < NP; ++k) {
                        s[q] = fma(wg, g[k], s[q]);
                        ++q;
                    }
                }
#pragma unroll
                for (int i = 0; i < NP; ++i) s[NT + i] = fma(w * g[i], dt, s[NT + i]);
                s[NT + NP] = fma(w * dt, dt, s[NT + NP]);
                s[NT + NP + 1] += 1.0;
                s[NT + NP + 2] += w;
            }
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            s[i] = loc_wave_sum(s[i]);
            if (lane == 0) wsum[wave * kRobustSums + i] = s[i];
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < NS; ++i)
                for (int w = 1; w < kLocWaves; ++w) s[i] += wsum[w * kRobustSums + i];
            const bool none = !(s[NT + NP + 1] > 0.0);       // a call without a used channel: a NaN row
            if (last) {
                double* G = gtg + call * (NP * NP);
                int q = 0;
#pragma unroll
                for (int i = 0; i < NP; ++i)
#pragma unroll
                    for (int k = i; k < NP; ++k) {
                        G[i * NP + k] = s[q];
                        G[k * NP + i] = s[q];
                        ++q;
                    }
                ssr[call] = s[NT + NP];
                nused[call] = (int)s[NT + NP + 1];
                if (wsum_out) wsum_out[call] = s[NT + NP + 2];
                if (scale_out) scale_out[call] = sc;
                out_n[call * 4 + 0] = none ? NAN : n0;
                out_n[call * 4 + 1] = none ? NAN : n1;
                out_n[call * 4 + 2] = none ? NAN : n2;
                out_n[call * 4 + 3] = none ? NAN : n3;
            } else {
                int q = 0;
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    s[q] += kLocLambda;                      // the diagonal entries of the upper triangle
                    q += NP - i;
                }
                double dn[NP];
                loc_solve_spd<NP>(s, s + NT, dn);
                const double f = j < 4 ? 0.7 : 1.0;          // loc.py:117-120
                double nn[4] = {n0, n1, n2, n3};
                nn[0] += f * dn[0];
                nn[1] += f * dn[1];
                if (FIXZ) nn[3] += f * dn[2];
                else { nn[2] += f * dn[2]; nn[3] += f * dn[3]; }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (none) nn[i] = NAN;
                    n_sh[i] = nn[i];
                    hist[(call * (size_t)nbiter + j) * 4 + i] = nn[i];
                }
            }
        }
        __syncthreads();
    }
}

template <bool FIXZ, bool RES>
static int robust_launch(const double* cable_pos, int nch, const double* Ti, int ncalls, const double* weights, long long wpitch, double c0,
                         int nbiter, int warmup, int loss, double tuning, double scale, const double* first_guess, double* history,
                         double* n_out, double* gtg, double* ssr, double* wsum, int* nused, double* scale_out, double* q_out, double* r_out,
                         void* ws, void* stream) {
    // the keys are needed only where a median is taken: l2 and a given scale run with loc_solve's occupancy
    const size_t lds = RES && loss != kRobustL2 && scale == 0.0 ? sizeof(unsigned long long) * (size_t)nch : 0;
    // above 64 KiB a kernel has to opt into its dynamic LDS size; a refused opt-in is this call's error, before any launch
    if (lds > 48 * 1024)
        D4W_HIP(hipFuncSetAttribute((const void*)robust_solve<FIXZ, RES>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    D4W_LAUNCH((robust_solve<FIXZ, RES>), dim3(ncalls), dim3(kLocThreads), lds, stream, cable_pos, nch, Ti, weights, wpitch, c0, nbiter,
               warmup, loss, tuning, scale, first_guess, history, n_out, gtg, ssr, wsum, nused, scale_out, q_out, r_out,
               (unsigned long long*)ws);
    return D4W_OK;
}

}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_loc_robust_limits(int* resident_channels, int* digit_bits) {
    if (!resident_channels || !digit_bits) return fail(D4W_EINVAL, "bad argument");
    *resident_channels = kRobustResident;
    *digit_bits = kRobustDigitBits;
    return D4W_OK;
}

int d4w_loc_robust_ws_bytes(int nch, int ncalls, size_t* bytes) {
    if (!bytes) return fail(D4W_EINVAL, "bad argument");
    if (nch < 1 || ncalls < 0) return fail(D4W_EINVAL, "loc_robust: %d channels, %d calls", nch, ncalls);
    *bytes = nch > kRobustResident ? sizeof(unsigned long long) * (size_t)nch * (size_t)ncalls : 0;
    return D4W_OK;
}

int d4w_loc_robust_f64(const double* cable_pos, int nch, const double* Ti, int ncalls, const double* weights, int weights_per_call,
                       double c0, int nbiter, int warmup, int fix_z, int loss, double tuning, double scale, const double* first_guess,
                       double* history, double* n_out, double* gtg, double* ssr, double* wsum, int* nused, double* scale_out,
                       double* robust_weights, double* residuals, void* ws, void* stream) {
    if (!cable_pos || !Ti || !n_out || !gtg || !ssr || !nused) return fail(D4W_EINVAL, "bad argument");
    if (nch < 1) return fail(D4W_EINVAL, "loc_robust: %d channels", nch);
    if (ncalls < 0) return fail(D4W_EINVAL, "loc_robust: %d calls", ncalls);
    if (!positive_finite(c0)) return fail(D4W_EINVAL, "loc_robust: the speed of sound must be positive and finite");
    if (nbiter < 0 || nbiter > 100000) return fail(D4W_EINVAL, "loc_robust: Nbiter = %d is not within 0 .. 100000", nbiter);
    if (nbiter > 0 && !history) return fail(D4W_EINVAL, "loc_robust: the history of %d iterations needs its output", nbiter);
    if (warmup < 0) return fail(D4W_EINVAL, "loc_robust: warmup = %d is negative", warmup);
    if (loss != kRobustL2 && loss != kRobustHuber && loss != kRobustBisquare)
        return fail(D4W_EINVAL, "loc_robust: loss %d is not 0 (l2), 1 (huber) or 2 (bisquare)", loss);
    if (!positive_finite(tuning)) return fail(D4W_EINVAL, "loc_robust: tuning must be positive and finite");
    if (scale != 0.0 && !positive_finite(scale)) return fail(D4W_EINVAL, "loc_robust: scale must be 0 (estimate it) or positive and finite");
    if (weights_per_call && !weights) return fail(D4W_EINVAL, "loc_robust: weights per call that are not given");
    const bool res = nch <= kRobustResident;
    if (!res && !ws && loss != kRobustL2 && scale == 0.0)
        return fail(D4W_EINVAL, "loc_robust: %d channels exceed the %d kept in LDS and need the workspace", nch, kRobustResident);
    if (ncalls == 0) return D4W_OK;
    const long long wpitch = weights_per_call ? nch : 0;
#define D4W_ROBUST(FZ, RS)                                                                                                      \
    return robust_launch<FZ, RS>(cable_pos, nch, Ti, ncalls, weights, wpitch, c0, nbiter, warmup, loss, tuning, scale, first_guess, \
                                 history, n_out, gtg, ssr, wsum, nused, scale_out, robust_weights, residuals, ws, stream)
    if (fix_z) {
        if (res) D4W_ROBUST(true, true);
        D4W_ROBUST(true, false);
    }
    if (res) D4W_ROBUST(false, true);
    D4W_ROBUST(false, false);
#undef D4W_ROBUST
}

}  // extern "C"
