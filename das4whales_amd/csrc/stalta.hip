// STA/LTA energy detector and its on/off trigger (no reference counterpart): the template-free first pass over
// a [channel x time] block.  With e[i] = x[i]^2 (the float32 sample widened to float64: the square is exact),
//   classic     STA[i] = mean e[i-nsta+1 .. i],  LTA[i] = mean e[i-gap-nlta+1 .. i-gap]
//   recursive   sta[i] = sta[i-1] + (e[i] - sta[i-1]) / nsta,  lta likewise with nlta
//   r[i] = STA / LTA  where the windows lie in known samples (recursive: nlta samples seen) and LTA > (floor A)^2,  0 elsewhere
// and the trigger turns r into events with two thresholds per row (ON above thr_on, OFF below thr_off, KEEP between them).
//
// One kernel, stalta_rows<SRC, WR, TRG>: a workgroup WALKS one row in tiles of kSlTile = 2048 samples, a thread owns 8 consecutive
// samples of the tile.  SRC says where the tile's ratios come from (the classic windows, the recursive scan, or a ratio that is
// read), WR whether they are written, TRG whether the trigger runs on them -- in registers, so the fused form (SRC = classic or
// recursive, TRG, no WR) forms every ratio with the very instructions of the ratio-only form and writes none.  Walking the row
// makes everything that crosses a tile a register of the workgroup (the recurrences' state, the trigger's flag, the open event
// and its running peak, the row's event count): there are no tile summaries to stitch in a second launch, at the price of one
// workgroup per row (blocks of thousands of channels fill the device; a block of 8 channels does not, and need not).
//
// Numerics of the classic windows.  A float64 prefix over the tile carries the rounding of everything since the tile's start
// into a window that may hold nothing (nmf.hip's header); a sliding sum carries the rounding of what has LEFT the window, and
// a window of exact zeros behind a loud stretch then holds 1e-8 instead of 0.  Here every window sum is a sum of parts OF THAT
// WINDOW, all non-negative:
//   1. the tile's samples and the max(nsta, nlta + gap) - 1 before them are staged in LDS as float32 (runs of 8, one pad word
//      per run, as nmf.hip), with float64 sums of squares of every run, of every 8 runs and of every 64 runs;
//   2. the 8 windows [lo + j, lo + j + n), j < 8, of a thread share the core [lo + 7, lo + n): summed ONCE from the tree (at most
//      7 samples, 7 runs and 7 blocks at either end plus the 512-sample blocks between: <= 78 terms at the largest window);
//      window j adds the j samples behind the core and the 7 - j before it (suffix and prefix sums of 7 samples each).
//   So the error of a window sum is at most (terms) 2^-53 of the sum itself -- nothing cancels -- and a window of zeros sums to 0.
//   Windows shorter than 8 are summed sample by sample.
// The recursive form is a scan over the pairs (a, b) of y -> a y + b in float64: 8 samples per thread, Hillis-Steele inside the
// wave with the powers a^(8 o) from the host, the four waves and the carry from the tile before folded in order.  All terms
// are non-negative.  The ratio is ONE float64 division rounded once to float32 (bound against the float64 restatement: 2^-24
// plus float64 noise; the tests allow 4 x 2^-24).  Every multiply-add is an explicit fma and contraction is off, so that the
// instantiations agree bit for bit.
//
// Bytes: x is read once from HBM and r written once (8 B per sample; the fused form 4 B).  The halo of a tile -- the samples the
// same workgroup staged for the tile before -- is read again from L2; samples before the block come from `prev` (n_prev of them,
// the tail the caller kept), unknown ones are zeros and yield r = 0.
#include "d4w_internal.h"

#ifndef D4W_EMU
#pragma clang fp contract(off)
#endif

namespace d4w {
namespace {

constexpr int kSlThreads = 256, kSlRun = 8, kSlTile = kSlThreads * kSlRun;         // 2048 samples per tile
constexpr int kSlMaxWindow = 16384;                                                 // nlta + gap (and nsta) at most
constexpr int kSlMaxEv = kSlTile / 2 + 2;                                           // events that touch one tile, at most
constexpr int kSlWaves = kSlThreads / 64;
enum { SL_CLASSIC = 0, SL_RECURSIVE = 1, SL_LOAD = 2 };

struct SlArgs {
    const float* x;            // [nx][ld]: the samples (SL_CLASSIC, SL_RECURSIVE) or the ratio that is read (SL_LOAD)
    const float* prev;         // [nx][ld_prev] or NULL: the n_prev samples before the block (their last is sample -1)
    const float* scale;        // [nx] A
    const double* rin;         // [nx][2] (sta, lta) before the block, or NULL: zeros
    double* rout;              // [nx][2] or NULL
    float* ratio;              // [nx][ld_r] (WR)
    const double* thr_on;      // [nx] (TRG)
    const double* thr_off;
    const int* act_in;         // [nx] or NULL: the flag on entry
    int* act_out;              // [nx] or NULL
    int* ev;                   // [nx][cap][3]: on, off, peak index
    float* evpeak;             // [nx][cap]
    int* counts;               // [nx]
    size_t ld, ld_prev, ld_r;
    long long nseen;           // samples before the block (SL_RECURSIVE)
    int nx, ns, n_prev, cap;
    int nsta, nlta, gap, halo; // halo = max(nsta, nlta + gap) - 1
    int nr8;                   // runs staged per tile, at most
    int off_keys, off_misc, off_xs;     // byte offsets into the dynamic LDS
    double inv_sta, inv_lta, floor;
    double a[2], a512[2];      // 1 - 1 / n and its 512th power (one wave's samples)
    double pl[2][64];          // a^(8 l)
};

__device__ __forceinline__ int sl_at(int q) { return q + (q >> 3); }               // sample q of the stage, one pad word per run

__device__ __forceinline__ double sl_sq(const float* xs, int q) {
    const double v = (double)xs[sl_at(q)];
    return v * v;
}

// sum of e over the staged samples [lo, hi): whole runs, blocks of 8 runs and of 64 runs wherever they lie inside
__device__ __forceinline__ double sl_range(const float* xs, const double* rs8, const double* rs64, const double* rs512, int lo, int hi) {
    double s = 0.0;
    while (lo < hi && (lo & 7)) s += sl_sq(xs, lo++);
    while (lo < hi && (hi & 7)) s += sl_sq(xs, --hi);
    lo >>= 3; hi >>= 3;
    while (lo < hi && (lo & 7)) s += rs8[lo++];
    while (lo < hi && (hi & 7)) s += rs8[--hi];
    lo >>= 3; hi >>= 3;
    while (lo < hi && (lo & 7)) s += rs64[lo++];
    while (lo < hi && (hi & 7)) s += rs64[--hi];
    lo >>= 3; hi >>= 3;
    for (; lo < hi; ++lo) s += rs512[lo];
    return s;
}

// S[j] = sum of e over [lo + j, lo + j + n), j < nj <= 8 (the samples up to lo + n + nj - 2 are staged)
__device__ __forceinline__ void sl_windows(const float* xs, const double* rs8, const double* rs64, const double* rs512, int lo, int n,
                                           int nj, double (&S)[kSlRun]) {
    if (n < kSlRun) {
#pragma unroll
        for (int j = 0; j < kSlRun; ++j) {
            double s = 0.0;
            if (j < nj)
                for (int k = 0; k < n; ++k) s += sl_sq(xs, lo + j + k);
            S[j] = s;
        }
        return;
    }
    const double core = sl_range(xs, rs8, rs64, rs512, lo + kSlRun - 1, lo + n);
    double head[kSlRun], tail[kSlRun];                       // head[j] = e[lo + j .. lo + 6],  tail[j] = e[lo + n .. lo + n + j - 1]
    head[kSlRun - 1] = 0.0;
#pragma unroll
    for (int j = kSlRun - 2; j >= 0; --j) head[j] = head[j + 1] + sl_sq(xs, lo + j);
    tail[0] = 0.0;
#pragma unroll
    for (int j = 1; j < kSlRun; ++j) tail[j] = (j < nj) ? tail[j - 1] + sl_sq(xs, lo + n + j - 1) : 0.0;
#pragma unroll
    for (int j = 0; j < kSlRun; ++j) S[j] = (core + head[j]) + tail[j];
}

// (value, position) as one unsigned key: the larger value wins, on ties the smaller position; never 0 for a real pair
__device__ __forceinline__ unsigned long long sl_key(float v, int pos) {
    unsigned u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)pos);
}
__device__ __forceinline__ void sl_unkey(unsigned long long k, float* v, int* pos) {
    unsigned u = (unsigned)(k >> 32);
    u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    *v = __uint_as_float(u);
    *pos = (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull));
}

template <int SRC, bool WR, bool TRG>
__global__ __launch_bounds__(kSlThreads) void stalta_rows(SlArgs P) {
    D4W_DYN_LDS(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x, ns = P.ns;
    double* rs8 = reinterpret_cast<double*>(smem);
    double* rs64 = rs8 + P.nr8;
    double* rs512 = rs64 + (P.nr8 / 8 + 1);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem + P.off_keys);
    double* wB = reinterpret_cast<double*>(smem + P.off_misc);                   // [2][kSlWaves] wave totals of the scan
    int* wsum = reinterpret_cast<int*>(wB + 2 * kSlWaves);                          // [kSlWaves] last operation of every wave
    int* wcnt = wsum + kSlWaves;                                                    // [kSlWaves] event starts of every wave
    float* xs = reinterpret_cast<float*>(smem + P.off_xs);

    const float* xr = P.x + (size_t)row * P.ld;
    const int halo = P.halo;
    float A = 0.f;
    double bar = 0.0;
    if constexpr (SRC != SL_LOAD) {
        A = P.scale[row];
        const double fa = P.floor * (double)A;
        bar = fa * fa;
    }
    const bool live = A > 0.f;                                                      // (a NaN scale: zeros as well)
    double carry[2] = {0.0, 0.0};                                                   // the recurrences' state before the tile
    if constexpr (SRC == SL_RECURSIVE) {
        if (P.rin) { carry[0] = P.rin[2 * (size_t)row]; carry[1] = P.rin[2 * (size_t)row + 1]; }
    }
    // the trigger's state before the tile, alike in every thread
    int t_state = 0, t_nev = 0;
    unsigned long long t_key = 0ull;
    double thr_on = 0.0, thr_off = 0.0;
    int* evr = nullptr;
    float* pkr = nullptr;
    if constexpr (TRG) {
        thr_on = P.thr_on[row]; thr_off = P.thr_off[row];
        evr = P.ev + (size_t)row * P.cap * 3;
        pkr = P.evpeak + (size_t)row * P.cap;
        if (P.act_in && P.act_in[row] != 0) {
            t_state = 1; t_nev = 1; t_key = sl_key(-INFINITY, 0);
            if (tid == 0) evr[0] = -1;
        }
    }

    for (int t0 = 0; t0 < ns; t0 += kSlTile) {
        const int nout = min(kSlTile, ns - t0);
        const int k0 = kSlRun * tid;
        const int nj = max(0, min(kSlRun, nout - k0));                              // this thread's samples inside the row
        float c[kSlRun];
#pragma unroll
        for (int j = 0; j < kSlRun; ++j) c[j] = 0.f;

        if constexpr (TRG) {
            for (int e = tid; e < kSlMaxEv; e += kSlThreads) keys[e] = (e == 0 && t_state) ? t_key : 0ull;
        }

        if constexpr (SRC == SL_CLASSIC) {
            // ---- stage samples t0 - halo .. t0 + nout - 1 (stage index q = sample - gbase), zeros to the end of the last run
            const int gbase = t0 - halo, nstage = halo + nout;
            const int nrun = (nstage + kSlRun - 1) / kSlRun;
            const float* pv = P.prev ? P.prev + (size_t)row * P.ld_prev + P.n_prev : nullptr;     // pv[g], g < 0
            for (int q = tid; q < -gbase && q < nstage; q += kSlThreads) {
                const int g = gbase + q;
                xs[sl_at(q)] = (pv && g >= -P.n_prev) ? pv[g] : 0.f;
            }
            for (int q = nstage + tid; q < nrun * kSlRun; q += kSlThreads) xs[sl_at(q)] = 0.f;
            const int glo = max(0, gbase), ghi = t0 + nout;
            const int e0 = (int)((reinterpret_cast<uintptr_t>(xr) >> 2) & 3);       // xr + g is 16-byte aligned iff 4 | g + e0
            for (int k = ((glo + e0) >> 2) + tid; 4 * k - e0 < ghi; k += kSlThreads) {
                const int g = 4 * k - e0;
                if (g >= glo && g + 4 <= ghi) {
                    const float4 v = *reinterpret_cast<const float4*>(xr + g);
                    const int q = g - gbase;
                    xs[sl_at(q)] = v.x; xs[sl_at(q + 1)] = v.y; xs[sl_at(q + 2)] = v.z; xs[sl_at(q + 3)] = v.w;
                } else {
                    for (int u = 0; u < 4; ++u)
                        if (g + u >= glo && g + u < ghi) xs[sl_at(g + u - gbase)] = xr[g + u];
                }
            }
            __syncthreads();
            // ---- sums of squares of every run
            for (int r = tid; r < nrun; r += kSlThreads) {
                const float* p = xs + r * (kSlRun + 1);
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < kSlRun; ++j) {
                    const double v = (double)p[j];
                    s = fma(v, v, s);
                }
                rs8[r] = s;
            }
            __syncthreads();
            // ---- of every 8 runs and every 64 runs that are complete
            const int n64 = nrun >> 3, n512 = nrun >> 6;
            for (int b = tid; b < n64 + n512; b += kSlThreads) {
                const bool big = b >= n64;
                const int first = big ? (b - n64) * 64 : b * 8, cnt = big ? 64 : 8;
                double s = 0.0;
                for (int j = 0; j < cnt; ++j) s += rs8[first + j];
                if (big) rs512[b - n64] = s; else rs64[b] = s;
            }
            __syncthreads();
            // ---- the thread's 8 ratios
            if (nj > 0) {
                const int q0 = halo + k0;                                           // stage index of the thread's first sample
                double Ss[kSlRun], Sl[kSlRun];
                sl_windows(xs, rs8, rs64, rs512, q0 - P.nsta + 1, P.nsta, nj, Ss);
                sl_windows(xs, rs8, rs64, rs512, q0 - P.gap - P.nlta + 1, P.nlta, nj, Sl);
#pragma unroll
                for (int j = 0; j < kSlRun; ++j) {
                    const double sta = Ss[j] * P.inv_sta, lta = Sl[j] * P.inv_lta;
                    const bool known = t0 + k0 + j - halo >= -P.n_prev;
                    if (j < nj && live && known && lta > bar) c[j] = (float)(sta / lta);
                }
            }
            __syncthreads();                                                        // the stage is filled again for the next tile
        } else if constexpr (SRC == SL_RECURSIVE) {
            double e[kSlRun];
            {
                const float* p = xr + t0 + k0;
                if (nj == kSlRun && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
                    const float4 u = *reinterpret_cast<const float4*>(p), w = *reinterpret_cast<const float4*>(p + 4);
                    const float v[kSlRun] = {u.x, u.y, u.z, u.w, w.x, w.y, w.z, w.w};
#pragma unroll
                    for (int j = 0; j < kSlRun; ++j) e[j] = (double)v[j] * (double)v[j];
                } else {
#pragma unroll
                    for (int j = 0; j < kSlRun; ++j) {
                        const double v = (j < nj) ? (double)p[j] : 0.0;
                        e[j] = v * v;
                    }
                }
            }
            double before[2];                                                       // the state before the thread's first sample
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                const double a = P.a[f], inv = f ? P.inv_lta : P.inv_sta;
                double B = 0.0;                                                     // the thread's 8 samples from a zero state
#pragma unroll
                for (int j = 0; j < kSlRun; ++j) B = fma(a, B, e[j] * inv);
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {                                  // inclusive scan of the wave's threads
                    const double up = __shfl_up(B, o);
                    if (lane >= o) B = fma(P.pl[f][o], up, B);
                }
                const double excl = __shfl_up(B, 1);
                if (lane == 63) wB[f * kSlWaves + wave] = B;
                before[f] = (lane > 0) ? excl : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                double cin = carry[f], end = carry[f];
                for (int w = 0; w < kSlWaves; ++w) {
                    end = fma(P.a512[f], end, wB[f * kSlWaves + w]);
                    if (w + 1 == wave) cin = end;
                }
                carry[f] = end;                                                     // (of a full tile; a cut one is the row's last)
                before[f] = fma(P.pl[f][lane], cin, before[f]);
            }
            double s0 = before[0], s1 = before[1];
#pragma unroll
            for (int j = 0; j < kSlRun; ++j) {
                s0 = fma(P.a[0], s0, e[j] * P.inv_sta);
                s1 = fma(P.a[1], s1, e[j] * P.inv_lta);
                const long long i = (long long)t0 + k0 + j;
                if (j < nj && live && P.nseen + i + 1 >= (long long)P.nlta && s1 > bar) c[j] = (float)(s0 / s1);
                if (P.rout && i == (long long)ns - 1) { P.rout[2 * (size_t)row] = s0; P.rout[2 * (size_t)row + 1] = s1; }
            }
            __syncthreads();                                                        // wB is written again in the next tile
        } else {
            const float* p = xr + t0 + k0;
            if (nj == kSlRun && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
                const float4 u = *reinterpret_cast<const float4*>(p), w = *reinterpret_cast<const float4*>(p + 4);
                c[0] = u.x; c[1] = u.y; c[2] = u.z; c[3] = u.w; c[4] = w.x; c[5] = w.y; c[6] = w.z; c[7] = w.w;
            } else {
#pragma unroll
                for (int j = 0; j < kSlRun; ++j)
                    if (j < nj) c[j] = p[j];
            }
        }

        if constexpr (WR) {
            float* yp = P.ratio + (size_t)row * P.ld_r + t0 + k0;
            if (nj == kSlRun && (reinterpret_cast<uintptr_t>(yp) & 15) == 0) {
                *reinterpret_cast<float4*>(yp) = make_float4(c[0], c[1], c[2], c[3]);
                *reinterpret_cast<float4*>(yp + 4) = make_float4(c[4], c[5], c[6], c[7]);
            } else {
#pragma unroll
                for (int j = 0; j < kSlRun; ++j)
                    if (j < nj) yp[j] = c[j];
            }
        }

        if constexpr (TRG) {
            // ---- the flag before every thread: the last ON / OFF before it, else the flag before the tile
            int last = 0;                                                           // 0 none, 1 ON, 2 OFF
#pragma unroll
            for (int j = 0; j < kSlRun; ++j) {
                const double v = (double)c[j];
                if (j < nj) last = (v > thr_on) ? 1 : (v < thr_off) ? 2 : last;
            }
            const unsigned long long bh = __ballot(last != 0), bo = __ballot(last == 1);
            if (lane == 0) wsum[wave] = bh ? (((bo >> (63 - __builtin_clzll(bh))) & 1ull) ? 1 : 2) : 0;
            __syncthreads();
            int st = t_state, fin = t_state;
            for (int w = 0; w < kSlWaves; ++w) {
                if (wsum[w]) fin = wsum[w] == 1;
                if (w + 1 == wave) st = fin;
            }
            const unsigned long long below = bh & ((1ull << lane) - 1ull);
            if (below) st = (int)((bo >> (63 - __builtin_clzll(below))) & 1ull);
            // ---- the events that start in the thread's samples, numbered along the tile
            int nstart = 0;
            {
                int s = st;
#pragma unroll
                for (int j = 0; j < kSlRun; ++j) {
                    const double v = (double)c[j];
                    if (j < nj) {
                        const int s2 = (v > thr_on) ? 1 : (v < thr_off) ? 0 : s;
                        nstart += (!s && s2);
                        s = s2;
                    }
                }
            }
            int incl = nstart;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(incl, o);
                if (lane >= o) incl += up;
            }
            if (lane == 63) wcnt[wave] = incl;
            __syncthreads();
            int prior = 0, total = 0;
            for (int w = 0; w < kSlWaves; ++w) {
                if (w < wave) prior += wcnt[w];
                total += wcnt[w];
            }
            // local number of an event: the one open on entry is 0, the starts follow; in the row it is gbase + local
            const int gbase = t_nev - t_state;
            int lid = prior + incl - nstart - 1 + t_state;
            {
                int s = st;
                unsigned long long best = 0ull;
#pragma unroll
                for (int j = 0; j < kSlRun; ++j) {
                    if (j < nj) {
                        const float vf = c[j];
                        const double v = (double)vf;
                        const int pos = t0 + k0 + j;
                        const int s2 = (v > thr_on) ? 1 : (v < thr_off) ? 0 : s;
                        if (!s && s2) {
                            ++lid;
                            if (gbase + lid < P.cap) evr[3 * (size_t)(gbase + lid)] = pos;
                            best = sl_key(-INFINITY, pos);
                        }
                        if (s2 && vf == vf) {
                            const unsigned long long k = sl_key(vf, pos);
                            best = k > best ? k : best;
                        }
                        if (s && !s2) {
                            if (best) atomicMax(keys + lid, best);
                            best = 0ull;
                            if (gbase + lid < P.cap) evr[3 * (size_t)(gbase + lid) + 1] = pos;
                        }
                        s = s2;
                    }
                }
                if (s && best) atomicMax(keys + lid, best);
            }
            __syncthreads();
            const int nloc = total + t_state, nclosed = fin ? nloc - 1 : nloc;
            for (int e = tid; e < nclosed; e += kSlThreads) {
                if (gbase + e < P.cap) {
                    float v; int pos;
                    sl_unkey(keys[e], &v, &pos);
                    evr[3 * (size_t)(gbase + e) + 2] = pos;
                    pkr[gbase + e] = v;
                }
            }
            t_key = fin ? keys[nloc - 1] : 0ull;
            t_nev += total;
            t_state = fin;
            __syncthreads();                                                        // keys are cleared for the next tile
        }
    }

    if constexpr (TRG) {
        if (tid == 0) {
            if (t_state && t_nev - 1 < P.cap) {                                     // still open at the end of the block
                float v; int pos;
                sl_unkey(t_key, &v, &pos);
                evr[3 * (size_t)(t_nev - 1) + 1] = ns;
                evr[3 * (size_t)(t_nev - 1) + 2] = pos;
                pkr[t_nev - 1] = v;
            }
            P.counts[row] = t_nev;
            if (P.act_out) P.act_out[row] = t_state;
        }
    }
}

// the events of all rows as one table out[4][total] (channel, on, off, peak index) and their peaks: row c's events go to
// columns [off[c] - cnt[c], off[c])
__global__ __launch_bounds__(kSlThreads) void pack_events(const int* __restrict__ ev, const float* __restrict__ peak,
                                                           const int* __restrict__ cnt, const long long* __restrict__ off, int nx,
                                                           int cap, long long total, long long* __restrict__ out,
                                                           float* __restrict__ pk) {
    for (int c = blockIdx.x; c < nx; c += gridDim.x) {
        const int n = min(cnt[c], cap);
        const long long base = off[c] - cnt[c];
        for (int j = threadIdx.x; j < n; j += kSlThreads) {
            const int* e = ev + ((size_t)c * cap + j) * 3;
            out[base + j] = c;
            out[total + base + j] = e[0];
            out[2 * total + base + j] = e[1];
            out[3 * total + base + j] = e[2];
            pk[base + j] = peak[(size_t)c * cap + j];
        }
    }
}

template <int SRC, bool WR, bool TRG>
int sl_launch(const SlArgs& P, size_t lds, void* stream) {
    auto kern = stalta_rows<SRC, WR, TRG>;
    if (lds > 64 * 1024) D4W_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    D4W_LAUNCH(kern, dim3((unsigned)P.nx), dim3(kSlThreads), lds, stream, P);
    return D4W_OK;
}

// the LDS layout of one launch: run sums (classic), event keys (trigger), the waves' exchange words, the stage (classic)
size_t sl_layout(SlArgs& P, bool classic, bool trig) {
    size_t at = 0;
    P.nr8 = classic ? ceil_div(P.halo + std::min(P.ns, kSlTile), kSlRun) : 0;
    if (classic) at += sizeof(double) * ((size_t)P.nr8 + (P.nr8 / 8 + 1) + (P.nr8 / 64 + 1));
    P.off_keys = (int)at;
    if (trig) at += sizeof(unsigned long long) * kSlMaxEv;
    P.off_misc = (int)at;
    at += sizeof(double) * 2 * kSlWaves + sizeof(int) * 2 * kSlWaves;
    P.off_xs = (int)at;
    if (classic) at += sizeof(float) * (size_t)P.nr8 * (kSlRun + 1);
    return at;
}

int sl_check_trigger(const double* thr_on, const double* thr_off, int32_t* ev, float* peak, int32_t* counts, int cap) {
    if (!thr_on || !thr_off || !ev || !peak || !counts) return fail(D4W_EINVAL, "events need thr_on, thr_off, ev, peak and counts");
    if (cap < 1) return fail(D4W_EINVAL, "cap = %d (at least one event slot per row)", cap);
    return D4W_OK;
}

}  // namespace
}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_stalta_max_window(void) { return kSlMaxWindow; }

int d4w_stalta_tile(void) { return kSlTile; }

int d4w_stalta_f32(const float* x, size_t ld, int nx, int ns, const float* prev, size_t ld_prev, int n_prev, int form, int nsta,
                   int nlta, int gap, double floor, const float* scale, const double* rstate_in, double* rstate_out,
                   long long nseen, float* ratio, size_t ld_r, const double* thr_on, const double* thr_off,
                   const int32_t* active_in, int32_t* active_out, int32_t* ev, float* peak, int32_t* counts, int cap,
                   void* stream) {
    if (!x || !scale || nx < 1 || ns < 1 || ld < (size_t)ns) return fail(D4W_EINVAL, "bad argument (x and scale are needed; nx, ns >= 1; ld >= ns)");
    if (form != SL_CLASSIC && form != SL_RECURSIVE) return fail(D4W_EINVAL, "form = %d (0: classic, 1: recursive)", form);
    if (nsta < 1 || nlta < 1) return fail(D4W_EINVAL, "nsta = %d, nlta = %d (both at least 1)", nsta, nlta);
    if (gap < 0) return fail(D4W_EINVAL, "gap = %d (>= 0)", gap);
    if (form == SL_RECURSIVE && gap != 0) return fail(D4W_EINVAL, "the recursive form takes gap = 0 (got %d)", gap);
    if ((long long)nlta + gap > kSlMaxWindow || nsta > kSlMaxWindow)
        return fail(D4W_EINVAL, "nlta + gap = %lld and nsta = %d must not exceed %d samples", (long long)nlta + gap, nsta, kSlMaxWindow);
    if (!(floor >= 0.0) || !std::isfinite(floor)) return fail(D4W_EINVAL, "floor must be finite and >= 0");
    if (n_prev < 0 || (n_prev > 0 && (!prev || ld_prev < (size_t)n_prev))) return fail(D4W_EINVAL, "a tail needs prev and 0 <= n_prev <= ld_prev");
    if (form == SL_RECURSIVE && nseen < 0) return fail(D4W_EINVAL, "nseen = %lld (>= 0)", nseen);
    const bool trig = thr_on || thr_off || ev || peak || counts;
    if (!ratio && !trig) return fail(D4W_EINVAL, "nothing to write: neither a ratio nor events are asked for");
    if (ratio && ld_r < (size_t)ns) return fail(D4W_EINVAL, "ld_r < ns");
    if (trig) {
        const int rc = sl_check_trigger(thr_on, thr_off, ev, peak, counts, cap);
        if (rc) return rc;
    }
    SlArgs P;
    memset(&P, 0, sizeof(P));
    P.x = x; P.ld = ld; P.prev = (form == SL_CLASSIC && n_prev > 0) ? prev : nullptr; P.ld_prev = ld_prev;
    P.n_prev = P.prev ? n_prev : 0;
    P.scale = scale; P.rin = rstate_in; P.rout = rstate_out; P.nseen = nseen; P.ratio = ratio; P.ld_r = ld_r;
    P.thr_on = thr_on; P.thr_off = thr_off; P.act_in = active_in; P.act_out = active_out;
    P.ev = ev; P.evpeak = peak; P.counts = counts; P.cap = cap;
    P.nx = nx; P.ns = ns; P.nsta = nsta; P.nlta = nlta; P.gap = gap;
    P.halo = std::max(nsta, nlta + gap) - 1;
    P.inv_sta = 1.0 / nsta; P.inv_lta = 1.0 / nlta; P.floor = floor;
    for (int f = 0; f < 2; ++f) {
        const double a = 1.0 - (f ? P.inv_lta : P.inv_sta);
        P.a[f] = a;
        P.pl[f][0] = 1.0;
        const double a8 = ((a * a) * (a * a)) * ((a * a) * (a * a));
        for (int l = 1; l < 64; ++l) P.pl[f][l] = P.pl[f][l - 1] * a8;
        P.a512[f] = P.pl[f][32] * P.pl[f][32];
    }
    const bool classic = form == SL_CLASSIC;
    const size_t lds = sl_layout(P, classic, trig);
    if (classic) {
        if (ratio && trig) return sl_launch<SL_CLASSIC, true, true>(P, lds, stream);
        return ratio ? sl_launch<SL_CLASSIC, true, false>(P, lds, stream) : sl_launch<SL_CLASSIC, false, true>(P, lds, stream);
    }
    if (ratio && trig) return sl_launch<SL_RECURSIVE, true, true>(P, lds, stream);
    return ratio ? sl_launch<SL_RECURSIVE, true, false>(P, lds, stream) : sl_launch<SL_RECURSIVE, false, true>(P, lds, stream);
}

int d4w_trigger_onset_f32(const float* r, size_t ld, int nx, int ns, const double* thr_on, const double* thr_off,
                          const int32_t* active_in, int32_t* active_out, int32_t* ev, float* peak, int32_t* counts, int cap,
                          void* stream) {
    if (!r || nx < 1 || ns < 1 || ld < (size_t)ns) return fail(D4W_EINVAL, "bad argument (r is needed; nx, ns >= 1; ld >= ns)");
    const int rc = sl_check_trigger(thr_on, thr_off, ev, peak, counts, cap);
    if (rc) return rc;
    SlArgs P;
    memset(&P, 0, sizeof(P));
    P.x = r; P.ld = ld; P.thr_on = thr_on; P.thr_off = thr_off; P.act_in = active_in; P.act_out = active_out;
    P.ev = ev; P.evpeak = peak; P.counts = counts; P.cap = cap; P.nx = nx; P.ns = ns;
    const size_t lds = sl_layout(P, false, true);
    return sl_launch<SL_LOAD, false, true>(P, lds, stream);
}

int d4w_pack_events_i64(const int32_t* ev, const float* peak, const int32_t* counts, const int64_t* offsets, int nx, int cap,
                        int64_t total, int64_t* out, float* peak_out, void* stream) {
    if (!ev || !peak || !counts || !offsets || nx < 1 || cap < 1 || total < 0) return fail(D4W_EINVAL, "bad argument");
    if (total == 0) return D4W_OK;
    if (!out || !peak_out) return fail(D4W_EINVAL, "bad argument");
    D4W_LAUNCH(pack_events, dim3(std::min(nx, 4096)), dim3(kSlThreads), 0, stream, (const int*)ev, peak, (const int*)counts,
               (const long long*)offsets, nx, cap, (long long)total, (long long*)out, peak_out);
    return D4W_OK;
}

}  // extern "C"
