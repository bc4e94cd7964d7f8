// Peak picking on MI355X (gfx950): scipy.signal.find_peaks(x, prominence=thr) per row (reference detect.py:192,217,271)
// and the packed 2 x K pick table of detect.convert_pick_times (detect.py:277-303).  HBM-streaming work with the walks
// in LDS; no MFMA.
#include "row_fft.h"      // kSpThreads, kSpLdsMax, allow_lds, with_flag

namespace d4w {

// ---------------------------------------------------------------------------------------------
// scipy.signal.find_peaks(x, prominence=thr)[0] per row  (detect.py:192,217,271)
//   _local_maxima_1d: a plateau whose left neighbour is lower and whose right neighbour is lower is
//   a peak at the plateau's middle sample (floor); the first and last sample never are.
//   _peak_prominences (wlen=None): walk left / right from the peak while samples are <= the peak,
//   tracking the minimum; prominence = peak - max(left_min, right_min); keep prominence >= thr.
// One workgroup per row; a thread owns a candidate left edge, accepted peaks are written in time
// order through a workgroup prefix sum.  idx[row][0..min(count, cap)) ; counts[row] = count.
// ---------------------------------------------------------------------------------------------
// Prominence walks use a two-level (max, min) summary of the whole row held in LDS (blocks of 2^b
// samples and super-blocks of 32 blocks): a walk steps sample by sample only to the edge of its block,
// block by block to the edge of its super-block, then over super-blocks while their maximum does not
// exceed the peak, and descends into the one block that stops it -- a few dozen dependent LDS reads
// instead of O(row) dependent loads (a smooth envelope of 120 000 samples has walks of thousands of
// samples, and in SIMT the longest walk of a wave is what every lane pays).  Rows of up to kFpRowLds
// samples are staged in LDS once (the sample steps are LDS reads); longer rows are read in place
// (L2-resident after the summary sweep).  Candidates are processed without barriers (a thread strides
// the row and marks its accepted peaks in an LDS bitmap); the time-ordered index list is produced at
// the end by a popcount prefix sum over the bitmap.
constexpr int kFpMaxBlocks = 4096;
constexpr int kFpRowLds = 16384;
constexpr int kFpThreads = 512;                // two 70-KB rows fit a CU: 16 waves instead of 8
constexpr int kFpFan = 32;                      // blocks per super-block (the walk code shifts by 5)
static_assert(kFpFan == 32, "fp_walk shifts by 5");

// min over the walk from q in direction DIR until the first sample > v (exclusive) or the row end.
// Every phase reads a BATCH of operands with independent loads before it looks at them: a walk is a
// chain of dependent decisions, and one LDS round trip per step is what it would otherwise cost.
constexpr int kFpBatch = 8;        // samples / summary entries read per dependent LDS round trip of a walk
constexpr int kFpBlkBatch = 4;

// Only the decision prominence >= thr is needed, not the prominence itself: a side is SATISFIED as soon
// as the running minimum reaches lim = the largest float <= v - thr, and the walk may stop there
// (the minimum can only decrease further).  Prominent peaks therefore walk only to their first deep
// dip and small ones to the next higher sample -- nobody walks across the row.
// scan `n` samples from q in direction DIR: 1 = a sample > v stopped it, 2 = satisfied, 0 = ran out
template <int DIR>
__device__ __forceinline__ int fp_scan_samples(const float* __restrict__ r, int ns, int& q, int n, float v, float lim,
                                               float& lmin) {
    for (int done = 0; done < n; done += kFpBatch) {
        float u[kFpBatch];
#pragma unroll
        for (int k = 0; k < kFpBatch; ++k) u[k] = r[min(max(q + DIR * k, 0), ns - 1)];   // clamped: speculative tail
        const int m = min(kFpBatch, n - done);
#pragma unroll
        for (int k = 0; k < kFpBatch; ++k) {
            if (k < m) {
                if (u[k] > v) { q += DIR * k; return 1; }
                lmin = fminf(lmin, u[k]);
                if (lmin <= lim) return 2;
            }
        }
        q += DIR * m;
    }
    return 0;
}

// scan `n` summary entries (stride `step` samples each) from q: 1 = an entry's max > v stopped it (q at
// that entry), 2 = satisfied, 0 = ran out
template <int DIR>
__device__ __forceinline__ int fp_scan_blocks(const float2* __restrict__ sm, int nent, int shift, int& q, int n,
                                              int step, float v, float lim, float& lmin) {
    for (int done = 0; done < n; done += kFpBlkBatch) {
        float2 e[kFpBlkBatch];
#pragma unroll
        for (int k = 0; k < kFpBlkBatch; ++k) e[k] = sm[min(max((q + DIR * k * step) >> shift, 0), nent - 1)];
        const int m = min(kFpBlkBatch, n - done);
#pragma unroll
        for (int k = 0; k < kFpBlkBatch; ++k) {
            if (k < m) {
                if (e[k].x > v) { q += DIR * k * step; return 1; }
                lmin = fminf(lmin, e[k].y);
                if (lmin <= lim) return 2;
            }
        }
        q += DIR * m * step;
    }
    return 0;
}

// running minimum of the walk from q in direction DIR up to the first sample > v, the row end, or the
// point where it reaches lim (whichever comes first)
template <int DIR>
__device__ __forceinline__ float fp_walk(const float* __restrict__ r, const float2* __restrict__ s1,
                                         const float2* __restrict__ s2, int ns, int nb, int nb2, int bshift, int q,
                                         float v, float lim) {
    const int BS = 1 << bshift, SB = BS * kFpFan;
    float lmin = v;
    // samples to the edge of the block (for DIR < 0 the block's first sample is included)
    int n = (DIR < 0) ? ((q + 1) & (BS - 1)) : ((BS - (q & (BS - 1))) & (BS - 1));
    if (DIR > 0) n = min(n, ns - q);
    if (fp_scan_samples<DIR>(r, ns, q, n, v, lim, lmin)) return lmin;
    if ((DIR < 0) ? (q < 0) : (q >= ns)) return lmin;
    // blocks to the edge of the super-block
    const int blk = q >> bshift;
    n = (DIR < 0) ? ((blk + 1) & (kFpFan - 1)) : ((kFpFan - (blk & (kFpFan - 1))) & (kFpFan - 1));
    if (DIR > 0) n = min(n, nb - blk);
    int st = fp_scan_blocks<DIR>(s1, nb, bshift, q, n, BS, v, lim, lmin);
    if (st == 2) return lmin;
    if (st == 0) {
        if ((DIR < 0) ? (q < 0) : (q >= ns)) return lmin;
        // super-blocks to the row end
        const int sb = q >> (bshift + 5);
        n = (DIR < 0) ? sb + 1 : nb2 - sb;
        if (fp_scan_blocks<DIR>(s2, nb2, bshift + 5, q, n, SB, v, lim, lmin) != 1) return lmin;
        // blocks of the stopping super-block (one of them has a larger sample)
        if (fp_scan_blocks<DIR>(s1, nb, bshift, q, kFpFan, BS, v, lim, lmin) == 2) return lmin;
    }
    // samples of the stopping block
    (void)fp_scan_samples<DIR>(r, ns, q, BS, v, lim, lmin);
    return lmin;
}

// The same decision taken by a whole WAVE for one side of one candidate: lane l looks at entry l of the phase (sample,
// block summary or super-block summary), two ballots give the first entry that stops the walk (max > v) and the first one
// that satisfies it (min <= lim), and the earlier of the two decides -- one LDS round trip and ~30 instructions per phase
// where the lane-per-side walk takes a round trip and ~150 instructions per 4-8 entries.  A row whose candidates are few
// (an envelope with thr a fraction of its strongest peak: ~10 per row) leaves 60 of 64 lanes idle in fp_walk and still
// pays its issue slots in every wave of the workgroup: 23 of 78 thousand cycles per row at 11020 x 12000
// (scripts/probe/fp_timing.py); fp_scan runs this form when the sides are few.  Returns whether the running minimum
// reaches lim before a sample > v or the row end (fp_walk(...) <= lim); q, v, lim are wave-uniform.
// W lanes per side (W = 16: four sides per wave advance together; sides in different phases diverge and reconverge
// after every phase): gl = lane within the group, gs = the group's first lane.
template <int W>
__device__ __forceinline__ int fp_group_phase(const float hi, const float lo, bool in, float v, float lim, int gs, int& first) {
    constexpr unsigned long long kMask = (W == 64) ? ~0ull : ((1ull << (W & 63)) - 1ull);
    const unsigned long long h = (__ballot(in && hi > v) >> gs) & kMask, sfy = (__ballot(in && lo <= lim) >> gs) & kMask;
    const int fh = h ? __builtin_ctzll(h) : 64, fs = sfy ? __builtin_ctzll(sfy) : 64;
    first = fh;
    return fs < fh ? 2 : (h ? 1 : 0);
}

template <int W>
__device__ __forceinline__ bool fp_walk_wave(const float* __restrict__ r, const float2* __restrict__ s1,
                                             const float2* __restrict__ s2, int ns, int nb, int nb2, int bshift, int DIR,
                                             int q, float v, float lim, int lane) {
    const int BS = 1 << bshift, SB = BS * kFpFan;
    const int gl = lane & (W - 1), gs = lane & ~(W - 1);
    if (v <= lim) return true;                                // thr <= 0: the peak itself is its base
    auto samples = [&](int n) -> int {                        // 2 satisfied, 1 stopped (q at the stopper), 0 ran out (q past them)
        for (int done = 0; done < n; done += W) {
            const int j = q + DIR * gl, m = min(W, n - done);
            const bool in = gl < m && j >= 0 && j < ns;
            const float u = r[min(max(j, 0), ns - 1)];
            int first;
            const int st = fp_group_phase<W>(u, u, in, v, lim, gs, first);
            if (st == 2) return 2;
            if (st == 1) { q += DIR * first; return 1; }
            q += DIR * m;
        }
        return 0;
    };
    auto blocks = [&](const float2* sm, int nent, int shift, int n, int step) -> int {
        for (int done = 0; done < n; done += W) {
            const int e = (q + DIR * gl * step) >> shift, m = min(W, n - done);
            const bool in = gl < m && e >= 0 && e < nent;
            const float2 sv = sm[min(max(e, 0), nent - 1)];
            int first;
            const int st = fp_group_phase<W>(sv.x, sv.y, in, v, lim, gs, first);
            if (st == 2) return 2;
            if (st == 1) { q += DIR * first * step; return 1; }
            q += DIR * m * step;
        }
        return 0;
    };
    // the phases of fp_walk, entry for entry
    int n = (DIR < 0) ? ((q + 1) & (BS - 1)) : ((BS - (q & (BS - 1))) & (BS - 1));
    if (DIR > 0) n = min(n, ns - q);
    int st = samples(n);
    if (st) return st == 2;
    if ((DIR < 0) ? (q < 0) : (q >= ns)) return false;
    const int blk = q >> bshift;
    n = (DIR < 0) ? ((blk + 1) & (kFpFan - 1)) : ((kFpFan - (blk & (kFpFan - 1))) & (kFpFan - 1));
    if (DIR > 0) n = min(n, nb - blk);
    st = blocks(s1, nb, bshift, n, BS);
    if (st == 2) return true;
    if (st == 0) {
        if ((DIR < 0) ? (q < 0) : (q >= ns)) return false;
        const int sb = q >> (bshift + 5);
        n = (DIR < 0) ? sb + 1 : nb2 - sb;
        st = blocks(s2, nb2, bshift + 5, n, SB);
        if (st != 1) return st == 2;                                        // satisfied, or the row end without a base
        if (blocks(s1, nb, bshift, kFpFan, BS) == 2) return true;         // blocks of the stopping super-block
    }
    return samples(BS) == 2;
}

// LDS tables of the picker for one row (after `lead` bytes the caller uses itself)
struct FpLds {
    float2* s1;        // [nb]  (max, min) of every block
    float2* s2;        // [nb2] (max, min) of every super-block
    unsigned* bits;    // [nwords] accepted peaks
    unsigned* cand;    // [nwords] rising edges of the maxima worth a walk
    int* clist;        // [kFpList] their positions, one round of bitmap words at a time
    float* rowl;       // [ns] the row (STAGED)
};

__device__ __forceinline__ void fp_summaries2(const FpLds& T, int nb, int nb2, int tid) {
    // one block summary per lane, 32-lane shuffle reduction (kFpFan = 32 = half a wave)
    for (int base = 0; base < nb; base += kFpThreads) {                  // wave-uniform trip count: every lane shuffles
        const int k = base + tid;
        float mx = -INFINITY, mn = INFINITY;
        if (k < nb) {
            const float2 e = T.s1[k];
            mx = e.x;
            mn = e.y;
        }
#pragma unroll
        for (int off = 1; off < kFpFan; off <<= 1) {
            mx = fmaxf(mx, __shfl_xor(mx, off));
            mn = fminf(mn, __shfl_xor(mn, off));
        }
        if ((k & (kFpFan - 1)) == 0 && k < nb) T.s2[k / kFpFan] = make_float2(mx, mn);
    }
    (void)nb2;
}

// block summaries of a row held in `r` (LDS or global): eight blocks per wave iteration (their loads are independent
// and in flight together), lanes stride a block, wave shuffle reduction
__device__ __forceinline__ void fp_summaries1(const float* __restrict__ r, const FpLds& T, int ns, int nb, int bshift, int tid) {
    const int BS = 1 << bshift, lane = tid & 63, wave = tid >> 6;
    constexpr int kBatch = 8;
    for (int bk0 = wave * kBatch; bk0 < nb; bk0 += (kFpThreads / 64) * kBatch) {
        float mx[kBatch], mn[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            mx[j] = -INFINITY;
            mn[j] = INFINITY;
            const int lo = (bk0 + j) << bshift, hi = min(lo + BS, ns);
            for (int i = lo + lane; i < hi; i += 64) {
                const float u = r[i];
                mx[j] = fmaxf(mx[j], u);
                mn[j] = fminf(mn[j], u);
            }
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                mx[j] = fmaxf(mx[j], __shfl_xor(mx[j], off));
                mn[j] = fminf(mn[j], __shfl_xor(mn[j], off));
            }
            if (lane == 0 && bk0 + j < nb) T.s1[bk0 + j] = make_float2(mx[j], mn[j]);
        }
    }
}

// stage the row into LDS and form the 32-sample block summaries in the same sweep: a lane loads four consecutive
// samples (16 bytes), eight neighbouring lanes cover one block and reduce with three shuffle steps
template <bool STORE>     // STORE: keep the row in T.rowl (rows that fit); otherwise only the summaries are formed
__device__ __forceinline__ void fp_stage_rows4(const float* __restrict__ rg, const FpLds& T, int ns, int nb, int tid) {
    const int ns4 = ns >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(rg);
    float4* l4 = reinterpret_cast<float4*>(T.rowl);
    constexpr int kAhead = 12;                                          // loads in flight per lane: the sweep is latency-bound
    for (int base = 0; base < 8 * nb; base += kAhead * kFpThreads) {    // wave-uniform trip count: every lane shuffles
        float4 q[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            const int v4 = base + k * kFpThreads + tid;
            q[k] = (v4 < ns4) ? g4[v4] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            const int v4 = base + k * kFpThreads + tid;
            float mx = -INFINITY, mn = INFINITY;
            if (v4 < ns4) {
                if (STORE) l4[v4] = q[k];
                mx = fmaxf(fmaxf(q[k].x, q[k].y), fmaxf(q[k].z, q[k].w));
                mn = fminf(fminf(q[k].x, q[k].y), fminf(q[k].z, q[k].w));
            }
#pragma unroll
            for (int off = 1; off <= 4; off <<= 1) {
                mx = fmaxf(mx, __shfl_xor(mx, off));
                mn = fminf(mn, __shfl_xor(mn, off));
            }
            if ((v4 & 7) == 0 && (v4 >> 3) < nb) T.s1[v4 >> 3] = make_float2(mx, mn);
        }
    }
}

// Rows too long for LDS, after the summary sweep: the maxima that can reach the threshold at all (v - thr not below the
// row minimum) are looked for in a second sweep that passes the row through LDS in windows of kFpSegW samples (a core of
// kFpSegS plus kFpSegH either side, in the space the candidate list occupies later; the next windows are already in
// registers while this one is worked on).  A window with a handful of such maxima (an envelope with thr a fraction of its
// strongest peak) just marks them in T.cand for the summary walks of fp_scan.  A window full of them (a raw correlogram
// has a maximum every ~9 samples, 14 000 per 120 000-sample row, and its minimum is as deep as its maximum is high) is
// settled on the spot: the window is COMPACTED to its turning points E (samples not below both or not above both
// neighbours -- the minimum of any stretch and the first sample above any level survive the compaction, so a walk over E
// decides exactly what a walk over the samples decides), the maxima of the core are listed, and lane t takes side t & 1 of
// maximum t >> 1 and walks E: two entries per oscillation instead of its ~9 samples, both sides of a maximum at once, one
// maximum per lane, LDS reads only; almost all are settled within two or three periods.  Accepted peaks go to T.bits
// directly; a maximum whose walk leaves the window or runs past kFpSegSteps entries, a plateau, and every maximum of a
// window with more turning points than the lists hold is marked in T.cand.  Samples outside the row read as +inf: a walk
// stops there, as at the row end.
constexpr int kFpSegH = 64;
constexpr int kFpSegW = 2048;
constexpr int kFpSegS = kFpSegW - 2 * kFpSegH;          // 1920 samples
constexpr int kFpSegE = 1024;                           // turning points held per window
constexpr int kFpSegC = 512;                            // maxima held per window
constexpr int kFpSegSteps = 8;                          // entries of E a side may walk
constexpr int kFpSegFew = 24;                           // lanes with a maximum up to which a window is not worth compacting
constexpr int kFpSegMax = (kFpMaxBlocks * 32 + kFpSegS - 1) / kFpSegS;   // windows of the longest row with 32-sample blocks
static_assert(kFpSegS % 32 == 0, "a window core is whole summary blocks");
static_assert(kFpSegW == 4 * kFpThreads && kFpSegH % 4 == 0, "window geometry: one 16-byte load per lane");

// one side of maximum v over the turning points: 2 = the running minimum reached lim before a higher entry, 1 = a higher
// entry (or the row end) came first, 0 = not decided inside the window
template <int DIR>
__device__ __forceinline__ int fp_turning_side(const float* __restrict__ E, int nE, int idx, float v, float lim) {
    float lmin = INFINITY;
    for (int done = 0; done < kFpSegSteps; done += 4) {
        float e[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = E[min(max(idx + DIR * k, 0), nE - 1)];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = idx + DIR * k;
            if (j < 0 || j >= nE) return 0;
            if (e[k] > v) return 1;
            lmin = fminf(lmin, e[k]);
            if (lmin <= lim) return 2;
        }
        idx += DIR * 4;
    }
    return 0;
}

// Returns the row position from which the maxima have NOT been looked at: the first two windows with something in them
// decide for the row -- when both hold only a handful of maxima the rest is left to the barrier-free marking sweep of fp_scan.
__device__ __forceinline__ int fp_sweep_segments(const float* __restrict__ rg, const FpLds& T, int ns, int nb, double thr,
                                                 float gmin, int* wave_tot, unsigned char* hot, int tid) {
    float* seg = reinterpret_cast<float*>(T.clist);
    float4* l4 = reinterpret_cast<float4*>(T.clist);
    float* E = seg + kFpSegW;                                              // [kFpSegE]
    unsigned* C = reinterpret_cast<unsigned*>(E + kFpSegE);               // [kFpSegC]  window position | plateau << 15 | index in E << 16
    unsigned char* res = reinterpret_cast<unsigned char*>(C + kFpSegC);   // [2 kFpSegC]
    int* seg_tot = reinterpret_cast<int*>(res + 2 * kFpSegC);             // [kFpThreads / 64]
    const float4* g4 = reinterpret_cast<const float4*>(rg);
    const int ns4 = ns >> 2, lane = tid & 63, wave = tid >> 6;
    const int nseg = (ns + kFpSegS - 1) / kFpSegS;
    const float4 inf4 = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
    // windows whose core holds no sample that could reach the threshold are neither loaded nor looked at
    for (int k = tid; k < kFpSegMax; k += kFpThreads) hot[k] = 0;
    __syncthreads();
    for (int bk = tid; bk < nb; bk += kFpThreads)
        if (!((double)T.s1[bk].x - thr < (double)gmin)) hot[bk / (kFpSegS / 32)] = 1;
    __syncthreads();
    auto fetch = [&](int s) -> float4 {
        const int v4 = (s * kFpSegS - kFpSegH) / 4 + tid;
        return (s < nseg && hot[s] && v4 >= 0 && v4 < ns4) ? g4[v4] : inf4;
    };
    float4 r0 = fetch(0), r1 = fetch(1), r2 = fetch(2);        // three windows in flight per lane
    int few = 0, full = 0, resume = ns;
    for (int s = 0; s < nseg; ++s) {
        const int w0 = s * kFpSegS - kFpSegH;                  // row position of the window's first sample
        const float4 cur = r0;
        r0 = r1;
        r1 = r2;
        r2 = fetch(s + 3);
        if (!hot[s]) continue;
        const int c = 4 * tid, i0 = w0 + c;
        const bool core = tid >= kFpSegH / 4 && tid < (kFpSegH + kFpSegS) / 4;
        l4[tid] = cur;
        __syncthreads();
        // maxima worth a walk among the lane's four samples
        const float u[6] = {c ? seg[c - 1] : INFINITY, cur.x, cur.y, cur.z, cur.w, (c + 4 < kFpSegW) ? seg[c + 4] : INFINITY};
        unsigned m = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + k;
            const float v = u[k + 1];
            if (core && i >= 1 && i < ns - 1 && u[k] < v && !(u[k + 2] > v) && !((double)v - thr < (double)gmin)) m |= 1u << k;
        }
        const unsigned long long busy = __ballot(m != 0u);
        if (lane == 0) wave_tot[wave] = __popcll(busy);
        __syncthreads();
        int nbusy = 0;
        for (int k = 0; k < kFpThreads / 64; ++k) nbusy += wave_tot[k];
        if (nbusy <= kFpSegFew) {                                // (uniform) nothing to gain from the lists
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((m >> k) & 1u) atomicOr(&T.cand[(i0 + k) >> 5], 1u << ((i0 + k) & 31));
            if (++few == 2 && !full) {
                resume = (s + 1) * kFpSegS;
                break;
            }
            continue;                                            // (the window and wave_tot are next written behind a barrier each)
        }
        ++full;
        unsigned em = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + k;
            const float v = u[k + 1];
            const bool hi = v >= u[k] && v >= u[k + 2], lo = v <= u[k] && v <= u[k + 2];
            if (hi || lo || i == 0 || i == ns - 1) em |= 1u << k;
        }
        const int mine = __popc(em) | (__popc(m) << 16);
        int incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int n = __shfl_up(incl, off);
            if (lane >= off) incl += n;
        }
        if (lane == 63) seg_tot[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < kFpThreads / 64; ++k) {
            if (k < wave) before += seg_tot[k];
            total += seg_tot[k];
        }
        const int nE = total & 0xFFFF, nC = total >> 16;
        const bool listed = nE <= kFpSegE && nC <= kFpSegC;
        if (listed) {
            int pe = (before + incl - mine) & 0xFFFF, pc = (before + incl - mine) >> 16;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if ((em >> k) & 1u) {
                    if ((m >> k) & 1u) C[pc++] = (unsigned)(c + k) | ((unsigned)pe << 16) | ((u[k + 2] == u[k + 1]) ? 0x8000u : 0u);
                    E[pe++] = u[k + 1];
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((m >> k) & 1u) atomicOr(&T.cand[(i0 + k) >> 5], 1u << ((i0 + k) & 31));
        }
        __syncthreads();
        if (listed) {
            for (int t = tid; t < 2 * nC; t += kFpThreads) {
                const unsigned cd = C[t >> 1];
                const int e = (int)(cd >> 16);
                int r = 0;
                if (!(cd & 0x8000u)) {                               // plateaus are left to fp_scan
                    const float v = E[e];
                    const double dl = (double)v - thr;               // as in fp_scan: lim = the largest float u with v - u >= thr
                    float lim = (float)dl;
                    if ((double)lim > dl) lim = nextafterf(lim, -INFINITY);
                    r = (t & 1) ? fp_turning_side<+1>(E, nE, e + 1, v, lim) : fp_turning_side<-1>(E, nE, e - 1, v, lim);
                }
                res[t] = (unsigned char)r;
            }
        }
        __syncthreads();
        if (listed) {
            for (int q = tid; q < nC; q += kFpThreads) {
                const int a = res[2 * q], b = res[2 * q + 1];
                if (a == 1 || b == 1) continue;                      // a higher sample before a deep enough base: not prominent
                const int i = w0 + (int)(C[q] & 0x7FFFu);
                if (a == 2 && b == 2) atomicOr(&T.bits[i >> 5], 1u << (i & 31));
                else atomicOr(&T.cand[i >> 5], 1u << (i & 31));
            }
        }
        // no barrier here: the window, the counts and the lists are each next written behind a later barrier than their last read
    }
    __syncthreads();
    return min(resume, ns);
}

// candidates -> accepted-peak bitmap, in two phases so that the prominence walks run with every lane busy:
//   (1) every thread marks the rising edges of maxima that can reach the threshold at all in the `cand` bitmap -- no
//       base can lie below the row minimum, so a maximum with v - thr below it is rejected here, without a walk (with
//       thr = a fraction of the strongest peak that is almost every maximum);
//   (2) per round of kFpThreads bitmap words the marked positions are listed (popcount prefix sum) and lane c walks
//       candidate c.  Walking inside the marking loop instead made a wave pay the SUM of its lanes' walks (one lane
//       walking, 63 masked): 0.72 of 0.97 ms at 11020 x 12000 with ~15 picks per row.
// r: the row (LDS or global).  Ends with the accepted peaks in T.bits; the last barrier is the caller's.
#ifdef D4W_FP_TIMING      // probe builds only (scripts/probe/fp_timing.py): cycles of workgroup 0's thread 0 between phase marks
__device__ unsigned long long g_fp_t[16];
#define FP_MARK(k) do { if (threadIdx.x == 0) { const unsigned long long t_ = clock64(); atomicAdd(&g_fp_t[k], t_ - fp_t0); fp_t0 = t_; } } while (0)
#define FP_T0 unsigned long long fp_t0 = clock64()
#else
#define FP_MARK(k) do {} while (0)
#define FP_T0 do {} while (0)
#endif

constexpr int kFpList = 4096;          // candidates per walk round
constexpr int kFpWaveSides = 256;      // up to this many walk sides per round a group of lanes takes a side (fp_walk_wave)
#ifndef D4W_FP_GROUP
#define D4W_FP_GROUP 16
#endif
constexpr int kFpGroup = D4W_FP_GROUP; // lanes per side
static_assert(kFpSegW + kFpSegE + kFpSegC + kFpSegC / 2 + kFpThreads / 64 <= kFpList, "the window and its lists live in the candidate list");

__device__ __forceinline__ void fp_scan(const float* __restrict__ r, const FpLds& T, int ns, int nb, int nb2, int bshift,
                                        double thr, int nwords, int* wave_tot, unsigned* cfail, bool vec4, int mark_from,
                                        int tid) {
    // mark_from: first sample whose maxima are still to be marked (0: the whole row; > 0: fp_sweep_segments has dealt with
    // the samples before it -- a multiple of 4 -- and left in T.cand only the maxima it could not settle inside their window)
    const int lane = tid & 63, wave = tid >> 6;
    FP_T0;
    float gmin = INFINITY;
    for (int k = 0; k < nb2; ++k) gmin = fminf(gmin, T.s2[k].y);
    int* ccount = wave_tot + kFpThreads / 64;                 // (zeroed by the kernel before its first barrier)
    // 32-sample blocks, the whole row still to mark: a block whose maximum cannot reach the threshold (almost all of them
    // when thr is a fraction of the strongest peak) costs one summary read; the others are looked at by half a wave each, a
    // lane per sample, their bitmap word is stored whole (no zeroing pass, no atomics) and their candidates go straight
    // into the list -- the sample-by-sample marking sweep of the whole row was 8 of 28 thousand cycles of this function at
    // 11020 x 12000 (scripts/probe/fp_timing.py), the separate counting pass 2.5.  (A lane per hot block, 32 samples
    // each, cost the same 8: every wave with one hot lane pays the whole scan.)
    bool by_block = vec4 && bshift == 5 && mark_from == 0;
    if (by_block) {
        // the threshold test in float32: vcut = the smallest float v with !((double)v - thr < (double)gmin) (the test is
        // monotone in v: float -> double is exact, the float64 subtraction rounds monotonically)
        float vcut = (float)((double)gmin + thr);
        for (int k = 0; k < 4 && (double)vcut - thr < (double)gmin; ++k) vcut = nextafterf(vcut, INFINITY);
        for (int k = 0; k < 4; ++k) {
            const float below = nextafterf(vcut, -INFINITY);
            if ((double)below - thr < (double)gmin || below == vcut) break;
            vcut = below;
        }
        const bool vcut_ok = !((double)vcut - thr < (double)gmin) && ((double)nextafterf(vcut, -INFINITY) - thr < (double)gmin);
        // (1) the blocks worth a look, listed from the END of the candidate list (a row whose candidates and hot blocks
        // together exceed the list takes the round-by-round path below, which lists from the bitmap again)
        int* hcount = ccount + 1;
        for (int bk = tid; bk < nwords; bk += kFpThreads) {                     // nwords == nb
            if (!((double)T.s1[bk].x - thr < (double)gmin)) T.clist[kFpList - 1 - atomicAdd(hcount, 1)] = bk;
            else T.cand[bk] = 0u;
        }
        __syncthreads();
        // (2) half a wave per hot block, a lane per sample: one ballot gives the block's bitmap word
        // (a row where a quarter of the blocks are hot -- thr small against the row's range -- is cheaper in the sweep of
        // all samples below: 0.36 against 0.48 ms at thr = 0)
        const int nhot = *hcount, l = lane & 31;
        if (4 * nhot > nb) by_block = false;
        for (int h0 = 0; by_block && h0 < nhot; h0 += kFpThreads / 32) {      // wave-uniform trip count
            const int h = h0 + (tid >> 5);
            const int bk = T.clist[kFpList - 1 - min(h, nhot - 1)];
            const int i = (bk << 5) + l;
            const bool in = h < nhot && i >= 1 && i < ns - 1;
            const float v = r[min(i, ns - 1)], a = r[max(i - 1, 0)], b = r[min(i + 1, ns - 1)];
            const bool pk = in && a < v && !(b > v) && (vcut_ok ? v >= vcut : !((double)v - thr < (double)gmin));
            unsigned m = (unsigned)(__ballot(pk) >> (lane & 32));
            if (l == 0 && h < nhot) {
                T.cand[bk] = m;
                if (m) {
                    const int cnt = __popc(m);
                    int p = atomicAdd(ccount, cnt);
                    if (p + cnt + nhot <= kFpList) {      // always: by_block has at most nb / 4 <= 128 hot blocks of at most 16 maxima each (no input reaches the else)
                        while (m) {
                            const int bit = __builtin_ctz(m);
                            m &= m - 1u;
                            T.clist[p++] = (bk << 5) + bit;
                        }
                    }
                }
            }
        }
    }
    if (!by_block && mark_from == 0) {
        for (int w = tid; w < nwords; w += kFpThreads) T.cand[w] = 0u;
        __syncthreads();
    }
    if (by_block) {
    } else if (vec4) {
        // four samples per lane: one 16-byte read and the two neighbours instead of three reads per sample; four such
        // groups in flight per lane (rows too long for LDS are read from global memory here)
        const float4* r4 = reinterpret_cast<const float4*>(r);
        constexpr int kAhead = 4;
        const int ns4 = ns >> 2;
        for (int g0 = tid + (mark_from >> 2); g0 < ns4; g0 += kAhead * kFpThreads) {
            float4 q[kAhead];
            float lo[kAhead], hi[kAhead];
#pragma unroll
            for (int j = 0; j < kAhead; ++j) {
                const int v4 = g0 + j * kFpThreads, i0 = 4 * v4;
                const bool in = v4 < ns4;
                q[j] = in ? r4[v4] : make_float4(0.f, 0.f, 0.f, 0.f);
                lo[j] = (in && i0) ? r[i0 - 1] : INFINITY;
                hi[j] = (in && i0 + 4 < ns) ? r[i0 + 4] : INFINITY;
            }
#pragma unroll
            for (int j = 0; j < kAhead; ++j) {
                const int v4 = g0 + j * kFpThreads, i0 = 4 * v4;
                if (v4 >= ns4) continue;
                const float u[6] = {lo[j], q[j].x, q[j].y, q[j].z, q[j].w, hi[j]};
                unsigned m = 0u;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float v = u[k + 1];
                    const int i = i0 + k;
                    if (i >= 1 && i < ns - 1 && u[k] < v && !(u[k + 2] > v) && !((double)v - thr < (double)gmin)) m |= 1u << k;
                }
                if (m) atomicOr(&T.cand[i0 >> 5], m << (i0 & 31));
            }
        }
    } else {
        for (int i = max(1, mark_from) + tid; i < ns - 1; i += kFpThreads) {
            const float v = r[i];
            if (r[i - 1] < v && !(r[i + 1] > v) && !((double)v - thr < (double)gmin)) atomicOr(&T.cand[i >> 5], 1u << (i & 31));
        }
    }
    __syncthreads();
    FP_MARK(4);                                               // marking sweep
    // walks + acceptance of the `total` candidates listed in T.clist (any order: accepted peaks go to a bitmap)
    auto walk_listed = [&](int total) {
        FP_MARK(5);                                           // counting + listing
        for (int w2 = tid; w2 < kFpList / 32; w2 += kFpThreads) cfail[w2] = 0u;
        __syncthreads();
        FP_MARK(6);
        // the left and the right walk of a candidate run on two lanes (a walk is a chain of dependent LDS reads: with
        // ~20 candidates per row most lanes idle anyway); a direction whose base is too high marks the candidate failed
        // ... dealt round-robin to the waves: a wave pays the longest of its lanes' walks in every phase of fp_walk
        if (2 * total <= kFpWaveSides) {
            // few sides: kFpGroup lanes per side (fp_walk_wave), everything uniform within a group
            constexpr int kPerWave = 64 / kFpGroup;
            for (int c2 = wave * kPerWave + lane / kFpGroup; c2 < 2 * total; c2 += (kFpThreads / 64) * kPerWave) {
                const int c = c2 >> 1;
                const int i = T.clist[c];
                const float v = r[i];
                int ia = i + 1;
                while (ia < ns - 1 && r[ia] == v) ++ia;
                bool ok = r[ia] < v && !((double)v - thr < (double)gmin);
                if (ok) {
                    const double dl = (double)v - thr;
                    float lim = (float)dl;
                    if ((double)lim > dl) lim = nextafterf(lim, -INFINITY);
                    ok = fp_walk_wave<kFpGroup>(r, T.s1, T.s2, ns, nb, nb2, bshift, (c2 & 1) ? 1 : -1, (c2 & 1) ? ia : i - 1, v, lim,
                                                lane);
                }
                if (!ok && (lane & (kFpGroup - 1)) == 0) atomicOr(&cfail[c >> 5], 1u << (c & 31));
            }
        } else
        for (int c2 = (tid & 63) * (kFpThreads / 64) + (tid >> 6); c2 < 2 * total; c2 += kFpThreads) {
            const int c = c2 >> 1;
            const int i = T.clist[c];
            const float v = r[i];
            int ia = i + 1;
            while (ia < ns - 1 && r[ia] == v) ++ia;                  // plateau: reported at its middle sample
            bool ok = r[ia] < v && !((double)v - thr < (double)gmin);     // (the second test: maxima fp_sweep_segments passed on)
            if (ok) {
                // float64 like scipy (float32 samples are exact in float64, a float32 subtraction is not):
                // lim = the largest float u with (double)v - (double)u >= thr
                const double dl = (double)v - thr;
                float lim = (float)dl;
                if ((double)lim > dl) lim = nextafterf(lim, -INFINITY);
                // (<= lim, not !(> lim): lim is NaN for a +inf sample under a +inf bar, and fp_walk_wave's ballots reject that side)
                if (c2 & 1) ok = fp_walk<+1>(r, T.s1, T.s2, ns, nb, nb2, bshift, ia, v, lim) <= lim;
                else ok = fp_walk<-1>(r, T.s1, T.s2, ns, nb, nb2, bshift, i - 1, v, lim) <= lim;    // else: left base too high
            }
            if (!ok) atomicOr(&cfail[c >> 5], 1u << (c & 31));
        }
        FP_MARK(7);                                           // thread 0's own walk
        __syncthreads();
        FP_MARK(8);                                           // ... and the wait for the longest one
        for (int c = tid; c < total; c += kFpThreads) {
            if ((cfail[c >> 5] >> (c & 31)) & 1u) continue;
            const int i = T.clist[c];
            const float v = r[i];
            int ia = i + 1;
            while (ia < ns - 1 && r[ia] == v) ++ia;
            const int mid = (i + ia - 1) / 2;
            atomicOr(&T.bits[mid >> 5], 1u << (mid & 31));
        }
        __syncthreads();
        FP_MARK(9);                                           // acceptance
    };
    // all candidates of the row in ONE list when they fit (the usual case: a walk phase costs its longest walk, however
    // few lanes walk), else one round of kFpList / 16 bitmap words at a time
    int total_all = 0;
    if (by_block) {
        total_all = *ccount;                                  // listed already when they fit ...
        if (total_all + ccount[1] > kFpList) total_all = kFpList + 1;        // ... beside the hot-block list
    } else {
        int mine = 0;
        for (int w = tid; w < nwords; w += kFpThreads) mine += __popc(T.cand[w]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off);
        if (lane == 0) wave_tot[wave] = mine;
        if (tid == 0) *ccount = 0;
        __syncthreads();
        for (int k = 0; k < kFpThreads / 64; ++k) total_all += wave_tot[k];
        if (total_all <= kFpList) {
            for (int w = tid; w < nwords; w += kFpThreads) {
                unsigned word = T.cand[w];
                if (!word) continue;
                int p = atomicAdd(ccount, __popc(word));
                while (word) {
                    const int bit = __builtin_ctz(word);
                    word &= word - 1u;
                    T.clist[p++] = (w << 5) + bit;
                }
            }
        }
    }
    if (total_all <= kFpList) {
        walk_listed(total_all);
        return;
    }
    __syncthreads();                                          // wave_tot is reused below
    constexpr int kWordsPerRound = kFpList / 16;              // a word marks at most 16 maxima
    for (int w0 = 0; w0 < nwords; w0 += kWordsPerRound) {
        const int w = w0 + tid;
        unsigned word = (tid < kWordsPerRound && w < nwords) ? T.cand[w] : 0u;
        const int cnt = __popc(word);
        int incl = cnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int n = __shfl_up(incl, off);
            if (lane >= off) incl += n;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < kFpThreads / 64; ++k) {
            if (k < wave) before += wave_tot[k];
            total += wave_tot[k];
        }
        int p = before + incl - cnt;
        while (word) {
            const int bit = __builtin_ctz(word);
            word &= word - 1u;
            T.clist[p++] = (w << 5) + bit;
        }
        walk_listed(total);
    }
}

// time-ordered index list: popcount prefix sum over the bitmap, kFpThreads words per round
__device__ __forceinline__ void fp_emit(const FpLds& T, int nwords, int* __restrict__ orow, int* __restrict__ count, int cap,
                                        int* wave_tot, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int w0 = 0; w0 < nwords; w0 += kFpThreads) {
        const int w = w0 + tid;
        unsigned word = (w < nwords) ? T.bits[w] : 0u;
        const int cnt = __popc(word);
        int incl = cnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int n = __shfl_up(incl, off);
            if (lane >= off) incl += n;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < kFpThreads / 64; ++k) {
            if (k < wave) before += wave_tot[k];
            total += wave_tot[k];
        }
        int p = base + before + incl - cnt;
        while (word) {
            const int bit = __builtin_ctz(word);
            word &= word - 1u;
            if (p < cap) orow[p] = (w << 5) + bit;
            ++p;
        }
        base += total;
        __syncthreads();
    }
    if (tid == 0) *count = base;
}

__device__ __forceinline__ FpLds fp_lds(unsigned char* p, int nb, int nb2, int nwords) {
    FpLds T;
    T.s1 = reinterpret_cast<float2*>(p);
    T.s2 = T.s1 + nb;
    const int nw4 = (nwords + 3) & ~3;
    T.bits = reinterpret_cast<unsigned*>(T.s1 + ((nb + nb2 + 1) & ~1));   // every table starts on 16 bytes:
    T.cand = T.bits + nw4;                                                // the row is staged with 16-byte accesses
    T.clist = reinterpret_cast<int*>(T.cand + nw4);
    T.rowl = reinterpret_cast<float*>(T.clist + kFpList);
    return T;
}

template <bool STAGED>
__global__ __launch_bounds__(kFpThreads) void find_peaks_prom(const float* __restrict__ x, int ns, double thr0,
                                                              int bshift, int* __restrict__ idx,
                                                              int* __restrict__ counts, int cap,
                                                              const float* __restrict__ thr_dev, int thr_rows) {
    // thr_dev: the threshold is thr0 x a DEVICE value (d4w_find_peaks_dthr_f32: "0.45 of the largest correlation" without the
    // host waiting for that maximum), formed in float64 like the host's 0.45 * float(c.max())
    // thr_rows: one value per row (d4w_find_peaks_rowthr_f32: "k times this channel's noise floor")
    const double thr = thr_dev ? thr0 * (double)thr_dev[thr_rows ? blockIdx.x : 0] : thr0;
    if (!(thr == thr)) {                                       // a NaN bar, through any entry point: no prominence is >= NaN (SciPy returns no peak)
        if (threadIdx.x == 0) counts[blockIdx.x] = 0;
        return;
    }
    D4W_DYN_LDS(smem_raw);
    __shared__ int wave_tot[kFpThreads / 64 + 2];              // + the candidate and hot-block counters of fp_scan
    __shared__ unsigned cfail[kFpList / 32];
    __shared__ unsigned char hot[kFpSegMax];                   // fp_sweep_segments: windows worth loading
    const int BS = 1 << bshift, nb = (ns + BS - 1) >> bshift, nb2 = (nb + kFpFan - 1) / kFpFan;
    const int nwords = (ns + 31) >> 5;
    const FpLds T = fp_lds(smem_raw, nb, nb2, nwords);
    const float* rg = x + (size_t)blockIdx.x * ns;
    const int tid = threadIdx.x;
    FP_T0;
    if (tid == 0) wave_tot[kFpThreads / 64] = wave_tot[kFpThreads / 64 + 1] = 0;     // fp_scan's candidate / hot-block counters
    for (int w = tid; w < nwords; w += kFpThreads) T.bits[w] = 0u;
    const bool al16 = (ns & 3) == 0 && ((reinterpret_cast<size_t>(rg) & 15) == 0);
    const bool vec4 = bshift == 5 && al16;
    const bool sweep = !STAGED && vec4;
    if (vec4) {
        fp_stage_rows4<STAGED>(rg, T, ns, nb, tid);
    } else {
        if (STAGED) {
            for (int i = tid; i < ns; i += kFpThreads) T.rowl[i] = rg[i];
            __syncthreads();
        }
        fp_summaries1(STAGED ? T.rowl : rg, T, ns, nb, bshift, tid);
    }
    __syncthreads();
    FP_MARK(0);                                               // staged + block summaries
    fp_summaries2(T, nb, nb2, tid);
    if (sweep)
        for (int w = tid; w < nwords; w += kFpThreads) T.cand[w] = 0u;
    __syncthreads();
    FP_MARK(1);
    {
        // A peak's prominence is its height less the higher of two minima of the row: never more than (row maximum - row minimum).
        // A row that cannot reach the threshold -- most channels of a file carry no call above 0.45 of the file's largest
        // correlation -- is done here: no candidates, no walks, no bitmap scan.  (Exact: the difference is formed in float64 like the walks', and the
        // test is false for a row holding a NaN, which then takes the full path; a NaN bar has left above.)
        float gmax = -INFINITY, gmin2 = INFINITY;
        for (int k = 0; k < nb2; ++k) { const float2 e = T.s2[k]; gmax = fmaxf(gmax, e.x); gmin2 = fminf(gmin2, e.y); }
        if ((double)gmax - (double)gmin2 < thr) {
            if (tid == 0) counts[blockIdx.x] = 0;
            return;
        }
    }
    int mark_from = 0;
    if (sweep) {
        float gmin = INFINITY;
        for (int k = 0; k < nb2; ++k) gmin = fminf(gmin, T.s2[k].y);
        mark_from = fp_sweep_segments(rg, T, ns, nb, thr, gmin, wave_tot, hot, tid);
    }
    fp_scan(STAGED ? T.rowl : rg, T, ns, nb, nb2, bshift, thr, nwords, wave_tot, cfail, STAGED ? (ns & 3) == 0 : al16,
            mark_from, tid);
    __syncthreads();
    FP_MARK(2);                                               // marking + listing + walks
    fp_emit(T, nwords, idx + (size_t)blockIdx.x * cap, counts + blockIdx.x, cap, wave_tot, tid);
    FP_MARK(3);
}

// picks of all rows as ONE packed 2 x K table (detect.convert_pick_times, detect.py:277-303: row 0 = channel,
// row 1 = time index): row c's cnt[c] indices go to columns [off[c] - cnt[c], off[c]) (off = inclusive prefix sum)
__global__ __launch_bounds__(kSpThreads) void pack_picks(const int* __restrict__ idx, const int* __restrict__ cnt,
                                                          const long long* __restrict__ off, int nx, int cap, long long total,
                                                          long long* __restrict__ out) {
    for (int c = blockIdx.x; c < nx; c += gridDim.x) {
        const int n = min(cnt[c], cap);
        const long long base = off[c] - cnt[c];
        for (int j = threadIdx.x; j < n; j += kSpThreads) {
            out[base + j] = c;
            out[total + base + j] = idx[(size_t)c * cap + j];
        }
    }
}

// Inclusive prefix sums of the per-row pick counts (what pack_picks places the rows by), their total and the largest count,
// in ONE small launch: one workgroup, a run of consecutive rows per thread.  (torch.cumsum + max + stack: a rocprim scan, two
// reductions and a concatenation per picker call before round 5.)
constexpr int kOffThreads = 1024;
__global__ __launch_bounds__(kOffThreads) void pick_offsets(const int* __restrict__ cnt, int nx, long long* __restrict__ off,
                                                            long long* __restrict__ summary) {
    __shared__ long long wsum[kOffThreads / 64];
    __shared__ int pmax[kOffThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (nx + kOffThreads - 1) / kOffThreads;
    const int a = min(tid * per, nx), b = min(a + per, nx);
    long long s = 0;
    int m = 0;
    for (int i = a; i < b; ++i) {
        const int c = cnt[i];
        s += c;
        m = max(m, c);
    }
    // inclusive scan of the threads' sums: inside a wave by shuffles, across the 16 waves through LDS (two barriers in all;
    // the Hillis-Steele form over 1024 threads took twenty)
    long long incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    for (int o = 32; o >= 1; o >>= 1) m = max(m, __shfl_xor(m, o));
    if (lane == 63) wsum[wave] = incl;
    if (lane == 0) pmax[wave] = m;
    __syncthreads();
    long long before = 0, total = 0;
    for (int w = 0; w < kOffThreads / 64; ++w) {
        if (w < wave) before += wsum[w];
        total += wsum[w];
    }
    long long run = before + incl - s;                     // exclusive prefix of this thread's rows
    for (int i = a; i < b; ++i) {
        run += cnt[i];
        off[i] = run;
    }
    if (tid == 0) {
        int mm = 0;
        for (int w = 0; w < kOffThreads / 64; ++w) mm = max(mm, pmax[w]);
        summary[0] = mm;
        summary[1] = total;
    }
}

}  // namespace d4w

using namespace d4w;

extern "C" {

static int find_peaks_launch(const float* x, int nx, int ns, double prominence, const float* thr_dev, int thr_rows, int32_t* idx,
                             int32_t* counts, int cap, void* stream) {
    if (!x || !idx || !counts || nx < 1 || ns < 1 || cap < 1) return fail(D4W_EINVAL, "bad argument");
    int bshift = 5;                                            // 32-sample blocks, larger for very long rows
    while (((ns + (1 << bshift) - 1) >> bshift) > kFpMaxBlocks) ++bshift;
    const int nb = (ns + (1 << bshift) - 1) >> bshift;
    static const int staged_env = [] { const char* v = getenv("D4W_FP_STAGED"); return v ? atoi(v) : -1; }();   // A/B switch
    const bool staged = staged_env >= 0 ? (staged_env > 0 && ns <= kFpRowLds) : (ns <= kFpRowLds);
    const int nb2 = (nb + kFpFan - 1) / kFpFan;
    const size_t lds = ((size_t)2 * ((nb + nb2 + 1) & ~1) + 2 * (size_t)((((ns + 31) >> 5) + 3) & ~3) + (size_t)kFpList +
                        (staged ? (size_t)ns : 0)) * sizeof(float);
    if (lds > kSpLdsMax) return fail(D4W_EINVAL, "rows of %d samples exceed the peak-picking LDS tables", ns);
    return with_flag(staged, [&](auto St) {
        constexpr auto kern = find_peaks_prom<decltype(St)::value>;
        allow_lds(kern, lds);
        D4W_LAUNCH(kern, dim3(nx), dim3(kFpThreads), lds, stream, x, ns, prominence, bshift, (int*)idx, (int*)counts, cap,
                   thr_dev, thr_rows);
        return (int)D4W_OK;
    });
}

int d4w_find_peaks_f32(const float* x, int nx, int ns, double prominence, int32_t* idx, int32_t* counts, int cap,
                       void* stream) {
    return find_peaks_launch(x, nx, ns, prominence, nullptr, 0, idx, counts, cap, stream);
}

int d4w_find_peaks_dthr_f32(const float* x, int nx, int ns, const float* value, double scale, int32_t* idx, int32_t* counts,
                            int cap, void* stream) {
    if (!value) return fail(D4W_EINVAL, "NULL argument");
    return find_peaks_launch(x, nx, ns, scale, value, 0, idx, counts, cap, stream);
}

int d4w_find_peaks_rowthr_f32(const float* x, int nx, int ns, const float* thr, double scale, int32_t* idx, int32_t* counts,
                              int cap, void* stream) {
    if (!thr) return fail(D4W_EINVAL, "NULL argument");
    return find_peaks_launch(x, nx, ns, scale, thr, 1, idx, counts, cap, stream);
}

#ifdef D4W_FP_TIMING
int d4w_fp_timing_read(unsigned long long* host16, int reset) {
    D4W_HIP(hipDeviceSynchronize());
    D4W_HIP(hipMemcpyFromSymbol(host16, HIP_SYMBOL(g_fp_t), sizeof(g_fp_t)));
    if (reset) {
        unsigned long long z[16] = {};
        D4W_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_fp_t), z, sizeof(z)));
    }
    return D4W_OK;
}
#endif

int d4w_pick_offsets_i64(const int32_t* counts, int nx, int64_t* offsets, int64_t* summary2, void* stream) {
    if (!counts || !offsets || !summary2 || nx < 1) return fail(D4W_EINVAL, "bad argument");
    D4W_LAUNCH(pick_offsets, dim3(1), dim3(kOffThreads), 0, stream, (const int*)counts, nx, (long long*)offsets, (long long*)summary2);
    return D4W_OK;
}

int d4w_pack_picks_i64(const int32_t* idx, const int32_t* counts, const int64_t* offsets, int nx, int cap, int64_t total,
                       int64_t* out, void* stream) {
    if (!idx || !counts || !offsets || nx < 1 || cap < 1 || total < 0) return fail(D4W_EINVAL, "bad argument");
    if (total == 0) return D4W_OK;
    if (!out) return fail(D4W_EINVAL, "bad argument");
    D4W_LAUNCH(pack_picks, dim3(std::min(nx, 4096)), dim3(kSpThreads), 0, stream, (const int*)idx, (const int*)counts,
               (const long long*)offsets, nx, cap, (long long)total, (long long*)out);
    return D4W_OK;
}

}  // extern "C"
