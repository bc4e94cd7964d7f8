// What the f-k translation units share: fk_filter.hip (single-device filter: generic pass kernels, planner, mask, apply),
// fk_dist.hip (distributed filter, fkd_*) and analytic_long.hip (analytic signal of rows too long for LDS).  The plan
// structs, the constants of the pass kernels, the host helpers that build a plan's tables, and the few functions that
// cross a unit boundary.  Every kernel is compiled in exactly one unit: another unit starts it through the host
// launchers declared at the end.
#pragma once
#include <algorithm>
#include <mutex>
#include <vector>

#include "fft_lds.h"
#include "fft_host.h"
#include "fk_entry.h"
#include "design_eval.h"

struct d4w_fkd_plan;

namespace d4w {

constexpr int kThreads = 256;      // threads of the small helper kernels
#ifndef D4W_FK_THREADS
#define D4W_FK_THREADS 512
#endif
constexpr int kMaxThreads = D4W_FK_THREADS;   // block size of the pass kernels
constexpr int kMaxTile = 8192;     // complex elements per LDS tile (64 KiB)
constexpr int kMaxTileBs = 8192;   // ... of the Bluestein pass C (16384 = 128 KiB, one workgroup per CU, measured slower: 2.36 vs 2.06 ms at 13223 x 12000)
constexpr int kPF = kMaxTile / kMaxThreads;   // prefetch registers (float2) per thread

// mask values as they are read by the fold: m, or m * a + b (dsp.fk_filt's min-max normalisation, dsp.py:945, applied to
// every value exactly as the separate pass did -- one fewer read and write of the dense mask)
struct FkAffine {
    float a, b;
    int on;
    __device__ __forceinline__ float operator()(float m) const { return on ? fmaf(m, a, b) : m; }
};

struct FkdSlab {
    int nx, nq, N2;           // slab [nx row positions][nq owned q1][N2 positions]
    const int* q1_of;         // [nq] n1-position of local column block jq
    const int* jq_partner;    // [nq] local index of the Hermitian partner q1
    const int* row_partner;   // [nx]
    const int* mirror0;       // [N2]
    const float2* wrow;       // [N1] indexed by q1
    const float2* wcol;       // [N2]
    const float* mask;        // [nx][nq][N2] folded mask of the owned sub-rows
    const float* nyq;         // [nx]
    int hilbert;              // 0: x folded mask (f-k filter); 1: x (-i sign(f)), rows self-paired (analytic signal)
};

// where a distributed plan's mask comes from: a dense shifted-grid mask, or a closed-form design
struct FkdMaskSrc {
    const float* dense = nullptr;
    DesignArgs A{};
    int mode = -1;
    FkAffine aff{1.f, 0.f, 0};           // dense only, generic plan only: a * m + b applied while folding
};

}  // namespace d4w

struct d4w_fk_plan {
    d4w::FkDev dev;
    d4w_fkd_plan* big = nullptr;           // set: every call goes through this world-1 distributed plan
    std::vector<void*> allocs;
    int* d_rowk = nullptr;
    int* d_k1 = nullptr;
    int* d_k2 = nullptr;
    float* d_mask = nullptr;
    float* d_nyq = nullptr;
    float* d_win_flat = nullptr;
    bool has_mask = false;
    bool genericA = false, genericB = false, genericC = false;
    size_t ldsA = 0, ldsB = 0, ldsC = 0;
    int threads = d4w::kMaxThreads;
    int npairs = 0;
    int num_cu = 256;
    int wg_per_cu = 2;
    const d4w::FkFastEntry* fast = nullptr;     // shape-specialised kernels, or nullptr = generic passes
    d4w::FkFastDev fdev;
    // dead-row pruning of the specialised path (set per mask)
    std::vector<int2> h_pairs;             // full pass-B work list (host copy)
    unsigned* d_rowmax = nullptr;          // [nx] bit pattern of max |M_h| per row (fk_fold_mask_tiled)
    int* d_q1_of_k1 = nullptr;             // [N1] position of time-axis digit k1
    int fold_R0 = 0, fold_IB = 0;          // tiling of fk_fold_mask_tiled (0: the gather kernel)
    double prune_eps = 0.0;                // tail pruning of the current mask (0 = exact)
    unsigned* d_livebits = nullptr;        // [C1][C2A]
    int2* d_pairs_live = nullptr;          // [npairs] compacted list
    int npairs_run = 0;                    // pairs the specialised pass B runs
    int live_rows = 0;
    int wgA = 1, wgC = 1, wgB = 1, wgBi = 1, wgBf = 1;
    int slab_sw = 0;                       // > 0: passes A/C and C'/A' run slab by slab, sw column blocks per slab
    // time-first order (fk_tf.h): chosen per mask by fk_mask_finish when it moves fewer bytes than dead-row skipping
    bool tf = false;
    d4w::FkTfDev tfdev;
    int npairsT = 0;
    unsigned* d_colkeys = nullptr;         // [2][M] min / max keys of the mask columns
    float* d_tgain = nullptr;              // [M]
    int2* d_ctab = nullptr;                // [NC][NB]
    int* d_colsrc = nullptr;               // [Lc] gather table: mask position of every column of W (-1 none, -2 Nyquist)
    float* d_cmask = nullptr;              // [nx][Lc] folded mask at the band columns
    float2* d_W = nullptr;                 // [nx][Lc] compact half spectrum (capacity cap_W elements, shared by the three)
    unsigned* d_cmlive = nullptr;          // [Cm tiles][C2A] liveness words of the band mask
    size_t cap_W = 0;
    int tf_band_cols = 0, tf_tail_cols = 0;   // per row: band (incl. Nyquist) and tail columns kept
    double bytes_cf = 42.0, bytes_tf = 42.0;  // modelled bytes per channel-sample of the two orders for the current mask
    // One plan, several host threads / streams (dsp.get_fk_plan hands the same plan to every thread filtering a shape): the
    // folded mask and its tables are rewritten by every set_mask, W of the time-first order and the exchange buffers of
    // `big` by every apply.  Every operation on the plan (set_mask*, apply*) takes the host mutex for its launch sequence,
    // makes its stream wait for the event the previous operation recorded if that ran on ANOTHER stream, and records the
    // event again at its end: a total order on the device, free when everything runs on one stream.
    std::mutex apply_mu;
    hipEvent_t apply_done = nullptr;
    hipStream_t apply_stream = nullptr;
    bool apply_used = false;
};

struct d4w_fkd_plan {
    int nx = 0, ns = 0, M = 0, world = 1, rank = 0;
    int row_begin = 0, row_end = 0;      // this rank's channel block
    int N1 = 1, N2 = 1, C1 = 1, C2 = 1, TA_t = 1, TA_c = 1, TC = 1;
    std::vector<int> owner;              // [N1] rank owning each n1-position
    std::vector<int> myq;                // owned n1-positions, ascending
    d4w_fk_plan tp, cp;                  // time-phase / channel-phase descriptors (tables owned here)
    d4w::FkdSlab slab;
    size_t lds_t = 0, lds_c1 = 0, lds_c2 = 0, lds_n2 = 0;
    bool gen_t = false, gen_n2 = false, gen_c1 = false, gen_c2 = false;
    int* d_rowk = nullptr; int* d_k1 = nullptr; int* d_k2 = nullptr; int* d_q1of = nullptr;
    float* d_mask = nullptr; float* d_nyq = nullptr;
    bool has_mask = false;
    int num_cu = 256;
    // ---- channel count with a prime factor > 31: Bluestein convolution of length bz_L in global memory (fkd_bz_*)
    int bz_L = 0, bz_W = 0;                 // transform length (0: off), columns per scratch chunk
    float2* bz_S = nullptr;                 // [bz_L][bz_W]
    const float2* bz_chirp = nullptr;       // [nx]    exp(-i pi n^2 / nx)
    const float2* bz_filt = nullptr;        // [bz_L]  FFT of the wrapped conjugate chirp / bz_L at the row positions of cp
    // the slab columns whose folded gains (or whose Hermitian partner column's) are not all zero: the only ones whose channel
    // transform matters -- a dead column leaves the pair op as zeros whatever it held, and the inverse transform of zeros is
    // zeros.  A fin-whale band of 14-30 Hz keeps a third of the columns (the band and its mirror image in the packed
    // spectrum): 19 997 x 120 000 runs 6 scratch chunks per direction instead of 18.
    int* bz_cols = nullptr;                 // [W] DEVICE, the first bz_nlive entries in use
    unsigned* bz_flags = nullptr;           // [W] DEVICE scratch of the scan (column maxima, then the live flags)
    int bz_nlive = -1;                      // -1: every column (no list)
    double prune_eps = 0.0;                 // opt-in gain level (x the largest gain) below which a column counts as dead
    std::vector<int> h_jqpart, h_mirror0;   // host copies of the pair op's column maps
    // ---- ns / 2 with a prime factor > 31: the same for the time transform of the packed rows (fkd_bt_*); the half
    //      spectrum then comes out in natural order, N1 = 1, N2 = ns / 2, while tp describes the length-bt_L transform
    int bt_L = 0, bt_R = 0;                 // transform length (0: off), rows per scratch chunk
    float2* bt_S = nullptr;                 // [bt_R][bt_L]
    const float2* bt_chirp = nullptr;       // [M]     exp(-i pi m^2 / M)
    const float2* bt_filt = nullptr;        // [bt_L]  at the positions [q1][i] of tp
    const float2* bt_win = nullptr;         // [M]     packed tukey(ns, 0.03)
    // ---- packed path: the shape has specialised kernels (fk_fast.h, FkGeo).  The exchange buffers need no repacking:
    //      the time phase writes sub-row q1 of local row l at  blk_off[owner[q1]] + l * nq[owner] * N2 + jq(q1) * N2
    //      (destination rank major), so that the all-to-all delivers the slab [nx][nq][N2] as it stands.
    d4w_fk_plan* sp = nullptr;              // tables of the single-device plan of the whole shape (no mask of its own)
    d4w::FkDev dev_t, dev_c;                     // time-phase / channel-phase argument blocks
    d4w::FkFastDev fdev_c;
    d4w::FkGeo geo_t, geo_c;
    std::vector<int2> h_pairs_slab;         // pass-B work list in slab keys r * nq + jq
    int2* d_pairs_slab = nullptr; int2* d_pairs_live = nullptr;
    int2* d_pairs_self = nullptr; int npairs_self = 0;   // pass-B work list "every row is its own Hermitian partner" (analytic signal)
    unsigned* d_livebits = nullptr; unsigned* d_rowmax = nullptr;
    int npairs_run = 0, live_rows = 0;
};

namespace d4w {

template <typename T>
inline int upload(d4w_fk_plan* pl, const std::vector<T>& h, const T** out) {
    void* p = nullptr;
    D4W_HIP(hipMalloc(&p, std::max<size_t>(h.size(), 1) * sizeof(T)));
    pl->allocs.push_back(p);
    D4W_HIP(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = (const T*)p;
    return D4W_OK;
}

inline int make_axis(d4w_fk_plan* pl, int L, AxisDesc* ax, std::vector<int>* p2f,
                     const std::vector<int>* forced = nullptr) {
    std::vector<int> rad;
    if (forced) rad = *forced;
    else if (!factor_radices(L, rad))
        return fail(D4W_EINVAL, "length %d has a prime factor > 31 and this axis has no Bluestein form (only the channel axis of the f-k filter has); dsp.supported_length(n) gives the nearest shorter supported length", L);
    ax->L = L;
    ax->nstage = (L == 1) ? 0 : (int)rad.size();
    for (int i = 0; i < kMaxStages; ++i) ax->radix[i] = (i < (int)rad.size() && L > 1) ? rad[i] : 1;
    if (L == 1) rad.clear();
    *p2f = pos_to_freq(L, rad);
    return upload(pl, twiddle_table2(L, &ax->nhi), &ax->tw2);
}

template <typename K, typename... Args>
inline int launch_k(K kern, dim3 grid, dim3 blk, size_t lds, void* stream, Args... args) {
    hipLaunchKernelGGL(kern, grid, blk, lds, (hipStream_t)stream, args...);
    D4W_HIP(hipGetLastError());
    return D4W_OK;
}

// n with every prime factor <= 31 divided out
inline int rough_part(int n) {
    for (int p = 2; p <= 31; ++p)
        while (n % p == 0) n /= p;
    return n;
}

inline int largest_divisor_le(int n, int lim) {
    int best = 1;
    for (int dd = 1; dd <= lim && dd <= n; ++dd)
        if (n % dd == 0) best = dd;
    return best;
}

// scipy.signal.windows.tukey(n, alpha), symmetric (used by dsp.taper_data, dsp.py:721)
inline std::vector<float> tukey_window(int n, double alpha) {
    std::vector<float> w(n, 1.0f);
    if (n <= 1 || alpha <= 0) return w;
    if (alpha >= 1.0) {
        for (int i = 0; i < n; ++i) w[i] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * i / (n - 1)));
        return w;
    }
    const int width = (int)floor(alpha * (n - 1) / 2.0);
    for (int i = 0; i <= width; ++i)
        w[i] = (float)(0.5 * (1.0 + cos(M_PI * (-1.0 + 2.0 * i / alpha / (n - 1)))));
    for (int i = n - width - 1; i < n; ++i)
        w[i] = (float)(0.5 * (1.0 + cos(M_PI * (-2.0 / alpha + 1.0 + 2.0 * i / alpha / (n - 1)))));
    return w;
}

// ---- fk_filter.hip
// alloc_mask = false: tables only (the distributed plan keeps its own slab mask); fast_only: D4W_EINVAL unless the
// shape has specialised kernels
int fk_plan_build(int nx, int ns, const int* opts, bool alloc_mask, bool fast_only, d4w_fk_plan** out);
void fk_plan_release(d4w_fk_plan* pl);      // frees the plan's device tables and its event (not the plan itself)
double fk_zero_gain(const FkDims& d, double prune_eps, double gmax);      // gains the filter treats as zero
// the generic pass kernels, started from any unit (generic: the loop-based radices as well as the unrolled ones)
int fk_launch_passA_fwd(bool taper, bool generic, dim3 grid, dim3 blk, size_t lds, void* stream, const FkDev& P,
                        const float2* src, float2* dst, int ntiles);
int fk_launch_passA_inv(bool generic, dim3 grid, dim3 blk, size_t lds, void* stream, const FkDev& P, float2* data, int ntiles);
int fk_launch_passC(bool inv, bool generic, dim3 grid, dim3 blk, size_t lds, void* stream, const FkDev& P, float2* data,
                    int ntiles);
void fk_pass_ac_lds_limit(int bytes);       // dynamic-LDS limit of every fk_passA_* / fk_passC instantiation

// ---- fk_dist.hip
// the distributed plan's generic form at world 1 carries the channel counts whose part with prime factors > 31 does not
// fit the LDS Bluestein tile (its channel phase is a Bluestein convolution in global memory, fkd_bz_*)
int fkd_plan_build(int nx, int ns, int world, int rank, bool want_mask, d4w_fkd_plan** out);
int fkd_plan_build_packed(int nx, int ns, int world, int rank, bool want_mask, d4w_fkd_plan** out, bool time_only = false);
int fkd_set_mask_dense_affine(d4w_fkd_plan* pl, const float* mask_shifted, float a, float b, int on, void* stream);
void fkd_set_prune(d4w_fkd_plan* pl, double prune_eps);      // the gain level the next mask's dead columns are decided by
int fkd_launch_pair_slab(const FkdSlab& S, float2* slab, void* stream);     // grid: (N2 in <= 8 blocks, nx, nq)

}  // namespace d4w
