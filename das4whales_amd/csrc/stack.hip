// Delay-and-sum stack of envelopes over a position grid on MI355X (gfx950): back-projection ("source scanning") of the
// correlogram envelopes along the moveouts |cable - node| / c0, the soft-decision twin of assoc.hip's vote.  Beyond the
// reference, which has nothing of the kind.
//
//   node g = iy nx + ix at (xs[ix], ys[iy], z)                 (misfit_grid's and assoc.hip's layout)
//   d[g][ch] = (int) floor(|cable[ch] - node_g| (1 / c0) fs + 0.5)                                       (stack_delay)
//   stack[g][k - k0] = sum over ch, in increasing ch, of w[ch] env[ch][k + d[g][ch]]
//                      over the channels with w[ch] != 0 and 0 <= k + d[g][ch] < ns,        k0 <= k < k1
//
// Arithmetic.  The delay is moveout.h's: float64, the distance every localisation unit shares, the reciprocal of c0 formed once
// on the host, and no contraction (the header sets it for its own functions): stack_delay is inlined into the table kernel
// and into the arrivals kernel, and beam.hip makes the same two calls, the same sequence of roundings in all three.  The sum
// is float32, one fmaf per term, in increasing channel order, by one thread per element: no atomics, no split over channels,
// so every element has one defined sequence of roundings, is run-to-run bit-identical, and is the same in both forms of the
// kernel.
//
// stack_grid<WINDOW, NORM>: grid (ceil(nt / 1024), tiles); with normalize ceil(nt / 512).  A workgroup of 256 threads owns a
//   tile of 4 x 4 neighbouring nodes (in ix and iy: neighbours in space have neighbouring delays, a run of flat indices would
//   wrap around the grid) and 1024 consecutive columns; a thread owns columns kb + tid + 256 j, j < 4, of all 16 nodes: 64
//   accumulators in registers.  With normalize the weight sums sit beside them, so a thread owns 2 columns (512 per
//   workgroup): 32 + 32.  The 16 delays of a channel are wave-uniform (scalar loads).
//   Window form: per channel the tile needs env[ch][kb + dmin .. kb + 1023 + dmax] (dmin, dmax over the tile's nodes).  The
//   workgroup loads that span once, coalesced and starting at a 128-byte boundary of the row, into one of two LDS buffers of
//   2048 words (1536 with normalize); every thread then reads word (d[n] - dmin) + slack + tid + 256 j for its nodes:
//   consecutive lanes read consecutive words, no bank conflicts.  The loop is double-buffered: the loads of channel ch + 1
//   are issued into registers before the adds of channel ch and written to the other buffer after them, one barrier per
//   channel.  A channel whose whole span lies inside the record takes the loop without the range test (one LDS read and one
//   fma per term).  LDS: 2 x 2048 x 4 B = 16 KiB static (12 KiB with normalize); the tile's delay spread dmax - dmin may be
//   at most 2048 - 1024 - 32 = 992 samples (kStackSpread, the same for both).
//   Direct form: the same loop with env read from global memory, lanes at consecutive addresses (coalesced, unaligned).
//   Compiler's report (gfx950): window 158 VGPRs (152 with normalize), 3 waves per SIMD, no scratch; direct 73 (74), 6 waves.
// stack_spread: the largest dmax - dmin over all tiles and channels of a table, by an integer atomicMax (order-independent).
//   The two forms of stack_grid are both enqueued and read that number on the device: the one it does not select returns at
//   once.  No host read.
// stack_best: 64 columns x 4 node groups per workgroup, lanes along the columns (coalesced), nodes in the loop.
// stack_arrivals: one wave per (call, channel), lanes stride over the window's samples, shuffle reduction.
//
// Cost model, in (node, channel, column) triples: the window form spends one LDS word read and one fma per triple plus
//   (1024 + spread) / (16 x 1024) global words; the direct form one global word read and ~5 vector instructions per triple.
//   ds_read_b32 delivers 32 words per clock and compute unit against 128 fma: the model's limit is the LDS read rate.
#include "moveout.h"

#include <type_traits>

#ifndef D4W_EMU
#pragma clang fp contract(off)
#endif

namespace d4w {

constexpr int kStackThreads = 256;
constexpr int kStackWaves = kStackThreads / 64;
constexpr int kStackTX = 4, kStackTY = 4;                    // the tile of nodes, in ix and iy
constexpr int kStackNodes = kStackTX * kStackTY;
constexpr int kStackAlign = 32;                              // words: the span starts at a 128-byte boundary
constexpr int kStackSpread = 992;                            // largest dmax - dmin within a tile that the window form takes
// columns per thread and per workgroup, words per LDS buffer and of it per thread; with normalize the weight sums double
// the accumulators, so a thread owns half the columns
constexpr int stack_cpt(bool norm) { return norm ? 2 : 4; }
constexpr int stack_cols(bool norm) { return kStackThreads * stack_cpt(norm); }
constexpr int stack_span(bool norm) { return stack_cols(norm) + kStackSpread + kStackAlign; }
constexpr int kBestCols = 64, kBestGroups = kStackThreads / kBestCols;

// the travel time from (px, py, pz) to the channel at (cx, cy, cz) in samples, rounded half up (moveout.h)
__device__ __forceinline__ int stack_delay(double cx, double cy, double cz, double px, double py, double pz, double inv_c0, double fs) {
    return moveout_round(moveout_samples(cx, cy, cz, px, py, pz, inv_c0, fs));
}

__device__ __forceinline__ int stack_wrap_add(int a, int b) { return (int)((unsigned)a + (unsigned)b); }

// grid (ceil(nch / 256), min(ngrid, 65535)); delays [ngrid][nch]
__global__ __launch_bounds__(kStackThreads) void stack_delays(const double* __restrict__ cable, int nch, double inv_c0, double fs,
                                                              const double* __restrict__ xs, int nx, const double* __restrict__ ys,
                                                              int ngrid, double z, int* __restrict__ delays) {
    const int ch = blockIdx.x * kStackThreads + threadIdx.x;
    if (ch >= nch) return;
    const double cx = cable[3 * (size_t)ch], cy = cable[3 * (size_t)ch + 1], cz = cable[3 * (size_t)ch + 2];
    for (int g = blockIdx.y; g < ngrid; g += gridDim.y)
        delays[(size_t)g * (size_t)nch + ch] = stack_delay(cx, cy, cz, xs[g % nx], ys[g / nx], z, inv_c0, fs);
}

// the flat indices of the tile's nodes, clamped into the grid (a clamped node repeats a neighbour: it widens no span)
__device__ __forceinline__ void stack_tile_nodes(int tile, int nx, int ny, int (&g)[kStackNodes]) {
    const int ntx = (nx + kStackTX - 1) / kStackTX;
    const int ix0 = (tile % ntx) * kStackTX, iy0 = (tile / ntx) * kStackTY;
#pragma unroll
    for (int n = 0; n < kStackNodes; ++n)
        g[n] = min(iy0 + n / kStackTX, ny - 1) * nx + min(ix0 + n % kStackTX, nx - 1);
}

// grid = tiles.  info[1] = max(info[1], the tile's largest dmax - dmin over the channels); the caller zeroes info first
__global__ __launch_bounds__(kStackThreads) void stack_spread(const int* __restrict__ delays, int nch, int nx, int ny, int* __restrict__ info) {
    __shared__ int sh[kStackWaves];
    int g[kStackNodes];
    stack_tile_nodes(blockIdx.x, nx, ny, g);
    int m = 0;
    for (int ch = threadIdx.x; ch < nch; ch += kStackThreads) {
        int lo = INT32_MAX, hi = INT32_MIN;
#pragma unroll
        for (int n = 0; n < kStackNodes; ++n) {
            const int d = delays[(size_t)g[n] * (size_t)nch + ch];
            lo = min(lo, d);
            hi = max(hi, d);
        }
        const long long s = (long long)hi - (long long)lo;
        m = max(m, s > (long long)INT32_MAX ? INT32_MAX : (int)s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_down(m, o));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kStackWaves; ++w) m = max(m, sh[w]);
        atomicMax(info + 1, m);
    }
}

// grid (ceil(nt / 512), tiles).  want: 0 = the form info[1] selects, 1 = window, 2 = direct.  info = {form that ran, spread}
template <bool WINDOW, bool NORM>
__global__ __launch_bounds__(kStackThreads) void stack_grid(const float* __restrict__ env, long long pitch, int nch, int ns,
                                                            const int* __restrict__ delays, const float* __restrict__ weights, int nx,
                                                            int ny, int k0, int nt, int want, int* __restrict__ info,
                                                            float* __restrict__ stack) {
    constexpr int kStackCpt = stack_cpt(NORM), kStackCols = stack_cols(NORM), kStackSpan = stack_span(NORM);
    constexpr int kStackLoads = kStackSpan / kStackThreads;
    static_assert(kStackSpan % kStackThreads == 0, "whole span words per thread");
    __shared__ float buf[WINDOW ? 2 : 1][WINDOW ? kStackSpan : 1];
    const int tid = threadIdx.x;
    const bool first = tid == 0 && blockIdx.x == 0 && blockIdx.y == 0;
    if (WINDOW) {
        if (info[1] > kStackSpread) {                        // the table does not fit the window: the direct form's launch
            if (want == 1 && first) info[0] = -1;
            return;
        }
    } else if (want == 0 && info[1] <= kStackSpread) {
        return;
    }
    if (first && info) info[0] = WINDOW ? 1 : 2;

    int g[kStackNodes];
    stack_tile_nodes(blockIdx.y, nx, ny, g);
    const int kb = k0 + (int)blockIdx.x * kStackCols;        // the workgroup's first column; k0 + nt <= 2^30
    const int mis = (int)((reinterpret_cast<uintptr_t>(env) >> 2) & (kStackAlign - 1));

    float acc[kStackNodes][kStackCpt], wsum[NORM ? kStackNodes : 1][kStackCpt];
#pragma unroll
    for (int n = 0; n < kStackNodes; ++n)
#pragma unroll
        for (int j = 0; j < kStackCpt; ++j) {
            acc[n][j] = 0.f;
            if constexpr (NORM) wsum[n][j] = 0.f;
        }

    // the channel in work: its weight, the extremes of its 16 delays, the words between the boundary and its span;
    // the same of the channel in flight; the span words of the latter on their way to LDS
    float w = 0.f, wn = 0.f, regs[kStackLoads];
    int dmin = 0, dmax = 0, slack = 0, dnmin = 0, dnmax = 0, nslack = 0;

    auto open = [&](int ch, float& cw, int& cmin, int& cmax, int& cslack) {
        cw = weights ? weights[ch] : 1.f;
        cmin = INT32_MAX;
        cmax = INT32_MIN;
#pragma unroll
        for (int n = 0; n < kStackNodes; ++n) {
            const int dd = delays[(size_t)g[n] * (size_t)nch + ch];
            cmin = min(cmin, dd);
            cmax = max(cmax, dd);
        }
        const long long e = (long long)mis + (long long)ch * pitch + (long long)stack_wrap_add(kb, cmin);
        cslack = (int)(((e % kStackAlign) + kStackAlign) % kStackAlign);
    };
    auto fetch = [&](int ch, int cmin, int cmax, int cslack) {
        const int lo = stack_wrap_add(kb, cmin) - cslack;                 // sample index of the buffer's word 0
        const int need = cslack + kStackCols + (cmax - cmin);             // <= kStackSpan: the spread was checked
        const float* __restrict__ row = env + (size_t)ch * (size_t)pitch;
#pragma unroll
        for (int r = 0; r < kStackLoads; ++r) {
            const int p = tid + r * kStackThreads;
            const int i = stack_wrap_add(lo, p);
            regs[r] = (p < need && (unsigned)i < (unsigned)ns) ? row[i] : 0.f;
        }
    };
    auto commit = [&](int b) {
#pragma unroll
        for (int r = 0; r < kStackLoads; ++r) buf[b][tid + r * kStackThreads] = regs[r];
    };
    // the 16 x kStackCpt terms of channel ch.  INSIDE: every sample of the span lies within the record (window form only)
    auto terms = [&](int ch, auto inside) {
        constexpr bool INSIDE = decltype(inside)::value;
        const float* __restrict__ row = env + (size_t)ch * (size_t)pitch;
        const float* __restrict__ lds = buf[WINDOW ? (ch & 1) : 0];
#pragma unroll
        for (int n = 0; n < kStackNodes; ++n) {
            const int dd = delays[(size_t)g[n] * (size_t)nch + ch];       // wave-uniform: a scalar load
            const int o = dd - dmin + slack + tid;
#pragma unroll
            for (int j = 0; j < kStackCpt; ++j) {
                if constexpr (INSIDE) {
                    acc[n][j] = fmaf(w, lds[o + j * kStackThreads], acc[n][j]);
                    if constexpr (NORM) wsum[n][j] += w;
                } else {
                    const int i = stack_wrap_add(kb + tid + j * kStackThreads, dd);
                    const bool ok = (unsigned)i < (unsigned)ns;
                    float v;
                    if constexpr (WINDOW) v = lds[o + j * kStackThreads];
                    else v = ok ? row[i] : 0.f;
                    acc[n][j] = ok ? fmaf(w, v, acc[n][j]) : acc[n][j];
                    if constexpr (NORM) wsum[n][j] = ok ? wsum[n][j] + w : wsum[n][j];
                }
            }
        }
    };

    open(0, w, dmin, dmax, slack);
    if (WINDOW) {
        if (w != 0.f) {
            fetch(0, dmin, dmax, slack);
            commit(0);
        }
        __syncthreads();
    }
    for (int ch = 0; ch < nch; ++ch) {
        const bool more = ch + 1 < nch;
        if (more) {
            open(ch + 1, wn, dnmin, dnmax, nslack);
            if (WINDOW && wn != 0.f) fetch(ch + 1, dnmin, dnmax, nslack);
        }
        if (w != 0.f) {                                      // a channel of weight 0 is not read at all
            if (WINDOW && (long long)kb + dmin >= 0 && (long long)kb + (kStackCols - 1) + dmax < (long long)ns) terms(ch, std::true_type());
            else terms(ch, std::false_type());
        }
        if (WINDOW) {
            if (more && wn != 0.f) commit((ch + 1) & 1);
            __syncthreads();
        }
        w = wn;
        dmin = dnmin;
        dmax = dnmax;
        slack = nslack;
    }

    const int ntx = (nx + kStackTX - 1) / kStackTX;
    const int ix0 = ((int)blockIdx.y % ntx) * kStackTX, iy0 = ((int)blockIdx.y / ntx) * kStackTY;
#pragma unroll
    for (int n = 0; n < kStackNodes; ++n) {
        if (ix0 + n % kStackTX >= nx || iy0 + n / kStackTX >= ny) continue;
#pragma unroll
        for (int j = 0; j < kStackCpt; ++j) {
            const long long col = (long long)blockIdx.x * kStackCols + tid + j * kStackThreads;
            if (col >= nt) continue;
            float v = acc[n][j];
            if constexpr (NORM) v = wsum[n][j] != 0.f ? v / wsum[n][j] : 0.f;
            stack[(size_t)g[n] * (size_t)nt + (size_t)col] = v;
        }
    }
}

// "a beats b" for (value, node): a has a node, and b has none, or a is larger, or equal with the smaller node.  NaNs never enter
__device__ __forceinline__ bool stack_beats(float va, int ga, float vb, int gb) { return ga >= 0 && (gb < 0 || va > vb || (va == vb && ga < gb)); }

// grid = ceil(nt / 64).  stack [ngrid][nt]
__global__ __launch_bounds__(kStackThreads) void stack_best(const float* __restrict__ stack, int ngrid, int nt, float* __restrict__ peak,
                                                            int* __restrict__ node) {
    __shared__ float sh_v[kBestGroups][kBestCols];
    __shared__ int sh_g[kBestGroups][kBestCols];
    const int lane = threadIdx.x % kBestCols, grp = threadIdx.x / kBestCols;
    const long long col = (long long)blockIdx.x * kBestCols + lane;
    float bv = 0.f;
    int bg = -1;
    if (col < nt)
        for (int gi = grp; gi < ngrid; gi += kBestGroups) {  // ascending: within a group the first of equals stays
            const float v = stack[(size_t)gi * (size_t)nt + (size_t)col];
            if (v == v && (bg < 0 || v > bv)) {
                bv = v;
                bg = gi;
            }
        }
    sh_v[grp][lane] = bv;
    sh_g[grp][lane] = bg;
    __syncthreads();
    if (grp == 0 && col < nt) {
        for (int q = 1; q < kBestGroups; ++q)
            if (stack_beats(sh_v[q][lane], sh_g[q][lane], bv, bg)) {
                bv = sh_v[q][lane];
                bg = sh_g[q][lane];
            }
        peak[col] = bg >= 0 ? bv : NAN;
        node[col] = bg;
    }
}

// grid (ceil(nch / 4), min(ncalls, 65535)), one wave per (call, channel).  pos [ncalls][3], t0 [ncalls], Ti [ncalls][nch]
__global__ __launch_bounds__(kStackThreads) void stack_arrivals(const float* __restrict__ env, long long pitch, int nch, int ns, double fs,
                                                                const double* __restrict__ cable, double inv_c0,
                                                                const double* __restrict__ pos, const double* __restrict__ t0, int ncalls,
                                                                int h, double threshold, const double* __restrict__ thresholds,
                                                                const float* __restrict__ weights, double* __restrict__ Ti) {
    const int lane = threadIdx.x & 63;
    const int ch = blockIdx.x * kStackWaves + (threadIdx.x >> 6);
    if (ch >= nch) return;                                   // whole waves leave
    const double cx = cable[3 * (size_t)ch], cy = cable[3 * (size_t)ch + 1], cz = cable[3 * (size_t)ch + 2];
    const float w = weights ? weights[ch] : 1.f;
    const double thr = thresholds ? thresholds[ch] : threshold;
    const float* __restrict__ row = env + (size_t)ch * (size_t)pitch;
    for (int c = blockIdx.y; c < ncalls; c += gridDim.y) {
        float bv = 0.f;
        long long bi = -1;
        const double q = floor(t0[c] * fs + 0.5);
        if (w != 0.f && fabs(q) < 1099511627776.0) {         // 2^40; a NaN or infinite emission time has no window
            const long long m = (long long)q + stack_delay(cx, cy, cz, pos[3 * (size_t)c], pos[3 * (size_t)c + 1], pos[3 * (size_t)c + 2], inv_c0, fs);
            const long long a = max(m - h, 0ll), b = min(m + h, (long long)ns - 1);
            for (long long i = a + lane; i <= b; i += 64) {  // ascending: the earliest of equals stays
                const float v = row[i];
                if (v == v && (bi < 0 || v > bv)) {
                    bv = v;
                    bi = i;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_down(bv, o);
            const long long oi = __shfl_down(bi, o);
            if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) {
                bv = ov;
                bi = oi;
            }
        }
        if (lane == 0) Ti[(size_t)c * (size_t)nch + ch] = (bi >= 0 && !((double)bv < thr)) ? (double)bi / fs : NAN;
    }
}

static int stack_check_grid(const char* who, int nx, int ny) {
    if (nx < 1 || ny < 1) return fail(D4W_EINVAL, "%s: the grid %d x %d is empty", who, ny, nx);
    if ((long long)nx * ny > (long long)INT32_MAX / 2) return fail(D4W_EINVAL, "%s: the grid %d x %d has too many nodes", who, ny, nx);
    if ((long long)ceil_div(nx, kStackTX) * ceil_div(ny, kStackTY) > 65535)
        return fail(D4W_EINVAL, "%s: the grid %d x %d has more than 65535 tiles of %d x %d nodes", who, ny, nx, kStackTY, kStackTX);
    return D4W_OK;
}

template <bool WINDOW>
static int stack_launch(const float* env, long long pitch, int nch, int ns, const int32_t* delays, const float* weights, int nx, int ny,
                        int k0, int nt, int normalize, int want, int32_t* info, float* stack, void* stream) {
    const dim3 grid(ceil_div(nt, stack_cols(normalize != 0)), ceil_div(nx, kStackTX) * ceil_div(ny, kStackTY));
    if (normalize)
        D4W_LAUNCH((stack_grid<WINDOW, true>), grid, dim3(kStackThreads), 0, stream, env, pitch, nch, ns, (const int*)delays, weights, nx, ny, k0,
                   nt, want, (int*)info, stack);
    else
        D4W_LAUNCH((stack_grid<WINDOW, false>), grid, dim3(kStackThreads), 0, stream, env, pitch, nch, ns, (const int*)delays, weights, nx, ny, k0,
                   nt, want, (int*)info, stack);
    return D4W_OK;
}

}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_stack_delays_i32(const double* cable_pos, int nch, double c0, double fs, const double* xs, int nx, const double* ys, int ny, double z,
                         int32_t* delays, void* stream) {
    if (!cable_pos || !xs || !ys || !delays) return fail(D4W_EINVAL, "bad argument");
    if (nch < 1) return fail(D4W_EINVAL, "stack_delays: %d channels", nch);
    const int rc = stack_check_grid("stack_delays", nx, ny);
    if (rc) return rc;
    if (!positive_finite(fs) || !positive_finite(c0)) return fail(D4W_EINVAL, "stack_delays: fs and c0 must be positive and finite");
    if (!std::isfinite(z)) return fail(D4W_EINVAL, "stack_delays: z must be finite");
    const int ngrid = nx * ny;
    D4W_LAUNCH(stack_delays, dim3(ceil_div(nch, kStackThreads), min(ngrid, 65535)), dim3(kStackThreads), 0, stream, cable_pos, nch, 1.0 / c0, fs,
               xs, nx, ys, ngrid, z, (int*)delays);
    return D4W_OK;
}

int d4w_stack_grid_f32(const float* env, int64_t pitch, int nch, int ns, const int32_t* delays, const float* weights, int nx, int ny, int k0,
                       int k1, int normalize, int form, float* stack, int32_t* info, void* stream) {
    if (!env || !delays || !stack) return fail(D4W_EINVAL, "bad argument");
    int rc = check_block("stack_grid", nch, ns, pitch);
    if (rc) return rc;
    rc = stack_check_grid("stack_grid", nx, ny);
    if (rc) return rc;
    if (form < 0 || form > 2) return fail(D4W_EINVAL, "stack_grid: form %d is none of 0 (choose), 1 (window), 2 (direct)", form);
    if (form != 2 && !info) return fail(D4W_EINVAL, "stack_grid: form %d decides on the device and needs info", form);
    if (k0 >= k1) return fail(D4W_EINVAL, "stack_grid: the column range [%d, %d) is empty", k0, k1);
    if (k0 < -kMoveoutDelayMax || k1 > kMoveoutDelayMax) return fail(D4W_EINVAL, "stack_grid: the column range [%d, %d) leaves +-2^30", k0, k1);
    if ((long long)k1 - (long long)k0 > (long long)INT32_MAX) return fail(D4W_EINVAL, "stack_grid: the column range [%d, %d) holds more than 2^31 - 1 columns", k0, k1);
    const int nt = k1 - k0;
    if (info) D4W_HIP(hipMemsetAsync(info, 0, 2 * sizeof(int32_t), (hipStream_t)stream));
    if (form != 2) {
        D4W_LAUNCH(stack_spread, dim3(ceil_div(nx, kStackTX) * ceil_div(ny, kStackTY)), dim3(kStackThreads), 0, stream, (const int*)delays, nch,
                   nx, ny, (int*)info);
        rc = stack_launch<true>(env, pitch, nch, ns, delays, weights, nx, ny, k0, nt, normalize, form, info, stack, stream);
        if (rc) return rc;
    }
    if (form != 1) rc = stack_launch<false>(env, pitch, nch, ns, delays, weights, nx, ny, k0, nt, normalize, form, info, stack, stream);
    return rc;
}

int d4w_stack_best_f32(const float* stack, int ngrid, int nt, float* peak, int32_t* node, void* stream) {
    if (!stack || !peak || !node) return fail(D4W_EINVAL, "bad argument");
    if (ngrid < 1 || nt < 1) return fail(D4W_EINVAL, "stack_best: the stack %d x %d is empty", ngrid, nt);
    D4W_LAUNCH(stack_best, dim3(ceil_div(nt, kBestCols)), dim3(kStackThreads), 0, stream, stack, ngrid, nt, peak, (int*)node);
    return D4W_OK;
}

int d4w_stack_arrivals_f64(const float* env, int64_t pitch, int nch, int ns, double fs, const double* cable_pos, double c0, const double* pos,
                           const double* t0, int ncalls, int halfwidth, double threshold, const double* thresholds, const float* weights,
                           double* Ti, void* stream) {
    if (!env || !cable_pos || !pos || !t0 || !Ti) return fail(D4W_EINVAL, "bad argument");
    const int rc = check_block("stack_arrivals", nch, ns, pitch);
    if (rc) return rc;
    if (ncalls < 1) return fail(D4W_EINVAL, "stack_arrivals: %d calls", ncalls);
    if (halfwidth < 0) return fail(D4W_EINVAL, "stack_arrivals: the half-width %d is negative", halfwidth);
    if (!positive_finite(fs) || !positive_finite(c0)) return fail(D4W_EINVAL, "stack_arrivals: fs and c0 must be positive and finite");
    D4W_LAUNCH(stack_arrivals, dim3(ceil_div(nch, kStackWaves), min(ncalls, 65535)), dim3(kStackThreads), 0, stream, env, (long long)pitch, nch,
               ns, fs, cable_pos, 1.0 / c0, pos, t0, ncalls, halfwidth, threshold, thresholds, weights, Ti);
    return D4W_OK;
}

}  // extern "C"
