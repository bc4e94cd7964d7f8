// Association of picks into calls on MI355X (gfx950): a delay-and-vote over a position grid, a Hough transform over the
// hyperbolic moveouts |cable - node| / c0.  Beyond the reference, whose loc.solve_lq is fed hand-selected times.
//
//   pick k: channel ch_k, sample i_k, t_k = i_k / fs          node g = iy nx + ix at (xs[ix], ys[iy], z)   (misfit_grid's layout)
//   e_kg = t_k - |cable[ch_k] - node_g| / c0                   bin(k, g) = floor((e_kg - lo) / dt)       (the distance: moveout.h)
//   votes[g][b] = #{k : bin(k, g) = b}, 0 <= b < nbins         s[g][b] = votes[g][b] + votes[g][b + 1], 0 <= b < nbins - 1
//
// One greedy round: the arg-max (g*, b*) of s (assoc_best), per channel the unassigned pick of bins b*, b* + 1 at g* nearest
// the window centre lo + (b* + 1) dt (assoc_select), and the chosen picks' votes taken off every node again (assoc_vote with
// sign -1 over the chosen-index list).  After every round the accumulator is the vote of the still-unassigned picks counted
// from scratch, because vote, select and subtract compute bin(k, g) with the same two inlined functions below (assoc_emit,
// assoc_bin) from the same inputs.
//
// Arithmetic.  float64 throughout, as in loc.hip.  The compiler may not contract a * b + c in this file (pragma below): the
// three kernels inline the bin function into different surroundings, and only without contraction is it the same sequence of
// roundings in each of them -- the invariant above rests on that, not on luck of the optimiser.  t_k = i_k / fs is a true
// division (the arrival times handed on to loc.solve_lq are NumPy's i / fs bit for bit).  The two divisions by c0 and dt are
// multiplications by reciprocals formed once on the host: q = (e - lo) / dt then differs from a divide-twice evaluation by a
// few ulp of q (about 1e-11 at |e| = 100 s, dt = 0.01 s), which moves a pick to the neighbouring bin only when q is that
// close to an integer.  The square root is the correctly rounded one.  Votes are integers: the histogram is independent of
// the order in which lanes add to it, so every result is run-to-run bit-identical although LDS atomics are used.
//
// assoc_vote: grid (ceil(G / 8), ceil(nbins / 1024)).  A workgroup of 256 threads owns the histogram rows of 8 consecutive
//   nodes over 1024 consecutive bins in LDS: 8 x 1024 x 4 B = 32 KiB (static; five workgroups fit a compute unit's 160 KiB).
//   Its threads stride over the picks (or over an index list, -1 = skip); a thread loads its pick once (16 B of the packed
//   table, the channel's three coordinates -- picks are ordered by channel, so neighbouring lanes read the same cache line),
//   forms t_k with the call's one division, and evaluates the 8 nodes from registers: per (pick, node) pair one square root,
//   ~14 float64 operations and one LDS integer atomic (ds_add_u32; lanes of one call hitting one bin at the true node
//   serialise there, nowhere else).  The tile then leaves with plain stores, votes[g][b] = sign * count or
//   votes[g][b] += sign * count: every element of votes belongs to exactly one workgroup, no global atomics.  nbins > 1024:
//   the second grid dimension walks the bin ranges, each workgroup streaming the picks again for its range (nbins = 65 536:
//   64 ranges).  The subtract pass of a round costs nch index entries per workgroup and stores only the bins it changed.
// assoc_best: two stages.  Stage one: a wave per node row (grid-stride over the rows, at most 1024 workgroups of 4 waves),
//   lanes stride over the pairs, keep (score, flat index) with "larger score, then smaller flat index g (nbins - 1) + b",
//   reduce by shuffles and through LDS, one partial per workgroup.  Stage two: one workgroup reduces the partials and writes
//   the round's record, or sets the stop flag when the score is below min_picks.
// assoc_select: one thread per channel over that channel's contiguous range of the pick table (offsets = the inclusive prefix
//   sum of the per-channel counts, d4w_pick_offsets_i64); then one workgroup sums the chosen emission times in a fixed tree
//   order for the call's first guess.
// Every kernel first reads the stop flag (state[0]) and returns when it is set: a caller enqueues all rounds up front without
// a host synchronisation and reads state[1], the number of calls found, once at the end.
//
// Cost model, in (pick, node) pair evaluations: initial vote K G ceil(nbins / 1024); per round at most nch G for the subtract,
// (K / nch) nch = K for the select, and one read of the G nbins accumulator for the arg-max.
#include "moveout.h"

#ifndef D4W_EMU
#pragma clang fp contract(off)
#endif

namespace d4w {

constexpr int kAssocThreads = 256;
constexpr int kAssocWaves = kAssocThreads / 64;
constexpr int kAssocNodes = 8;                   // nodes per workgroup of the vote
constexpr int kAssocBins = 1024;                 // bins per node of the LDS histogram tile
constexpr int kAssocParts = 1024;                // most partial results of the arg-max's first stage

// emission time of a pick at time t on the channel at (cx, cy, cz), heard from the node (px, py, pz)
__device__ __forceinline__ double assoc_emit(double t, double cx, double cy, double cz, double px, double py, double pz, double inv_c0) {
    return t - moveout_dist(cx, cy, cz, px, py, pz) * inv_c0;
}
// the bin of emission time e, -1 outside 0 .. nbins - 1 (and for a NaN)
__device__ __forceinline__ int assoc_bin(double e, double lo, double inv_dt, int nbins) {
    const double q = floor((e - lo) * inv_dt);
    return (q >= 0.0 && q < (double)nbins) ? (int)q : -1;
}

// "a beats b": the larger score, then the smaller flat index
__device__ __forceinline__ bool assoc_beats(int sa, long long ia, int sb, long long ib) { return sa > sb || (sa == sb && ia < ib); }

// the best (score, index) of the workgroup in thread 0; every thread of the workgroup calls it
__device__ __forceinline__ void assoc_block_best(int& s, long long& i, int* sh_s, long long* sh_i) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int so = __shfl_down(s, o);
        const long long io = __shfl_down(i, o);
        if (assoc_beats(so, io, s, i)) { s = so; i = io; }
    }
    if (lane == 0) { sh_s[wave] = s; sh_i[wave] = i; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kAssocWaves; ++w)
            if (assoc_beats(sh_s[w], sh_i[w], s, i)) { s = sh_s[w]; i = sh_i[w]; }
}

// grid (ceil(ngrid / 8), ceil(nbins / 1024)).  picks [2][npicks] int64 (row 0 channel, row 1 sample); idx [nidx] or null
__global__ __launch_bounds__(kAssocThreads) void assoc_vote(const long long* __restrict__ picks, int npicks, const int* __restrict__ idx,
                                                            int nidx, int sign, int accumulate, const double* __restrict__ cable, int nch,
                                                            double fs, double inv_c0, const double* __restrict__ xs, int nx,
                                                            const double* __restrict__ ys, int ngrid, double z, double lo, double inv_dt,
                                                            int nbins, int* __restrict__ votes, const int* __restrict__ stop) {
    __shared__ int hist[kAssocNodes * kAssocBins];
    if (stop && *stop) return;
    const int tid = threadIdx.x;
    const int g0 = blockIdx.x * kAssocNodes, b0 = blockIdx.y * kAssocBins;
    const int nn = min(kAssocNodes, ngrid - g0), nb = min(kAssocBins, nbins - b0);
    double px[kAssocNodes], py[kAssocNodes];
#pragma unroll
    for (int n = 0; n < kAssocNodes; ++n) {
        const int g = min(g0 + n, ngrid - 1);
        px[n] = xs[g % nx];
        py[n] = ys[g / nx];
    }
    for (int i = tid; i < kAssocNodes * kAssocBins; i += kAssocThreads) hist[i] = 0;
    __syncthreads();
    const int count = idx ? nidx : npicks;
    for (int j = tid; j < count; j += kAssocThreads) {
        int k = j;
        if (idx) {
            k = idx[j];
            if (k < 0 || k >= npicks) continue;  // -1: no pick chosen on this channel
        }
        const long long ch = picks[k];
        if (ch < 0 || ch >= nch) continue;
        const double t = (double)picks[(size_t)npicks + k] / fs;
        const double cx = cable[3 * (size_t)ch], cy = cable[3 * (size_t)ch + 1], cz = cable[3 * (size_t)ch + 2];
#pragma unroll
        for (int n = 0; n < kAssocNodes; ++n) {
            if (n >= nn) continue;
            const int b = assoc_bin(assoc_emit(t, cx, cy, cz, px[n], py[n], z, inv_c0), lo, inv_dt, nbins) - b0;
            if ((unsigned)b < (unsigned)nb) atomicAdd(&hist[n * kAssocBins + b], 1);
        }
    }
    __syncthreads();
    for (int i = tid; i < nn * kAssocBins; i += kAssocThreads) {
        const int n = i / kAssocBins, b = i % kAssocBins;
        if (b >= nb) continue;
        const size_t o = (size_t)(g0 + n) * (size_t)nbins + (size_t)(b0 + b);
        const int v = sign * hist[i];
        if (!accumulate) votes[o] = v;
        else if (v) votes[o] += v;
    }
}

// stage one: grid = nparts workgroups; part_s [nparts], part_i [nparts]
__global__ __launch_bounds__(kAssocThreads) void assoc_best_rows(const int* __restrict__ votes, int ngrid, int nbins, const int* __restrict__ state,
                                                                 int* __restrict__ part_s, long long* __restrict__ part_i) {
    __shared__ int sh_s[kAssocWaves];
    __shared__ long long sh_i[kAssocWaves];
    if (state[0]) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int s = INT32_MIN;
    long long i = INT64_MAX;
    for (long long g = (long long)blockIdx.x * kAssocWaves + wave; g < ngrid; g += (long long)gridDim.x * kAssocWaves) {
        const int* __restrict__ v = votes + (size_t)g * (size_t)nbins;
        for (int b = lane; b < nbins - 1; b += 64) {
            const int p = v[b] + v[b + 1];
            const long long f = g * (long long)(nbins - 1) + b;
            if (assoc_beats(p, f, s, i)) { s = p; i = f; }
        }
    }
    assoc_block_best(s, i, sh_s, sh_i);
    if (threadIdx.x == 0) {
        part_s[blockIdx.x] = s;
        part_i[blockIdx.x] = i;
    }
}

// stage two: one workgroup.  state = {stop, calls found}; rec [.][4] = node, bin, score, picks
__global__ __launch_bounds__(kAssocThreads) void assoc_best_final(const int* __restrict__ part_s, const long long* __restrict__ part_i, int nparts,
                                                                  int nbins, int min_picks, int call, int* __restrict__ state,
                                                                  int* __restrict__ rec) {
    __shared__ int sh_s[kAssocWaves];
    __shared__ long long sh_i[kAssocWaves];
    if (state[0]) return;
    int s = INT32_MIN;
    long long i = INT64_MAX;
    for (int p = threadIdx.x; p < nparts; p += kAssocThreads)
        if (assoc_beats(part_s[p], part_i[p], s, i)) { s = part_s[p]; i = part_i[p]; }
    assoc_block_best(s, i, sh_s, sh_i);
    if (threadIdx.x == 0) {
        if (s < min_picks) {
            state[0] = 1;
        } else {
            rec[4 * (size_t)call] = (int)(i / (nbins - 1));
            rec[4 * (size_t)call + 1] = (int)(i % (nbins - 1));
            rec[4 * (size_t)call + 2] = s;
            rec[4 * (size_t)call + 3] = 0;
            state[1] = call + 1;
        }
    }
}

// grid = ceil(nch / 256), one thread per channel.  offsets [nch] = inclusive prefix sum of the per-channel pick counts
__global__ __launch_bounds__(kAssocThreads) void assoc_select(const long long* __restrict__ picks, int npicks, const long long* __restrict__ offsets,
                                                              const double* __restrict__ cable, int nch, double fs, double inv_c0,
                                                              const double* __restrict__ xs, int nx, const double* __restrict__ ys, double z,
                                                              double lo, double dt, double inv_dt, int nbins, int call,
                                                              const int* __restrict__ state, const int* __restrict__ rec,
                                                              int* __restrict__ assigned, double* __restrict__ Ti, int* __restrict__ chosen,
                                                              double* __restrict__ e_chosen) {
    if (state[0]) return;
    const int ch = blockIdx.x * kAssocThreads + threadIdx.x;
    if (ch >= nch) return;
    const int g = rec[4 * (size_t)call], bs = rec[4 * (size_t)call + 1];
    const double px = xs[g % nx], py = ys[g / nx];
    const double ec = lo + (double)(bs + 1) * dt;            // the centre of the two-bin window
    const double cx = cable[3 * (size_t)ch], cy = cable[3 * (size_t)ch + 1], cz = cable[3 * (size_t)ch + 2];
    const long long ka = min(max(ch ? offsets[ch - 1] : 0ll, 0ll), (long long)npicks);
    const long long kb = min(max(offsets[ch], ka), (long long)npicks);
    int best = -1;
    double bd = INFINITY, be = NAN, bt = NAN;
    for (long long k = ka; k < kb; ++k) {
        if (assigned[k]) continue;
        const double t = (double)picks[(size_t)npicks + k] / fs;
        const double e = assoc_emit(t, cx, cy, cz, px, py, z, inv_c0);
        const int b = assoc_bin(e, lo, inv_dt, nbins);
        if (b != bs && b != bs + 1) continue;
        const double d = fabs(e - ec);
        if (best < 0 || d < bd) {                            // ties keep the smaller k
            best = (int)k;
            bd = d;
            be = e;
            bt = t;
        }
    }
    Ti[(size_t)call * (size_t)nch + ch] = bt;
    chosen[ch] = best;
    e_chosen[ch] = be;
    if (best >= 0) assigned[best] = call + 1;
}

// one workgroup: the call's pick count and first guess [x, y, z, mean emission time of the chosen picks]
__global__ __launch_bounds__(kAssocThreads) void assoc_record(const int* __restrict__ chosen, const double* __restrict__ e_chosen, int nch,
                                                              const double* __restrict__ xs, int nx, const double* __restrict__ ys, double z,
                                                              int call, const int* __restrict__ state, int* __restrict__ rec,
                                                              double* __restrict__ first_guess) {
    __shared__ double sh_e[kAssocWaves];
    __shared__ int sh_n[kAssocWaves];
    if (state[0]) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double s = 0.0;
    int n = 0;
    for (int ch = threadIdx.x; ch < nch; ch += kAssocThreads)
        if (chosen[ch] >= 0) {
            s += e_chosen[ch];
            ++n;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_down(s, o);
        n += __shfl_down(n, o);
    }
    if (lane == 0) { sh_e[wave] = s; sh_n[wave] = n; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kAssocWaves; ++w) { s += sh_e[w]; n += sh_n[w]; }
        const int g = rec[4 * (size_t)call];
        rec[4 * (size_t)call + 3] = n;
        first_guess[4 * (size_t)call] = xs[g % nx];
        first_guess[4 * (size_t)call + 1] = ys[g / nx];
        first_guess[4 * (size_t)call + 2] = z;
        first_guess[4 * (size_t)call + 3] = n ? s / (double)n : NAN;
    }
}

// the checks the three entry points share; 0 or D4W_EINVAL with the message left behind
static int assoc_check(const char* who, int npicks, int nch, int nx, int ny, int nbins, double fs, double c0, double dt, double lo, double z) {
    if (npicks < 0 || npicks > (1 << 30)) return fail(D4W_EINVAL, "%s: %d picks is not within 0 .. 2^30", who, npicks);
    if (nch < 1) return fail(D4W_EINVAL, "%s: %d channels", who, nch);
    if (nx < 1 || ny < 1) return fail(D4W_EINVAL, "%s: the grid %d x %d is empty", who, ny, nx);
    if ((long long)nx * ny > INT32_MAX - kAssocNodes) return fail(D4W_EINVAL, "%s: the grid %d x %d has too many nodes", who, ny, nx);
    if (nbins < 2) return fail(D4W_EINVAL, "%s: %d bins, the pair score needs two", who, nbins);
    if (ceil_div(nbins, kAssocBins) > 65535) return fail(D4W_EINVAL, "%s: %d bins exceed the grid limit", who, nbins);
    if (!positive_finite(fs) || !positive_finite(c0) || !positive_finite(dt)) return fail(D4W_EINVAL, "%s: fs, c0 and dt must be positive and finite", who);
    if (!std::isfinite(lo) || !std::isfinite(z)) return fail(D4W_EINVAL, "%s: lo and z must be finite", who);
    return D4W_OK;
}

}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_assoc_vote_i32(const int64_t* picks, int npicks, const int32_t* idx, int nidx, int sign, int accumulate, const double* cable_pos,
                       int nch, double fs, double c0, const double* xs, int nx, const double* ys, int ny, double z, double lo, double dt,
                       int nbins, int32_t* votes, const int32_t* stop, void* stream) {
    if (!cable_pos || !xs || !ys || !votes || (npicks > 0 && !picks)) return fail(D4W_EINVAL, "bad argument");
    if (sign != 1 && sign != -1) return fail(D4W_EINVAL, "assoc_vote: sign %d is neither +1 nor -1", sign);
    if (nidx < 0) return fail(D4W_EINVAL, "assoc_vote: %d index entries", nidx);
    const int rc = assoc_check("assoc_vote", npicks, nch, nx, ny, nbins, fs, c0, dt, lo, z);
    if (rc) return rc;
    const int ngrid = nx * ny;
    const dim3 grid(ceil_div(ngrid, kAssocNodes), ceil_div(nbins, kAssocBins));
    D4W_LAUNCH(assoc_vote, grid, dim3(kAssocThreads), 0, stream, (const long long*)picks, npicks, idx, nidx, sign, accumulate ? 1 : 0, cable_pos,
               nch, fs, 1.0 / c0, xs, nx, ys, ngrid, z, lo, 1.0 / dt, nbins, votes, stop);
    return D4W_OK;
}

size_t d4w_assoc_best_ws_bytes(void) { return (size_t)kAssocParts * (sizeof(long long) + sizeof(int)); }

int d4w_assoc_best_i32(const int32_t* votes, int nx, int ny, int nbins, int min_picks, int call, int32_t* state, int32_t* rec, void* ws,
                       void* stream) {
    if (!votes || !state || !rec || !ws) return fail(D4W_EINVAL, "bad argument");
    if (nx < 1 || ny < 1) return fail(D4W_EINVAL, "assoc_best: the grid %d x %d is empty", ny, nx);
    if ((long long)nx * ny > INT32_MAX - kAssocNodes) return fail(D4W_EINVAL, "assoc_best: the grid %d x %d has too many nodes", ny, nx);
    if (nbins < 2) return fail(D4W_EINVAL, "assoc_best: %d bins, the pair score needs two", nbins);
    if (call < 0) return fail(D4W_EINVAL, "assoc_best: call %d", call);
    const int ngrid = nx * ny;
    const int nparts = min(ceil_div(ngrid, kAssocWaves), kAssocParts);
    long long* part_i = static_cast<long long*>(ws);         // [kAssocParts] int64, then [kAssocParts] int32
    int* part_s = reinterpret_cast<int*>(part_i + kAssocParts);
    D4W_LAUNCH(assoc_best_rows, dim3(nparts), dim3(kAssocThreads), 0, stream, votes, ngrid, nbins, (const int*)state, part_s, part_i);
    D4W_LAUNCH(assoc_best_final, dim3(1), dim3(kAssocThreads), 0, stream, (const int*)part_s, (const long long*)part_i, nparts, nbins, min_picks,
               call, state, rec);
    return D4W_OK;
}

int d4w_assoc_select_f64(const int64_t* picks, int npicks, const int64_t* offsets, const double* cable_pos, int nch, double fs, double c0,
                         const double* xs, int nx, const double* ys, int ny, double z, double lo, double dt, int nbins, int call,
                         const int32_t* state, int32_t* rec, int32_t* assigned, double* Ti, int32_t* chosen, double* e_chosen,
                         double* first_guess, void* stream) {
    if (!offsets || !cable_pos || !xs || !ys || !state || !rec || !Ti || !chosen || !e_chosen || !first_guess ||
        (npicks > 0 && (!picks || !assigned)))
        return fail(D4W_EINVAL, "bad argument");
    if (call < 0) return fail(D4W_EINVAL, "assoc_select: call %d", call);
    const int rc = assoc_check("assoc_select", npicks, nch, nx, ny, nbins, fs, c0, dt, lo, z);
    if (rc) return rc;
    D4W_LAUNCH(assoc_select, dim3(ceil_div(nch, kAssocThreads)), dim3(kAssocThreads), 0, stream, (const long long*)picks, npicks,
               (const long long*)offsets, cable_pos, nch, fs, 1.0 / c0, xs, nx, ys, z, lo, dt, 1.0 / dt, nbins, call, state, (const int*)rec,
               assigned, Ti, chosen, e_chosen);
    D4W_LAUNCH(assoc_record, dim3(1), dim3(kAssocThreads), 0, stream, (const int*)chosen, (const double*)e_chosen, nch, xs, nx, ys, z, call,
               state, rec, first_guess);
    return D4W_OK;
}

}  // extern "C"
