// Least-squares localisation on MI355X (gfx950) -- the numerical part of the reference's loc.py, batched over calls:
//
//   calc_arrival_times       loc.py:13-25    t0 + |cable - pos| / c0, for many candidate positions at once
//   solve_lq                 loc.py:57-128   damped Gauss-Newton on [x, y, z, t0] (or [x, y, t0] with fix_z)
//   calc_covariance_matrix   loc.py:156-191  G^T G at the returned position (the host inverts it)
//   (new) misfit grid                        per candidate node: best emission time and RMS residual
//
// float64 throughout: positions are tens of kilometres and the answers matter at the millimetre and microsecond level.
// Every output element is written by exactly one thread and every sum has a fixed order: run-to-run bit-identical, no atomics.
// The compiler may not contract a * b + c in this file (pragma below, and moveout.h's own): the distance |cable - pos| is
// moveout.h's moveout_dist, the one every localisation unit uses, and the division by c0 stays here as the reference's
// "/ c0" (the other units multiply by a reciprocal; the two differ in the last bit).  The travel time is then the same
// roundings that NumPy makes, so noise-free arrival times leave residuals of exactly zero at the true position.  The
// accumulations that profit from a fused multiply-add ask for it by name.
//
// loc_solve<FIXZ>: ONE workgroup (256 threads, one compute unit) per call, the whole iteration inside the kernel.  Per
//   iteration the threads stride over the channels; a channel whose arrival time is NaN carries no pick and is skipped.  With
//   d = n[:3] - cable, r = |d_xy|, R = |d| the reference's row of G is
//       cos(th) cos(ph) / c0, cos(th) sin(ph) / c0, sin(th) / c0, 1     th = atan2(|d_z|, r), ph = atan2(d_y, d_x)
//   which is d_x / (R c0), d_y / (R c0), |d_z| / (R c0), 1 -- the algebraic form, one division and no trigonometry.  |d_z| is
//   the reference's (its z column does not change sign below the cable) and stays.  r = 0 is where the two forms part:
//   atan2(0, 0) = 0 makes ph = 0, and th = pi / 2 (R > 0; cos(pi / 2) = 6.1e-17 in float64) or th = 0 (R = 0); those rows are
//   written out as the reference computes them.  Each thread keeps the upper triangle of G^T G, G^T dt, sum dt^2 and the pick
//   count in registers (16 sums, 11 with fix_z); they are added within the wave by shuffles and across the four waves through
//   LDS in wave order.  Thread 0 adds lambda = 1e-5 on the diagonal, solves the 4 x 4 (3 x 3) system by Cholesky (the matrix
//   is positive definite by construction), applies the reference's step -- 0.7 dn for the first four iterations, dn after --
//   writes the iterate to the history and shares it through LDS.  One more pass over the channels after the last step gives
//   G^T G without lambda, the sum of squared residuals and the pick count AT the returned position.
//   Work per call: (Nbiter + 1) nch rows of ~45 float64 operations, one square root and two divisions; the 11 020 x 4 doubles
//   of a call (353 KB) stay in L2 between iterations.  One call cannot be faster than one compute unit: the kernel is for batches.
// loc_misfit_grid: one thread per node of a 64 x 4 tile, grid z = call.  Cable coordinates and the call's arrival times are
//   staged through LDS in chunks of 256 channels (one global load per workgroup, every thread then reads the same LDS address:
//   a broadcast, no bank conflicts).  e_j = Ti_j - |cable_j - node| / c0 is accumulated in channel order as sum (e_j - K) and
//   sum (e_j - K)^2 with K = e of the node's first picked channel, so that the variance does not cancel against the square of
//   an emission time of tens of seconds: t0 = K + mean, rms = sqrt(mean square - mean^2).  At a node where every e_j is the
//   same the result is exactly rms = 0.
// loc_arrival_times: one thread per (position, channel).
#include "loc_common.h"

#ifndef D4W_EMU
#pragma clang fp contract(off)
#endif

namespace d4w {

constexpr int kLocSums = 16;                     // 10 + 4 + 2 (free z); 6 + 3 + 2 with fix_z
constexpr int kLocChunk = 256;                   // channels staged per LDS chunk of the grid kernel
constexpr int kLocTileW = 64, kLocTileH = 4;     // nodes per workgroup of the grid kernel

// grid = ncalls.  hist [ncalls][nbiter][4], out_n [ncalls][4], gtg [ncalls][NP][NP], ssr [ncalls], npick [ncalls]
template <bool FIXZ>
__global__ __launch_bounds__(kLocThreads) void loc_solve(const double* __restrict__ cable, int nch, const double* __restrict__ Ti,
                                                         double c0, int nbiter, const double* __restrict__ first_guess,
                                                         double* __restrict__ hist, double* __restrict__ out_n,
                                                         double* __restrict__ gtg, double* __restrict__ ssr, int* __restrict__ npick) {
    constexpr int NP = FIXZ ? 3 : 4;
    constexpr int NT = NP * (NP + 1) / 2;
    constexpr int NS = NT + NP + 2;              // + sum dt^2 + pick count
    __shared__ double wsum[kLocWaves * kLocSums];
    __shared__ double n_sh[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t call = blockIdx.x;
    const double* __restrict__ t = Ti + call * (size_t)nch;

    if (first_guess) {
        if (tid < 4) n_sh[tid] = first_guess[call * 4 + tid];
    } else {                                     // loc.py:86, the minimum over the channels that carry a pick
        double m = INFINITY;
        for (int ch = tid; ch < nch; ch += kLocThreads) {
            const double v = t[ch];
            if (v == v) m = fmin(m, v);
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
        double s[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) s[i] = 0.0;
        for (int ch = tid; ch < nch; ch += kLocThreads) {
            const double tt = t[ch];
            if (tt != tt) continue;
            double g[4], R;
            loc_row(n0, n1, n2, cable[3 * (size_t)ch], cable[3 * (size_t)ch + 1], cable[3 * (size_t)ch + 2], c0, g[0], g[1], g[2], R);
            if (FIXZ) g[2] = 1.0; else g[3] = 1.0;
            const double dt = tt - (n3 + R / c0);
            int q = 0;
#pragma unroll
            for (int i = 0; i < NP; ++i)
#pragma unroll
                for (int k = i; k < NP; ++k) {
                    s[q] = fma(g[i], g[k], s[q]);
                    ++q;
                }
#pragma unroll
            for (int i = 0; i < NP; ++i) s[NT + i] = fma(g[i], dt, s[NT + i]);
            s[NT + NP] = fma(dt, dt, s[NT + NP]);
            s[NT + NP + 1] += 1.0;
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            s[i] = loc_wave_sum(s[i]);
            if (lane == 0) wsum[wave * kLocSums + i] = s[i];
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < NS; ++i)
                for (int w = 1; w < kLocWaves; ++w) s[i] += wsum[w * kLocSums + i];
            const bool none = !(s[NT + NP + 1] > 0.0);       // a call without a pick: a NaN row
            if (j == nbiter) {
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
                npick[call] = (int)s[NT + NP + 1];
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

// grid (ceil(nx / 64), ceil(ny / 4), ncalls).  rms, t0 [ncalls][ny][nx]
__global__ __launch_bounds__(kLocThreads) void loc_misfit_grid(const double* __restrict__ cable, int nch, const double* __restrict__ Ti,
                                                               double c0, const double* __restrict__ xs, int nx,
                                                               const double* __restrict__ ys, int ny, double z,
                                                               double* __restrict__ rms, double* __restrict__ t0) {
    __shared__ double sc[4 * kLocChunk];         // x, y, z, arrival time of the staged channels
    const int tid = threadIdx.x;
    const int ix = blockIdx.x * kLocTileW + (tid & (kLocTileW - 1)), iy = blockIdx.y * kLocTileH + tid / kLocTileW;
    const size_t call = blockIdx.z;
    const bool live = ix < nx && iy < ny;
    const double px = live ? xs[ix] : 0.0, py = live ? ys[iy] : 0.0;
    const double* __restrict__ t = Ti + call * (size_t)nch;
    double K = 0.0, s1 = 0.0, s2 = 0.0;
    int cnt = 0;
    for (int base = 0; base < nch; base += kLocChunk) {
        const int ch = base + tid;
        if (ch < nch) {
            sc[tid] = cable[3 * (size_t)ch];
            sc[kLocChunk + tid] = cable[3 * (size_t)ch + 1];
            sc[2 * kLocChunk + tid] = cable[3 * (size_t)ch + 2];
            sc[3 * kLocChunk + tid] = t[ch];
        }
        __syncthreads();
        const int m = min(kLocChunk, nch - base);
        for (int k = 0; k < m; ++k) {
            const double tt = sc[3 * kLocChunk + k];
            if (tt != tt) continue;              // the same for every thread of the workgroup
            double e = tt - moveout_dist(sc[k], sc[kLocChunk + k], sc[2 * kLocChunk + k], px, py, z) / c0;
            if (cnt == 0) K = e;
            e -= K;
            s1 += e;
            s2 = fma(e, e, s2);
            ++cnt;
        }
        __syncthreads();
    }
    if (!live) return;
    const size_t o = (call * (size_t)ny + iy) * (size_t)nx + ix;
    if (cnt == 0) {
        rms[o] = NAN;
        t0[o] = NAN;
        return;
    }
    const double mean = s1 / (double)cnt;
    const double var = s2 / (double)cnt - mean * mean;
    rms[o] = var > 0.0 ? sqrt(var) : 0.0;
    t0[o] = K + mean;
}

// grid (ceil(nch / 256), npos).  out [npos][nch] = t0[p] + |cable[ch] - pos[p]| / c0
__global__ __launch_bounds__(kLocThreads) void loc_arrival_times(const double* __restrict__ cable, int nch, const double* __restrict__ pos,
                                                                 const double* __restrict__ t0, double c0, double* __restrict__ out) {
    const int ch = blockIdx.x * kLocThreads + threadIdx.x;
    if (ch >= nch) return;
    const size_t p = blockIdx.y;
    const double d = moveout_dist(cable[3 * (size_t)ch], cable[3 * (size_t)ch + 1], cable[3 * (size_t)ch + 2], pos[3 * p], pos[3 * p + 1],
                                  pos[3 * p + 2]);
    out[p * (size_t)nch + ch] = t0[p] + d / c0;
}

}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_loc_solve_f64(const double* cable_pos, int nch, const double* Ti, int ncalls, double c0, int nbiter, int fix_z,
                      const double* first_guess, double* history, double* n_out, double* gtg, double* ssr, int* npick,
                      void* stream) {
    if (!cable_pos || !Ti || !n_out || !gtg || !ssr || !npick) return fail(D4W_EINVAL, "bad argument");
    if (nch < 1) return fail(D4W_EINVAL, "loc_solve: %d channels", nch);
    if (ncalls < 0) return fail(D4W_EINVAL, "loc_solve: %d calls", ncalls);
    if (!positive_finite(c0)) return fail(D4W_EINVAL, "loc_solve: the speed of sound must be positive and finite");
    if (nbiter < 0 || nbiter > 100000) return fail(D4W_EINVAL, "loc_solve: Nbiter = %d is not within 0 .. 100000", nbiter);
    if (nbiter > 0 && !history) return fail(D4W_EINVAL, "loc_solve: the history of %d iterations needs its output", nbiter);
    if (ncalls == 0) return D4W_OK;
    if (fix_z)
        D4W_LAUNCH(loc_solve<true>, dim3(ncalls), dim3(kLocThreads), 0, stream, cable_pos, nch, Ti, c0, nbiter, first_guess, history,
                   n_out, gtg, ssr, npick);
    else
        D4W_LAUNCH(loc_solve<false>, dim3(ncalls), dim3(kLocThreads), 0, stream, cable_pos, nch, Ti, c0, nbiter, first_guess, history,
                   n_out, gtg, ssr, npick);
    return D4W_OK;
}

int d4w_loc_misfit_grid_f64(const double* cable_pos, int nch, const double* Ti, int ncalls, double c0, const double* xs, int nx,
                            const double* ys, int ny, double z, double* rms, double* t0, void* stream) {
    if (!cable_pos || !Ti || !xs || !ys || !rms || !t0) return fail(D4W_EINVAL, "bad argument");
    if (nch < 1) return fail(D4W_EINVAL, "loc_misfit_grid: %d channels", nch);
    if (ncalls < 0 || ncalls > 65535) return fail(D4W_EINVAL, "loc_misfit_grid: %d calls is not within 0 .. 65535", ncalls);
    if (nx < 1 || ny < 1) return fail(D4W_EINVAL, "loc_misfit_grid: the grid %d x %d is empty", ny, nx);
    if (ceil_div(ny, kLocTileH) > 65535) return fail(D4W_EINVAL, "loc_misfit_grid: %d grid rows exceed the grid limit", ny);
    if (!positive_finite(c0)) return fail(D4W_EINVAL, "loc_misfit_grid: the speed of sound must be positive and finite");
    if (!std::isfinite(z)) return fail(D4W_EINVAL, "loc_misfit_grid: z must be finite");
    if (ncalls == 0) return D4W_OK;
    const dim3 grid(ceil_div(nx, kLocTileW), ceil_div(ny, kLocTileH), ncalls);
    D4W_LAUNCH(loc_misfit_grid, grid, dim3(kLocThreads), 0, stream, cable_pos, nch, Ti, c0, xs, nx, ys, ny, z, rms, t0);
    return D4W_OK;
}

int d4w_loc_arrival_times_f64(const double* cable_pos, int nch, const double* pos, const double* t0, int npos, double c0,
                              double* out, void* stream) {
    if (!cable_pos || !pos || !t0 || !out) return fail(D4W_EINVAL, "bad argument");
    if (nch < 1) return fail(D4W_EINVAL, "loc_arrival_times: %d channels", nch);
    if (npos < 0 || npos > 65535) return fail(D4W_EINVAL, "loc_arrival_times: %d positions is not within 0 .. 65535", npos);
    if (!positive_finite(c0)) return fail(D4W_EINVAL, "loc_arrival_times: the speed of sound must be positive and finite");
    if (npos == 0) return D4W_OK;
    D4W_LAUNCH(loc_arrival_times, dim3(ceil_div(nch, kLocThreads), npos), dim3(kLocThreads), 0, stream, cable_pos, nch, pos, t0, c0,
               out);
    return D4W_OK;
}

}  // extern "C"
