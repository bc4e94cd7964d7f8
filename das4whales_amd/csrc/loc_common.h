// The pieces of the Gauss-Newton localisation that loc.hip (loc_solve) and robust.hip (robust_solve) share: the workgroup
// shape, the wave reductions, the reference's row of G and the Cholesky solve of the normal equations.  They were loc.hip's
// own until the robust solver needed the same roundings: "l2 without weights equals solve_lq_batch bit for bit" is a property
// of this header and not of two texts kept alike by hand.  No contraction (moveout.h's pragma and the units' own).
#pragma once
#include "moveout.h"

#ifndef D4W_EMU
#pragma clang fp contract(off)
#endif

namespace d4w {

constexpr int kLocThreads = 256;
constexpr int kLocWaves = kLocThreads / 64;
constexpr double kLocLambda = 1e-5;              // loc.py:89
constexpr double kLocCosHalfPi = 6.123233995736766e-17;   // cos(atan2(|dz|, 0)) in float64

__device__ __forceinline__ double loc_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;                                    // lane 0 holds the wave's sum
}
__device__ __forceinline__ double loc_wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_down(v, o));
    return v;
}

// the reference's row of G without the trailing 1, and R, for the position (nx, ny, nz) and the channel at (cx, cy, cz)
__device__ __forceinline__ void loc_row(double nx, double ny, double nz, double cx, double cy, double cz, double c0, double& g0, double& g1,
                                        double& g2, double& R) {
    const double dx = nx - cx, dy = ny - cy, dz = nz - cz;
    const double r2 = dx * dx + dy * dy;         // the first two terms of moveout_dist's sum
    const double adz = fabs(dz);
    R = moveout_dist(nx, ny, nz, cx, cy, cz);
    if (r2 > 0.0) {
        const double inv = 1.0 / (R * c0);
        g0 = dx * inv;
        g1 = dy * inv;
        g2 = adz * inv;
    } else if (adz > 0.0) {                      // directly above or below the channel: ph = 0, th = pi / 2
        g0 = kLocCosHalfPi / c0;
        g1 = 0.0;
        g2 = 1.0 / c0;
    } else {                                     // on the channel: ph = 0, th = 0
        g0 = 1.0 / c0;
        g1 = 0.0;
        g2 = 0.0;
    }
}

// x = A^-1 b for a symmetric positive definite A (upper triangle given row by row) by Cholesky; NaN when A is not
template <int NP>
__device__ __forceinline__ void loc_solve_spd(const double* a_upper, const double* b, double* x) {
    double A[NP][NP], L[NP][NP], y[NP];
    int q = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int k = i; k < NP; ++k) {
            A[i][k] = a_upper[q];
            A[k][i] = a_upper[q];
            ++q;
        }
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int k = 0; k <= i; ++k) {
            double s = A[i][k];
#pragma unroll
            for (int m = 0; m < k; ++m) s -= L[i][m] * L[k][m];
            L[i][k] = (i == k) ? sqrt(s) : s / L[k][k];
        }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        double s = b[i];
#pragma unroll
        for (int m = 0; m < i; ++m) s -= L[i][m] * y[m];
        y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = NP - 1; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int m = i + 1; m < NP; ++m) s -= L[m][i] * x[m];
        x[i] = s / L[i][i];
    }
}

}  // namespace d4w
