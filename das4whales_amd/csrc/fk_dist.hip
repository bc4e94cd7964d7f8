// =============================================================================================
// Distributed f-k filter (one channel block per GPU): pencil decomposition with ONE exchange each
// way.  The packed 2-D transform factorises per axis, so the five passes regroup as
//   time phase   (local rows)        : n1 sub-FFT + four-step twiddle (pass A with C1 = 1), then the
//                                      contiguous n2 sub-FFT of every sub-row            [fkd_rows_n2]
//   all-to-all                       : re-shard by n1-position q1 (sub-rows of N2 bins); a q1 and its
//                                      Hermitian partner q1' always travel to the same rank
//   channel phase (all nx channels   : c1 sub-FFT + twiddle (pass A with N1 = 1), c2 sub-FFT (pass C),
//                  of the owned q1s)   real-spectrum pair op x folded mask                [fkd_pair_slab],
//                                      inverse c2, inverse c1 (x 1/(nx M))
//   all-to-all back, inverse time phase.
// The generic pass kernels are reused unchanged through two FkDev descriptors with a degenerate
// axis each.  Host plumbing (pack, RCCL all_to_all_single, unpack) lives in das4whales_amd/shard.py.
// =============================================================================================
#include <cstdlib>
#include <cstring>
#include <cmath>

#include "fk_plan.h"

namespace d4w {

// contiguous n2 sub-FFT of every sub-row (forward: natural -> digit-reversed; inverse: back)
template <bool INV, bool GENERIC>
__global__ __launch_bounds__(kMaxThreads) void fkd_rows_n2(FkDev P, float2* __restrict__ data, int nsub) {
    D4W_DYN_LDS(smem_raw);
    float2* tile = reinterpret_cast<float2*>(smem_raw);
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int N2 = P.d.N2;
    const TwLds tw = tw_stage(P.ax_n2, tile + N2, tid, nthr);
    for (int t = blockIdx.x; t < nsub; t += gridDim.x) {
        float2* row = data + (size_t)t * N2;
        for (int w = tid; w < N2; w += nthr) tile[w] = row[w];
        lds_barrier();
        lds_fft<INV, false, GENERIC>(tile, P.ax_n2, tw, 1, 1, 0, 1, 0, tid, nthr);
        for (int w = tid; w < N2; w += nthr) row[w] = tile[w];
        lds_barrier();
    }
}

// pair op of fk_passB on the slab layout (see the algebra there); one thread per Hermitian pair
__global__ __launch_bounds__(kThreads) void fkd_pair_slab(FkdSlab S, float2* __restrict__ slab) {
    const int jq = blockIdx.z, r = blockIdx.y;
    const int rp = S.hilbert ? r : S.row_partner[r], jp = S.jq_partner[jq];
    const long keyA = (long)r * S.nq + jq, keyB = (long)rp * S.nq + jp;
    if (keyB < keyA) return;
    const bool same = (keyA == keyB);
    const bool k1zero = (S.q1_of[jq] == 0);
    float2* A = slab + (size_t)keyA * S.N2;
    float2* B = slab + (size_t)keyB * S.N2;
    const float* mA = S.hilbert ? nullptr : S.mask + (size_t)keyA * S.N2;
    const float* mB = S.hilbert ? nullptr : S.mask + (size_t)keyB * S.N2;
    const float2 wr = S.wrow[S.q1_of[jq]];
    const float nyq = S.hilbert ? 0.f : S.nyq[r];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < S.N2; i += gridDim.x * blockDim.x) {
        const int j = k1zero ? S.mirror0[i] : (S.N2 - 1 - i);
        if (same && j < i) continue;
        const float2 a = A[i];
        const float2 Bc = c_conj(B[j]);
        const float2 w = c_mul(wr, S.wcol[i]);
        const float2 E = c_scale(c_add(a, Bc), 0.5f);
        const float2 O = c_mul_mi(c_scale(c_sub(a, Bc), 0.5f));
        const float2 tO = c_mul(w, O);
        float2 Yp, Ym;
        if (S.hilbert) {
            // spectrum of the Hilbert transform: -i X(f) for 0 < f < M, +i X(f) for the negative
            // frequencies f + M, zero at DC and Nyquist (scipy's h = 1 there belongs to the real part)
            const bool dc = k1zero && i == 0;
            Yp = dc ? make_float2(0.f, 0.f) : c_mul_mi(c_add(E, tO));
            Ym = dc ? make_float2(0.f, 0.f) : c_mul_pi(c_sub(E, tO));
        } else {
            const float ma = mA[i];
            const float mb = (k1zero && i == 0) ? nyq : mB[j];
            Yp = c_scale(c_add(E, tO), ma);
            Ym = c_scale(c_sub(E, tO), mb);
        }
        const float2 Sm = c_scale(c_add(Yp, Ym), 0.5f);
        const float2 D = c_mul_pi(c_mulc(c_scale(c_sub(Yp, Ym), 0.5f), w));
        A[i] = c_add(Sm, D);
        B[j] = c_conj(c_sub(Sm, D));
    }
}

// ---------------------------------------------------------------------------------------------
// Channel transform of ANY length (a channel count with a prime factor > 31) as a Bluestein convolution in global
// memory: column by column,
//   a[n] = z[n] w[n] (n < nx, zero up to L = 2^a 3^b 5^c >= 2 nx - 1),  A = FFT_L(a),  A *= FFT_L(conj w, wrapped) / L,
//   c = IFFT_L(A),  Z[k] = w[k] c[k] (k < nx),  w[n] = exp(-i pi n^2 / nx);  the inverse conjugates w and the filter.
// The two length-L transforms are passes A and C of the generic kernels on a scratch [L][Wc] (a chunk of Wc slab columns
// at a time) with the elementwise steps folded into them: three launches per direction, 5 sweeps of the scratch.  Rows come
// out in natural wavenumber order.  Tiles and pipelining as fk_passA_fwd / fk_passC / fk_passA_inv with N1 = 1.
// ---------------------------------------------------------------------------------------------
//   fkd_bz_passA_fwd : slab rows x chirp (zero beyond nx / beyond the chunk's columns) -> c1 transform, x W_L -> scratch
//   fkd_bz_passC     : c2 transform, x filter at the row position, inverse c2 transform, in place on the scratch
//   fkd_bz_passA_inv : x conj W_L, inverse c1 transform, x chirp x scale -> slab rows < nx
struct FkdBz {
    const float2* chirp;      // [nx]
    const float2* filt;       // [L] at row positions
    size_t pitch;             // slab row pitch (complex)
    int nx, ncol, inv;        // rows of the slab, valid columns of this chunk, 1: conjugated tables
    float scale;
    const int* cols;          // NULL: scratch column t = slab column t; else slab column cols[t] (the live columns, below)
};

template <bool GENERIC>
__global__ __launch_bounds__(kMaxThreads) void fkd_bz_passA_fwd(FkDev P, FkdBz Z, const float2* __restrict__ slab,
                                                                float2* __restrict__ S, int ntiles) {
    D4W_DYN_LDS(smem_raw);
    float2* tile = reinterpret_cast<float2*>(smem_raw);
    const FkDims& d = P.d;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int TA = d.TA;
    const int nelem = d.C1 * TA;
    const int ntx = (d.N2 + TA - 1) / TA;
    const FDiv dTA(TA), dntx(ntx);
    const TwLds tw_c1 = tw_stage(P.ax_c1, tile + nelem, tid, nthr);
    float2 pf[kPF];
    auto issue = [&](int t) {
        const int c2 = dntx.div(t), b0 = (t - c2 * ntx) * TA;
#pragma unroll
        for (int it = 0; it < kPF; ++it) {
            const int w = tid + it * nthr;
            float2 v = make_float2(0.f, 0.f);
            if (w < nelem) {
                const int c1 = dTA.div(w), tt = w - c1 * TA;
                const int row = c1 * d.C2 + c2, col = b0 + tt;
                if (row < Z.nx && col < Z.ncol) {
                    float2 ch = Z.chirp[row];
                    if (Z.inv) ch.y = -ch.y;
                    v = c_mul(slab[(size_t)row * Z.pitch + (Z.cols ? Z.cols[col] : col)], ch);
                }
            }
            pf[it] = v;
        }
    };
    int t = blockIdx.x;
    if (t < ntiles) issue(t);
    while (t < ntiles) {
#pragma unroll
        for (int it = 0; it < kPF; ++it) {
            const int w = tid + it * nthr;
            if (w < nelem) tile[w] = pf[it];
        }
        lds_barrier();
        const int next = t + gridDim.x;
        if (next < ntiles) issue(next);
        lds_fft<false, true, GENERIC>(tile, P.ax_c1, tw_c1, TA, TA, 1, 1, 0, tid, nthr);
        const int c2 = dntx.div(t), b0 = (t - c2 * ntx) * TA;
        const int ncol = min(TA, d.N2 - b0);
        for (int w = tid; w < nelem; w += nthr) {
            const int q = dTA.div(w), tt = w - q * TA;
            if (tt < ncol) {
                const size_t row = (size_t)q * d.C2 + c2;
                S[row * d.M + b0 + tt] = c_mul(tile[w], P.twc[q * d.C2 + c2]);
            }
        }
        lds_barrier();
        t = next;
    }
}

template <bool GENERIC>
__global__ __launch_bounds__(kMaxThreads) void fkd_bz_passA_inv(FkDev P, FkdBz Z, const float2* __restrict__ S,
                                                                float2* __restrict__ slab, int ntiles) {
    D4W_DYN_LDS(smem_raw);
    float2* tile = reinterpret_cast<float2*>(smem_raw);
    const FkDims& d = P.d;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int TA = d.TA;
    const int nelem = d.C1 * TA;
    const int ntx = (d.N2 + TA - 1) / TA;
    const FDiv dTA(TA), dntx(ntx);
    const TwLds tw_c1 = tw_stage(P.ax_c1, tile + nelem, tid, nthr);
    float2 pf[kPF];
    auto issue = [&](int t) {
        const int c2 = dntx.div(t), b0 = (t - c2 * ntx) * TA;
        const int ncol = min(TA, d.N2 - b0);
#pragma unroll
        for (int it = 0; it < kPF; ++it) {
            const int w = tid + it * nthr;
            float2 v = make_float2(0.f, 0.f);
            if (w < nelem) {
                const int q = dTA.div(w), tt = w - q * TA;
                if (tt < ncol) v = S[((size_t)q * d.C2 + c2) * d.M + b0 + tt];
            }
            pf[it] = v;
        }
    };
    int t = blockIdx.x;
    if (t < ntiles) issue(t);
    while (t < ntiles) {
        const int c2 = dntx.div(t), b0 = (t - c2 * ntx) * TA;
#pragma unroll
        for (int it = 0; it < kPF; ++it) {
            const int w = tid + it * nthr;
            if (w < nelem) {
                const int q = dTA.div(w);
                tile[w] = c_mulc(pf[it], P.twc[q * d.C2 + c2]);
            }
        }
        lds_barrier();
        const int next = t + gridDim.x;
        if (next < ntiles) issue(next);
        lds_fft<true, true, GENERIC>(tile, P.ax_c1, tw_c1, TA, TA, 1, 1, 0, tid, nthr);
        for (int w = tid; w < nelem; w += nthr) {
            const int c1 = dTA.div(w), tt = w - c1 * TA;
            const int row = c1 * d.C2 + c2, col = b0 + tt;
            if (row < Z.nx && col < Z.ncol) {
                float2 ch = Z.chirp[row];
                if (Z.inv) ch.y = -ch.y;
                slab[(size_t)row * Z.pitch + (Z.cols ? Z.cols[col] : col)] = c_mul(tile[w], c_scale(ch, Z.scale));
            }
        }
        lds_barrier();
        t = next;
    }
}

template <bool GENERIC>
__global__ __launch_bounds__(kMaxThreads) void fkd_bz_passC(FkDev P, FkdBz Z, float2* __restrict__ S, int ntiles) {
    D4W_DYN_LDS(smem_raw);
    float2* tile = reinterpret_cast<float2*>(smem_raw);
    const FkDims& d = P.d;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int TC = d.TC;
    const int nelem = d.C2 * TC;
    const int ntx = (d.M + TC - 1) / TC;
    const FDiv dTC(TC), dntx(ntx);
    const TwLds tw = tw_stage(P.ax_c2, tile + nelem, tid, nthr);
    float2 pf[kPF];
    auto issue = [&](int t) {
        const int q = dntx.div(t), p0 = (t - q * ntx) * TC;
        const int ncol = min(TC, d.M - p0);
        const float2* base = S + ((size_t)q * d.C2) * d.M + p0;
#pragma unroll
        for (int it = 0; it < kPF; ++it) {
            const int w = tid + it * nthr;
            float2 v = make_float2(0.f, 0.f);
            if (w < nelem) {
                const int c2 = dTC.div(w), tt = w - c2 * TC;
                if (tt < ncol) v = base[(size_t)c2 * d.M + tt];
            }
            pf[it] = v;
        }
    };
    int t = blockIdx.x;
    if (t < ntiles) issue(t);
    while (t < ntiles) {
#pragma unroll
        for (int it = 0; it < kPF; ++it) {
            const int w = tid + it * nthr;
            if (w < nelem) tile[w] = pf[it];
        }
        lds_barrier();
        const int next = t + gridDim.x;
        if (next < ntiles) issue(next);
        lds_fft<false, true, GENERIC>(tile, P.ax_c2, tw, TC, TC, 1, 1, 0, tid, nthr);
        const int q = dntx.div(t), p0 = (t - q * ntx) * TC;
        for (int w = tid; w < nelem; w += nthr) {
            float2 f = Z.filt[q * d.C2 + dTC.div(w)];
            if (Z.inv) f.y = -f.y;
            tile[w] = c_mul(tile[w], f);
        }
        lds_barrier();
        lds_fft<true, true, GENERIC>(tile, P.ax_c2, tw, TC, TC, 1, 1, 0, tid, nthr);
        const int ncol = min(TC, d.M - p0);
        float2* base = S + ((size_t)q * d.C2) * d.M + p0;
        for (int w = tid; w < nelem; w += nthr) {
            const int c2 = dTC.div(w), tt = w - c2 * TC;
            if (tt < ncol) base[(size_t)c2 * d.M + tt] = tile[w];
        }
        lds_barrier();
        t = next;
    }
}

// The time transform of the packed rows (length M = ns / 2 with a prime factor > 31) the same way, row by row: a chunk
// of rows in a scratch [R][L], L = 2^a 3^b 5^c >= 2 M - 1, and per direction
//   fkd_bt_passA_fwd : row x (window) x chirp, zero beyond M -> n1 transform, x W_L -> scratch   (fk_passA_fwd, C1 = 1)
//   fkd_bt_rows      : n2 transform, x filter at the position, inverse n2 transform             (fkd_rows_n2 twice)
//   fkd_bt_passA_inv : x conj W_L, inverse n1 transform, x chirp x scale -> the row's first M elements
struct FkdBt {
    const float2* chirp;      // [M]
    const float2* filt;       // [L] at positions [q1][i]
    const float2* win;        // [M] packed window, or NULL
    size_t pitch;             // row pitch of the rows outside the scratch (complex) = M
    int m, inv;               // M; 1: conjugated tables
    float scale;
};

template <bool GENERIC>
__global__ __launch_bounds__(kMaxThreads) void fkd_bt_passA_fwd(FkDev P, FkdBt Z, const float2* __restrict__ rows,
                                                                float2* __restrict__ S, int ntiles) {
    D4W_DYN_LDS(smem_raw);
    float2* tile = reinterpret_cast<float2*>(smem_raw);
    const FkDims& d = P.d;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int TA = d.TA;
    const int nelem = d.N1 * TA;
    const int ntx = (d.N2 + TA - 1) / TA;
    const FDiv dTA(TA), dntx(ntx);
    const TwLds tw_n1 = tw_stage(P.ax_n1, tile + nelem, tid, nthr);
    float2 pf[kPF];
    auto issue = [&](int t) {
        const int row = dntx.div(t), b0 = (t - row * ntx) * TA;
        const int ncol = min(TA, d.N2 - b0);
#pragma unroll
        for (int it = 0; it < kPF; ++it) {
            const int w = tid + it * nthr;
            float2 v = make_float2(0.f, 0.f);
            if (w < nelem) {
                const int n1 = dTA.div(w), tt = w - n1 * TA;
                const int col = n1 * d.N2 + b0 + tt;
                if (tt < ncol && col < Z.m) {
                    v = rows[(size_t)row * Z.pitch + col];
                    if (Z.win) {
                        const float2 wv = Z.win[col];
                        v.x *= wv.x;
                        v.y *= wv.y;
                    }
                    float2 ch = Z.chirp[col];
                    if (Z.inv) ch.y = -ch.y;
                    v = c_mul(v, ch);
                }
            }
            pf[it] = v;
        }
    };
    int t = blockIdx.x;
    if (t < ntiles) issue(t);
    while (t < ntiles) {
#pragma unroll
        for (int it = 0; it < kPF; ++it) {
            const int w = tid + it * nthr;
            if (w < nelem) tile[w] = pf[it];
        }
        lds_barrier();
        const int next = t + gridDim.x;
        if (next < ntiles) issue(next);
        lds_fft<false, true, GENERIC>(tile, P.ax_n1, tw_n1, TA, TA, 1, 1, d.N1 * TA, tid, nthr);
        const int row = dntx.div(t), b0 = (t - row * ntx) * TA;
        const int ncol = min(TA, d.N2 - b0);
        for (int w = tid; w < nelem; w += nthr) {
            const int q1 = dTA.div(w), tt = w - q1 * TA;
            if (tt < ncol) S[(size_t)row * d.M + q1 * d.N2 + b0 + tt] = c_mul(tile[w], P.twt[q1 * d.N2 + b0 + tt]);
        }
        lds_barrier();
        t = next;
    }
}

template <bool GENERIC>
__global__ __launch_bounds__(kMaxThreads) void fkd_bt_passA_inv(FkDev P, FkdBt Z, const float2* __restrict__ S,
                                                                float2* __restrict__ rows, int ntiles) {
    D4W_DYN_LDS(smem_raw);
    float2* tile = reinterpret_cast<float2*>(smem_raw);
    const FkDims& d = P.d;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int TA = d.TA;
    const int nelem = d.N1 * TA;
    const int ntx = (d.N2 + TA - 1) / TA;
    const FDiv dTA(TA), dntx(ntx);
    const TwLds tw_n1 = tw_stage(P.ax_n1, tile + nelem, tid, nthr);
    float2 pf[kPF];
    auto issue = [&](int t) {
        const int row = dntx.div(t), b0 = (t - row * ntx) * TA;
        const int ncol = min(TA, d.N2 - b0);
#pragma unroll
        for (int it = 0; it < kPF; ++it) {
            const int w = tid + it * nthr;
            float2 v = make_float2(0.f, 0.f);
            if (w < nelem) {
                const int q1 = dTA.div(w), tt = w - q1 * TA;
                if (tt < ncol) v = S[(size_t)row * d.M + q1 * d.N2 + b0 + tt];
            }
            pf[it] = v;
        }
    };
    int t = blockIdx.x;
    if (t < ntiles) issue(t);
    while (t < ntiles) {
        const int row = dntx.div(t), b0 = (t - row * ntx) * TA;
        const int ncol = min(TA, d.N2 - b0);
#pragma unroll
        for (int it = 0; it < kPF; ++it) {
            const int w = tid + it * nthr;
            if (w < nelem) {
                const int q1 = dTA.div(w), tt = w - q1 * TA;
                float2 v = pf[it];
                if (tt < ncol) v = c_mulc(v, P.twt[q1 * d.N2 + b0 + tt]);
                tile[w] = v;
            }
        }
        lds_barrier();
        const int next = t + gridDim.x;
        if (next < ntiles) issue(next);
        lds_fft<true, true, GENERIC>(tile, P.ax_n1, tw_n1, TA, TA, 1, 1, d.N1 * TA, tid, nthr);
        for (int w = tid; w < nelem; w += nthr) {
            const int n1 = dTA.div(w), tt = w - n1 * TA;
            const int col = n1 * d.N2 + b0 + tt;
            if (tt < ncol && col < Z.m) {
                float2 ch = Z.chirp[col];
                if (Z.inv) ch.y = -ch.y;
                rows[(size_t)row * Z.pitch + col] = c_mul(tile[w], c_scale(ch, Z.scale));
            }
        }
        lds_barrier();
        t = next;
    }
}

template <bool GENERIC>
__global__ __launch_bounds__(kMaxThreads) void fkd_bt_rows(FkDev P, FkdBt Z, float2* __restrict__ S, int nsub) {
    D4W_DYN_LDS(smem_raw);
    float2* tile = reinterpret_cast<float2*>(smem_raw);
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int N2 = P.d.N2, N1 = P.d.N1;
    const TwLds tw = tw_stage(P.ax_n2, tile + N2, tid, nthr);
    for (int t = blockIdx.x; t < nsub; t += gridDim.x) {
        float2* row = S + (size_t)t * N2;
        const float2* f = Z.filt + (size_t)(t % N1) * N2;
        for (int w = tid; w < N2; w += nthr) tile[w] = row[w];
        lds_barrier();
        lds_fft<false, false, GENERIC>(tile, P.ax_n2, tw, 1, 1, 0, 1, 0, tid, nthr);
        for (int w = tid; w < N2; w += nthr) {
            float2 fv = f[w];
            if (Z.inv) fv.y = -fv.y;
            tile[w] = c_mul(tile[w], fv);
        }
        lds_barrier();
        lds_fft<true, false, GENERIC>(tile, P.ax_n2, tw, 1, 1, 0, 1, 0, tid, nthr);
        for (int w = tid; w < N2; w += nthr) row[w] = tile[w];
        lds_barrier();
    }
}

// folded mask of the owned sub-rows (fk_fold_mask restricted to a q1 subset)
__global__ __launch_bounds__(kThreads) void fkd_fold_mask(int nx, int ns, int N1, int N2, int nq,
                                                           const float* __restrict__ ms,
                                                           const int* __restrict__ rowk,
                                                           const int* __restrict__ q1_of,
                                                           const int* __restrict__ k1_of_q1,
                                                           const int* __restrict__ k2_of_i,
                                                           float* __restrict__ mask, float* __restrict__ nyq, FkAffine aff) {
    const int r = blockIdx.y;
    const int k = rowk[r];
    const int km = (nx - k) % nx;
    const int sx = nx / 2, st = ns / 2, M = ns / 2;
    const size_t rowp = (size_t)((k + sx) % nx) * ns;
    const size_t rowm = (size_t)((km + sx) % nx) * ns;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < nq * N2; p += gridDim.x * blockDim.x) {
        const int jq = p / N2, i = p - jq * N2;
        const int f = k1_of_q1[q1_of[jq]] + N1 * k2_of_i[i];
        const int fm = (ns - f) % ns;
        mask[(size_t)r * nq * N2 + p] = 0.5f * (aff(ms[rowp + (f + st) % ns]) + aff(ms[rowm + (fm + st) % ns]));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        nyq[r] = 0.5f * (aff(ms[rowp + (M + st) % ns]) + aff(ms[rowm + ((ns - M) + st) % ns]));
}

// ... evaluated in closed form instead of read (fk_fold_design restricted to a q1 subset): a rank never holds the
// dense mask, only the gains of the sub-rows it owns
__global__ __launch_bounds__(kThreads) void fkd_fold_design(int nx, int ns, int N1, int N2, int nq, DesignArgs A, int mode,
                                                             const int* __restrict__ rowk,
                                                             const int* __restrict__ q1_of,
                                                             const int* __restrict__ k1_of_q1,
                                                             const int* __restrict__ k2_of_i,
                                                             float* __restrict__ mask, float* __restrict__ nyq) {
    const int r = blockIdx.y;
    const int k = rowk[r];
    const int km = (nx - k) % nx;
    const int sx = nx / 2, st = ns / 2, M = ns / 2;
    const int ip = (k + sx) % nx, im = (km + sx) % nx;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < nq * N2; p += gridDim.x * blockDim.x) {
        const int jq = p / N2, i = p - jq * N2;
        const int f = k1_of_q1[q1_of[jq]] + N1 * k2_of_i[i];
        const int fm = (ns - f) % ns;
        mask[(size_t)r * nq * N2 + p] = design_folded(A, mode, ip, (f + st) % ns, im, (fm + st) % ns);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        nyq[r] = design_folded(A, mode, ip, (M + st) % ns, im, ((ns - M) + st) % ns);
}

// bit pattern of max |mask| over the owned sub-rows of every row position (slab mask [nx][W]) and its Nyquist gain
// (C linkage: the kernel's name in the code object has always been the plain `fkd_row_max`, and stays so)
extern "C" __global__ __launch_bounds__(kThreads) void fkd_row_max(const float* __restrict__ mask, const float* __restrict__ nyq,
                                                                    int W, unsigned* __restrict__ rowmaxbits) {
    const int r = blockIdx.x;
    unsigned vb = (threadIdx.x == 0) ? (__float_as_uint(nyq[r]) & 0x7fffffffu) : 0u;
    for (int p = threadIdx.x; p < W; p += blockDim.x) vb = max(vb, __float_as_uint(mask[(size_t)r * W + p]) & 0x7fffffffu);
    for (int off = 32; off >= 1; off >>= 1) vb = max(vb, __shfl_xor(vb, off));
    if ((threadIdx.x & 63) == 0 && vb) atomicMax(rowmaxbits + r, vb);
}

// colmax[c] = max over the rows of |folded gain| at slab column c, as the bits of a non-negative float (NaN: +inf)
__global__ __launch_bounds__(kThreads) void fkd_col_max(const float* __restrict__ mask, int nx, int W,
                                                        unsigned* __restrict__ colmax) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= W) return;
    float m = 0.f;
    for (int r = blockIdx.y; r < nx; r += gridDim.y) {
        const float g = fabsf(mask[(size_t)r * W + c]);
        m = (g != g) ? INFINITY : fmaxf(m, g);
    }
    atomicMax(&colmax[c], __float_as_uint(m));
}
// the gains of the columns that are not transformed become exact zeros (they are below fk_zero_gain, the level the
// specialised plans drop as well)
__global__ __launch_bounds__(kThreads) void fkd_zero_dead_cols(float* __restrict__ mask, int nx, int W,
                                                               const unsigned* __restrict__ live) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= W || live[c]) return;
    for (int r = blockIdx.y; r < nx; r += gridDim.y) mask[(size_t)r * W + c] = 0.f;
}

// host launchers: the picks of an instantiation, and the pair op for analytic_long.hip (fk_plan.h)
static int fkd_launch_rows_n2(bool inv, bool generic, dim3 grid, dim3 blk, size_t lds, void* stream, const FkDev& P,
                              float2* data, int nsub) {
    auto k = inv ? (generic ? fkd_rows_n2<true, true> : fkd_rows_n2<true, false>)
                 : (generic ? fkd_rows_n2<false, true> : fkd_rows_n2<false, false>);
    return launch_k(k, grid, blk, lds, stream, P, data, nsub);
}

int fkd_launch_pair_slab(const FkdSlab& S, float2* slab, void* stream) {
    return launch_k(fkd_pair_slab, dim3(std::min(ceil_div(S.N2, kThreads), 8), S.nx, S.nq), dim3(kThreads), 0, stream, S, slab);
}

}  // namespace d4w

using namespace d4w;

static void fkd_block(int nx, int world, int r, int* a, int* b) {
    const int base = nx / world, extra = nx % world;
    *a = r * base + std::min(r, extra);
    *b = *a + base + (r < extra ? 1 : 0);
}

extern "C" {

int d4w_fkd_plan_destroy(d4w_fkd_plan* pl) {
    if (!pl) return D4W_OK;
    fk_plan_release(&pl->tp);
    fk_plan_release(&pl->cp);
    if (pl->sp) d4w_fk_plan_destroy(pl->sp);
    delete pl;
    return D4W_OK;
}

}  // extern "C"

// Packed path of the distributed plan: shapes with specialised kernels (fk_fast.h).  Returns D4W_EINVAL (and leaves
// *out NULL) when the shape has none -- the caller then builds the generic plan.
int d4w::fkd_plan_build_packed(int nx, int ns, int world, int rank, bool want_mask, d4w_fkd_plan** out, bool time_only) {
    *out = nullptr;
    const char* g = getenv("D4W_FKD_GENERIC");
    if (g && atoi(g) > 0) return fail(D4W_EINVAL, "generic distributed plan requested");
    d4w_fk_plan* sp = nullptr;
    int rc = fk_plan_build(nx, ns, nullptr, false, true, &sp);
    if (rc) return rc;
    const FkFastEntry& F = *sp->fast;
    // (time_only: only the time phase and pass B are used -- the analytic signal of long rows -- and the channel-phase
    // constraints do not apply)
    if (!time_only && (F.C2X > 1 || F.TA != F.TC || (F.NA * F.NB * F.NC) % (F.N1 * F.TA) != 0)) {     // pass A MODE 2 walks N1 adjacent strips inside a sub-row
        d4w_fk_plan_destroy(sp);
        return fail(D4W_EINVAL, "shape config not usable for the packed distributed plan");
    }
    d4w_fkd_plan* pl = new d4w_fkd_plan();
    pl->sp = sp;
    const FkDims& d = sp->dev.d;
    pl->nx = nx; pl->ns = ns; pl->M = d.M; pl->world = world; pl->rank = rank;
    fkd_block(nx, world, rank, &pl->row_begin, &pl->row_end);
    pl->N1 = d.N1; pl->N2 = d.N2; pl->C1 = d.C1; pl->C2 = d.C2; pl->TA_t = d.TA; pl->TA_c = d.TA; pl->TC = d.TC;
    pl->num_cu = sp->num_cu;
    const int N1 = d.N1, N2 = d.N2, nxl = pl->row_end - pl->row_begin;
    // ownership of the n1-positions (single radix: position = frequency digit): Hermitian classes {q1, N1 - q1} dealt
    // to the least loaded rank
    pl->owner.assign(N1, -1);
    {
        std::vector<int> load(world, 0);
        for (int q1 = 0; q1 < N1; ++q1) {
            if (pl->owner[q1] >= 0) continue;
            int best = 0;
            for (int r = 1; r < world; ++r) if (load[r] < load[best]) best = r;
            const int qp = (N1 - q1) % N1;
            pl->owner[q1] = best; ++load[best];
            if (qp != q1) { pl->owner[qp] = best; ++load[best]; }
        }
    }
    std::vector<int> nq_of(world, 0), jq_of(N1, 0);
    for (int q1 = 0; q1 < N1; ++q1) jq_of[q1] = nq_of[pl->owner[q1]]++;
    for (int q1 = 0; q1 < N1; ++q1) if (pl->owner[q1] == rank) pl->myq.push_back(q1);
    const int nq = (int)pl->myq.size();
    const long W = (long)std::max(nq, 1) * N2;
    if ((long)nx * W >= (1L << 31) || (long)nxl * d.M >= (1L << 31)) {
        d4w_fkd_plan_destroy(pl);
        return fail(D4W_EINVAL, "block too large for 32-bit element offsets");
    }
    // packed buffer layout of THIS rank's local rows
    std::vector<int> qoff(N1), qpitch(N1);
    {
        std::vector<long> blk(world + 1, 0);
        for (int sr = 0; sr < world; ++sr) blk[sr + 1] = blk[sr] + (long)nxl * nq_of[sr] * N2;
        for (int q1 = 0; q1 < N1; ++q1) {
            const int o = pl->owner[q1];
            qoff[q1] = (int)(blk[o] + (long)jq_of[q1] * N2);
            qpitch[q1] = nq_of[o] * N2;
        }
    }
    std::vector<int> myq = pl->myq;
    if (myq.empty()) myq.push_back(0);
    const int *c_qoff, *c_qpitch, *c_q1of;
#define D4W_TRY(x) do { rc = (x); if (rc != D4W_OK) { d4w_fkd_plan_destroy(pl); return rc; } } while (0)
    D4W_TRY(upload(sp, qoff, &c_qoff));
    D4W_TRY(upload(sp, qpitch, &c_qpitch));
    D4W_TRY(upload(sp, myq, &c_q1of));
    pl->d_q1of = const_cast<int*>(c_q1of);
    pl->geo_t = FkGeo{nxl, d.M, nq, c_qoff, c_qpitch, c_q1of};
    pl->geo_c = FkGeo{nx, (int)W, (int)(W / d.TC), c_qoff, c_qpitch, c_q1of};     // pass C: nq = column blocks per row
    pl->dev_t = sp->dev;
    pl->dev_t.scale = 1.0f;
    pl->dev_c = sp->dev;
    // pass-B work list in slab keys
    std::vector<int> jq_mine(N1, -1);
    for (int j = 0; j < nq; ++j) jq_mine[pl->myq[j]] = j;
    for (const int2& pr : sp->h_pairs) {
        const int ra = pr.x / N1, qa = pr.x % N1, rb = pr.y / N1, qb = pr.y % N1;
        if (jq_mine[qa] < 0) continue;
        pl->h_pairs_slab.push_back(make_int2(ra * nq + jq_mine[qa], rb * nq + jq_mine[qb]));
    }
    {
        const int2* c_pairs;
        D4W_TRY(upload(sp, pl->h_pairs_slab, &c_pairs));
        pl->d_pairs_slab = const_cast<int2*>(c_pairs);
        void* q = nullptr;
        if (hipMalloc(&q, std::max<size_t>(pl->h_pairs_slab.size(), 1) * sizeof(int2)) != hipSuccess) { d4w_fkd_plan_destroy(pl); return fail(D4W_ENOMEM, "hipMalloc failed"); }
        sp->allocs.push_back(q); pl->d_pairs_live = (int2*)q;
        if (hipMalloc(&q, (size_t)d.C1 * F.C2A * sizeof(unsigned)) != hipSuccess) { d4w_fkd_plan_destroy(pl); return fail(D4W_ENOMEM, "hipMalloc failed"); }
        sp->allocs.push_back(q); pl->d_livebits = (unsigned*)q;
        if (hipMalloc(&q, (size_t)nx * sizeof(unsigned)) != hipSuccess) { d4w_fkd_plan_destroy(pl); return fail(D4W_ENOMEM, "hipMalloc failed"); }
        sp->allocs.push_back(q); pl->d_rowmax = (unsigned*)q;
    }
    pl->fdev_c = sp->fdev;
    pl->fdev_c.pairs = pl->d_pairs_slab;
    pl->fdev_c.live = nullptr;
    pl->npairs_run = (int)pl->h_pairs_slab.size();
    pl->live_rows = nx;
    if (want_mask) {
        void* q = nullptr;
        if (hipMalloc(&q, (size_t)nx * W * sizeof(float)) != hipSuccess) { d4w_fkd_plan_destroy(pl); return fail(D4W_ENOMEM, "hipMalloc of the slab mask failed"); }
        sp->allocs.push_back(q); pl->d_mask = (float*)q;
        pl->d_nyq = sp->d_nyq;
    }
    pl->dev_c.mask = pl->d_mask;
    pl->dev_c.nyq = pl->d_nyq;
#undef D4W_TRY
    *out = pl;
    return D4W_OK;
}

int d4w::fkd_plan_build(int nx, int ns, int world, int rank, bool want_mask, d4w_fkd_plan** out) {
    if (!out) return fail(D4W_EINVAL, "plan pointer is NULL");
    *out = nullptr;
    if (nx < 1 || ns < 2 || (ns & 1)) return fail(D4W_EINVAL, "bad shape %d x %d (ns must be even)", nx, ns);
    if (world < 1 || rank < 0 || rank >= world || world > nx) return fail(D4W_EINVAL, "bad world %d / rank %d", world, rank);
    if (want_mask && fkd_plan_build_packed(nx, ns, world, rank, want_mask, out) == D4W_OK) return D4W_OK;
    const int M = ns / 2;
    // ns / 2 with a prime factor > 31: the time transform of the packed rows is a Bluestein convolution of length bt_L in
    // global memory (fkd_bt_*); tp describes that length and the half spectrum comes out in natural order (N1 = 1)
    const int bt_L = (rough_part(M) > 1) ? smooth_len_235(2L * M - 1) : 0;
    const int Mt = bt_L ? bt_L : M;
    // time axis Mt = tN1 * tN2: tN2 in one LDS row, and enough n1-positions (Hermitian classes) to balance the ranks
    int tN1 = 0;
    for (int cand = 1; cand <= Mt; ++cand) {
        if (Mt % cand) continue;
        if (Mt / cand > kMaxTile / 2) continue;
        if (tN1 == 0) tN1 = cand;                            // smallest admissible
        if (cand >= 4 * (bt_L ? 1 : world) && cand <= 512) { tN1 = cand; break; }
        if (cand > 512) break;
    }
    if (tN1 == 0) return fail(D4W_EINVAL, "ns/2 = %d has no factorisation with N2 <= %d", M, kMaxTile / 2);
    const int tN2 = Mt / tN1;
    const int N1 = bt_L ? 1 : tN1, N2 = bt_L ? M : tN2;      // layout of the half spectrum: [row][N1][N2]
    // a channel count with a prime factor > 31: the channel transform is a Bluestein convolution of length bz_L = 2^a 3^b 5^c
    // in global memory (fkd_bz_*), and the channel-phase descriptor below is the one of that length
    // (D4W_FKD_BZ_MINPRIME = p: also channel counts with a prime factor >= p, whose loop-based radix stages are slow)
    auto largest_prime = [](int n) {
        int lp = 1;
        for (int p = 2; (long)p * p <= n; ++p)
            while (n % p == 0) { lp = p; n /= p; }
        return std::max(lp, n);
    };
    static const int bz_minprime = [] { const char* v = getenv("D4W_FKD_BZ_MINPRIME"); return (v && atoi(v) > 1) ? atoi(v) : 32; }();
    const int bz_L = (want_mask && largest_prime(nx) >= bz_minprime) ? smooth_len_235(2L * nx - 1) : 0;
    // (no mask = the time phase only, d4w_analytic_long_f32: any row count, the channel descriptor stays a dummy)
    const int Lc = !want_mask ? 1 : (bz_L ? bz_L : nx);
    int C2 = largest_divisor_le(Lc, kMaxTile / 8);
    int C1 = Lc / C2;
    if (C1 > kMaxTile) return fail(D4W_EINVAL, "nx = %d does not factor into C1 <= %d, C2 <= %d", nx, kMaxTile, kMaxTile / 8);
    d4w_fkd_plan* pl = new d4w_fkd_plan();
    pl->nx = nx; pl->ns = ns; pl->M = M; pl->world = world; pl->rank = rank;
    fkd_block(nx, world, rank, &pl->row_begin, &pl->row_end);
    pl->N1 = N1; pl->N2 = N2; pl->C1 = C1; pl->C2 = C2;
    const int nxl = pl->row_end - pl->row_begin;
    int rc;
#define D4W_TRY(x) do { rc = (x); if (rc != D4W_OK) { d4w_fkd_plan_destroy(pl); return rc; } } while (0)
    // ---------------- time-phase descriptor: C1 = 1, C2 = local rows
    d4w_fk_plan& tp = pl->tp;
    memset(&tp.dev, 0, sizeof(tp.dev));
    // one degenerate axis leaves the whole LDS tile to the other: long contiguous strips
    int TA = 512;
    while (TA > 1 && ((long)tN1 * TA > kMaxTile || TA > tN2)) TA /= 2;
    if ((long)tN1 * TA > kMaxTile) { d4w_fkd_plan_destroy(pl); return fail(D4W_EINVAL, "N1 = %d exceeds the LDS tile", tN1); }
    pl->TA_t = TA;
    tp.dev.d = FkDims{nxl, 2 * Mt, Mt, 1, nxl, tN1, tN2, TA, 1};
    tp.dev.scale = 1.0f;
    std::vector<int> f_one, tf_n1, tf_n2, f_n1, f_n2, f_c1, f_c2;
    D4W_TRY(make_axis(&tp, 1, &tp.dev.ax_c1, &f_one));
    D4W_TRY(make_axis(&tp, 1, &tp.dev.ax_c2, &f_one));
    D4W_TRY(make_axis(&tp, tN1, &tp.dev.ax_n1, &tf_n1));
    D4W_TRY(make_axis(&tp, tN2, &tp.dev.ax_n2, &tf_n2));
    {
        std::vector<float2> ones((size_t)nxl, make_float2(1.f, 0.f)), twt((size_t)tN1 * tN2);
        for (int q1 = 0; q1 < tN1; ++q1)
            for (int b = 0; b < tN2; ++b) twt[(size_t)q1 * tN2 + b] = wexp((long long)b * tf_n1[q1], Mt);
        D4W_TRY(upload(&tp, ones, &tp.dev.twc));
        D4W_TRY(upload(&tp, twt, &tp.dev.twt));
        std::vector<float> win = tukey_window(ns, 0.03);
        std::vector<float2> winp(M);
        for (int m = 0; m < M; ++m) winp[m] = make_float2(win[2 * m], win[2 * m + 1]);
        D4W_TRY(upload(&tp, winp, &tp.dev.win));
        pl->bt_win = tp.dev.win;
    }
    pl->gen_t = axis_needs_generic(tp.dev.ax_n1);
    pl->gen_n2 = axis_needs_generic(tp.dev.ax_n2);
    pl->lds_t = ((size_t)tN1 * TA + 2 * kTwLo + tp.dev.ax_c1.nhi + tp.dev.ax_n1.nhi) * sizeof(float2);
    pl->lds_n2 = ((size_t)tN2 + kTwLo + tp.dev.ax_n2.nhi) * sizeof(float2);
    if (bt_L) {
        f_n1.assign(1, 0);
        f_n2.resize(M);
        for (int i = 0; i < M; ++i) f_n2[i] = i;
        std::vector<float2> chirp(M), filt(bt_L);
        std::vector<double> bre(bt_L, 0.0), bim(bt_L, 0.0);
        for (int n = 0; n < M; ++n) {
            const double ph = M_PI * (double)(((long long)n * n) % (2LL * M)) / (double)M;
            chirp[n] = make_float2((float)cos(ph), (float)-sin(ph));
            bre[n] = cos(ph); bim[n] = sin(ph);                               // conj(chirp)
            if (n) { bre[bt_L - n] = cos(ph); bim[bt_L - n] = sin(ph); }
        }
        host_dft_any(bre, bim);
        for (int q1 = 0; q1 < tN1; ++q1)
            for (int i = 0; i < tN2; ++i) {
                const int f = tf_n1[q1] + tN1 * tf_n2[i];                     // frequency at position [q1][i]
                filt[(size_t)q1 * tN2 + i] = make_float2((float)(bre[f] / bt_L), (float)(bim[f] / bt_L));
            }
        D4W_TRY(upload(&tp, chirp, &pl->bt_chirp));
        D4W_TRY(upload(&tp, filt, &pl->bt_filt));
        const char* ch = getenv("D4W_FKD_BT_CHUNK");
        const int lim = (ch && atoi(ch) > 0) ? atoi(ch) : std::max(1, (int)(((size_t)1 << 27) / (size_t)bt_L));
        const int R = std::min(nxl, lim);
        void* p = nullptr;
        if (hipMalloc(&p, (size_t)R * bt_L * sizeof(float2)) != hipSuccess) {
            d4w_fkd_plan_destroy(pl);
            return fail(D4W_ENOMEM, "hipMalloc of the Bluestein scratch (%d x %d complex) failed", R, bt_L);
        }
        tp.allocs.push_back(p);
        pl->bt_S = (float2*)p;
        pl->bt_L = bt_L; pl->bt_R = R;
    } else {
        f_n1 = tf_n1;
        f_n2 = tf_n2;
    }

    // ---------------- ownership of the n1-positions: Hermitian classes {q1, q1'} dealt round-robin
    std::vector<int> p_n1(N1), q1part(N1);
    for (int p = 0; p < N1; ++p) p_n1[f_n1[p]] = p;
    for (int q1 = 0; q1 < N1; ++q1) q1part[q1] = p_n1[(N1 - f_n1[q1]) % N1];
    pl->owner.assign(N1, -1);
    {
        std::vector<int> load(world, 0);
        for (int q1 = 0; q1 < N1; ++q1) {
            if (pl->owner[q1] >= 0) continue;
            int best = 0;
            for (int r = 1; r < world; ++r) if (load[r] < load[best]) best = r;
            pl->owner[q1] = best; ++load[best];
            if (q1part[q1] != q1) { pl->owner[q1part[q1]] = best; ++load[best]; }
        }
    }
    for (int q1 = 0; q1 < N1; ++q1) if (pl->owner[q1] == rank) pl->myq.push_back(q1);
    const int nq = (int)pl->myq.size();
    const int W = std::max(nq, 1) * N2;                       // slab width (complex columns)

    // ---------------- channel-phase descriptor: N1 = 1, "N2" = slab width
    d4w_fk_plan& cp = pl->cp;
    memset(&cp.dev, 0, sizeof(cp.dev));
    int TC = 16, TAc = 512;
    // Bluestein: the scratch [bz_L][Wc] holds a chunk of Wc slab columns at a time (<= 1 GiB; D4W_FKD_BZ_CHUNK pins Wc)
    int Wc = W;
    if (bz_L) {
        const char* ch = getenv("D4W_FKD_BZ_CHUNK");
        int lim = (ch && atoi(ch) > 0) ? atoi(ch) : std::max(16, (int)(((size_t)1 << 27) / (size_t)bz_L) & ~15);
        Wc = std::min(W, lim);
        if (Wc < W && !(ch && atoi(ch) > 0)) {
            // equal chunks: the passes sweep the scratch's full width whatever the last chunk holds
            const int nchunk = ceil_div(W, Wc);
            Wc = std::min(Wc, (ceil_div(W, nchunk) + 15) & ~15);
        }
    }
    while (TC > 1 && (long)C2 * TC > kMaxTile) TC /= 2;
    while (TAc > 1 && ((long)C1 * TAc > kMaxTile || TAc > Wc)) TAc /= 2;
    pl->TC = TC; pl->TA_c = TAc;
    cp.dev.d = FkDims{Lc, 2 * Wc, Wc, C1, C2, 1, Wc, TAc, TC};
    // Bluestein: 1 / bz_L sits in the filter table and 1 / (nx M) in fkd_bz_out of the inverse transform
    cp.dev.scale = bz_L ? 1.0f : (float)(1.0 / ((double)nx * (double)M));
    D4W_TRY(make_axis(&cp, C1, &cp.dev.ax_c1, &f_c1));
    D4W_TRY(make_axis(&cp, C2, &cp.dev.ax_c2, &f_c2));
    D4W_TRY(make_axis(&cp, 1, &cp.dev.ax_n1, &f_one));
    D4W_TRY(make_axis(&cp, 1, &cp.dev.ax_n2, &f_one));
    {
        std::vector<float2> twc((size_t)C1 * C2), ones((size_t)Wc, make_float2(1.f, 0.f));
        for (int q = 0; q < C1; ++q)
            for (int c2 = 0; c2 < C2; ++c2) twc[(size_t)q * C2 + c2] = wexp((long long)c2 * f_c1[q], Lc);
        D4W_TRY(upload(&cp, twc, &cp.dev.twc));
        D4W_TRY(upload(&cp, ones, &cp.dev.twt));
    }
    if (bz_L) {
        std::vector<float2> chirp(nx), filt(bz_L);
        std::vector<double> bre(bz_L, 0.0), bim(bz_L, 0.0);
        for (int n = 0; n < nx; ++n) {
            const double ph = M_PI * (double)(((long long)n * n) % (2LL * nx)) / (double)nx;
            chirp[n] = make_float2((float)cos(ph), (float)-sin(ph));
            bre[n] = cos(ph); bim[n] = sin(ph);                               // conj(chirp)
            if (n) { bre[bz_L - n] = cos(ph); bim[bz_L - n] = sin(ph); }
        }
        host_dft_any(bre, bim);
        for (int q = 0; q < C1; ++q)
            for (int p2 = 0; p2 < C2; ++p2) {
                const int f = f_c1[q] + C1 * f_c2[p2];                        // frequency at row position q C2 + p2
                filt[(size_t)q * C2 + p2] = make_float2((float)(bre[f] / bz_L), (float)(bim[f] / bz_L));
            }
        D4W_TRY(upload(&cp, chirp, &pl->bz_chirp));
        D4W_TRY(upload(&cp, filt, &pl->bz_filt));
        void* p = nullptr;
        if (hipMalloc(&p, (size_t)bz_L * Wc * sizeof(float2)) != hipSuccess) {
            d4w_fkd_plan_destroy(pl);
            return fail(D4W_ENOMEM, "hipMalloc of the Bluestein scratch (%d x %d complex) failed", bz_L, Wc);
        }
        cp.allocs.push_back(p);
        pl->bz_S = (float2*)p;
        pl->bz_L = bz_L; pl->bz_W = Wc;
    }
    pl->gen_c1 = axis_needs_generic(cp.dev.ax_c1);
    pl->gen_c2 = axis_needs_generic(cp.dev.ax_c2);
    pl->lds_c1 = ((size_t)C1 * TAc + 2 * kTwLo + cp.dev.ax_c1.nhi + cp.dev.ax_n1.nhi) * sizeof(float2);
    pl->lds_c2 = ((size_t)C2 * TC + kTwLo + cp.dev.ax_c2.nhi) * sizeof(float2);

    // ---------------- pair-op tables
    std::vector<int> p_c1(C1), p_c2(C2), p_n2(N2), rowk(nx), rowpart(nx), mirror0(N2), jqpart(std::max(nq, 1), 0);
    for (int p = 0; p < C1; ++p) p_c1[f_c1[p]] = p;
    for (int p = 0; p < C2; ++p) p_c2[f_c2[p]] = p;
    for (int p = 0; p < N2; ++p) p_n2[f_n2[p]] = p;
    if (bz_L || !want_mask) {                      // Bluestein: natural wavenumber order
        for (int r = 0; r < nx; ++r) { rowk[r] = r; rowpart[r] = (nx - r) % nx; }
    } else {
        for (int q = 0; q < C1; ++q)
            for (int p2 = 0; p2 < C2; ++p2) rowk[q * C2 + p2] = f_c1[q] + C1 * f_c2[p2];
        for (int r = 0; r < nx; ++r) {
            const int km = (nx - rowk[r]) % nx;
            rowpart[r] = p_c1[km % C1] * C2 + p_c2[km / C1];
        }
    }
    for (int i = 0; i < N2; ++i) mirror0[i] = p_n2[(N2 - f_n2[i]) % N2];
    for (int j = 0; j < nq; ++j)
        for (int j2 = 0; j2 < nq; ++j2)
            if (pl->myq[j2] == q1part[pl->myq[j]]) jqpart[j] = j2;
    std::vector<float2> wrow(N1), wcol(N2);
    for (int q1 = 0; q1 < N1; ++q1) wrow[q1] = wexp(f_n1[q1], ns);
    for (int i = 0; i < N2; ++i) wcol[i] = wexp((long long)N1 * f_n2[i], ns);
    pl->h_jqpart = jqpart; pl->h_mirror0 = mirror0;
    std::vector<int> myq = pl->myq;
    if (myq.empty()) myq.push_back(0);
    const int *c_rowk, *c_k1, *c_k2, *c_q1of;
    FkdSlab& S = pl->slab;
    S.nx = nx; S.nq = nq; S.N2 = N2;
    D4W_TRY(upload(&cp, myq, &c_q1of));
    D4W_TRY(upload(&cp, jqpart, &S.jq_partner));
    D4W_TRY(upload(&cp, rowpart, &S.row_partner));
    D4W_TRY(upload(&cp, mirror0, &S.mirror0));
    D4W_TRY(upload(&cp, wrow, &S.wrow));
    D4W_TRY(upload(&cp, wcol, &S.wcol));
    D4W_TRY(upload(&cp, rowk, &c_rowk));
    D4W_TRY(upload(&cp, f_n1, &c_k1));
    D4W_TRY(upload(&cp, f_n2, &c_k2));
    S.q1_of = c_q1of;
    pl->d_rowk = const_cast<int*>(c_rowk); pl->d_k1 = const_cast<int*>(c_k1); pl->d_k2 = const_cast<int*>(c_k2);
    pl->d_q1of = const_cast<int*>(c_q1of);
    S.hilbert = 0;
    if (want_mask) {
        void* p = nullptr;
        if (hipMalloc(&p, (size_t)nx * W * sizeof(float)) != hipSuccess) { d4w_fkd_plan_destroy(pl); return fail(D4W_ENOMEM, "hipMalloc of the slab mask failed"); }
        cp.allocs.push_back(p); pl->d_mask = (float*)p;
        if (hipMalloc(&p, (size_t)nx * sizeof(float)) != hipSuccess) { d4w_fkd_plan_destroy(pl); return fail(D4W_ENOMEM, "hipMalloc failed"); }
        cp.allocs.push_back(p); pl->d_nyq = (float*)p;
    }
    S.mask = pl->d_mask; S.nyq = pl->d_nyq;
#undef D4W_TRY
    {
        int devid = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&devid) == hipSuccess && hipGetDeviceProperties(&prop, devid) == hipSuccess)
            pl->num_cu = prop.multiProcessorCount;
        fk_pass_ac_lds_limit(80 * 1024);
        const void* fns[] = {
            (const void*)fkd_rows_n2<false, true>, (const void*)fkd_rows_n2<false, false>,
            (const void*)fkd_rows_n2<true, true>, (const void*)fkd_rows_n2<true, false>,
            (const void*)fkd_bz_passA_fwd<true>, (const void*)fkd_bz_passA_fwd<false>,
            (const void*)fkd_bz_passA_inv<true>, (const void*)fkd_bz_passA_inv<false>,
            (const void*)fkd_bz_passC<true>, (const void*)fkd_bz_passC<false>,
            (const void*)fkd_bt_passA_fwd<true>, (const void*)fkd_bt_passA_fwd<false>,
            (const void*)fkd_bt_passA_inv<true>, (const void*)fkd_bt_passA_inv<false>,
            (const void*)fkd_bt_rows<true>, (const void*)fkd_bt_rows<false>};
        for (const void* f : fns)
            (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
    }
    *out = pl;
    return D4W_OK;
}

extern "C" {

int d4w_fkd_plan_create(int nx, int ns, int world, int rank, d4w_fkd_plan** out) {
    return fkd_plan_build(nx, ns, world, rank, true, out);
}

/* info12 = {nx, ns, world, rank, row_begin, row_end, N1, N2, nq_local, C1, C2, packed (0 / 1)} */
int d4w_fkd_plan_info(const d4w_fkd_plan* pl, int* info) {
    if (!pl || !info) return fail(D4W_EINVAL, "NULL argument");
    const int v[12] = {pl->nx, pl->ns, pl->world, pl->rank, pl->row_begin, pl->row_end, pl->N1, pl->N2,
                       (int)pl->myq.size(), pl->C1, pl->C2, pl->sp ? 1 : 0};
    memcpy(info, v, sizeof(v));
    return D4W_OK;
}

/* info2 = {slab columns the Bluestein channel phase transforms with the mask set last, slab columns} ({0, 0}: the plan's
 * channel phase is not the global-memory Bluestein form) */
int d4w_fkd_plan_live_columns(const d4w_fkd_plan* pl, int* info2) {
    if (!pl || !info2) return fail(D4W_EINVAL, "NULL argument");
    const int W = (int)pl->myq.size() * pl->N2;
    info2[0] = pl->bz_L ? (pl->bz_nlive >= 0 ? pl->bz_nlive : W) : 0;
    info2[1] = pl->bz_L ? W : 0;
    return D4W_OK;
}

int d4w_fkd_plan_q1_owner(const d4w_fkd_plan* pl, int* owner) {
    if (!pl || !owner) return fail(D4W_EINVAL, "NULL argument");
    memcpy(owner, pl->owner.data(), pl->owner.size() * sizeof(int));
    return D4W_OK;
}

}  // extern "C"

// The live columns of a Bluestein channel phase (see d4w_fkd_plan::bz_cols): column maxima of the folded mask, the zero-gain
// level of fk_zero_gain (2^-24 / sqrt(nx ns) of the largest gain: the Gaussian tails of hybrid_ninf never reach an exact
// zero), closure under the pair op's column map, one small copy each way.  D4W_FKD_BZ_BAND=0 keeps every column (A/B).
static int fkd_bz_live_columns(d4w_fkd_plan* pl, void* stream) {
    pl->bz_nlive = -1;
    static const int band_env = [] { const char* v = getenv("D4W_FKD_BZ_BAND"); return v ? atoi(v) : 1; }();
    const int nq = (int)pl->myq.size(), N2 = pl->N2, W = nq * N2;
    if (!pl->bz_L || !band_env || nq == 0 || !pl->d_mask) return D4W_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!pl->bz_cols) {
        void* p = nullptr;
        if (hipMalloc(&p, (size_t)W * sizeof(int)) != hipSuccess) return fail(D4W_ENOMEM, "hipMalloc of the live-column list failed");
        pl->cp.allocs.push_back(p); pl->bz_cols = (int*)p;
        if (hipMalloc(&p, (size_t)W * sizeof(unsigned)) != hipSuccess) return fail(D4W_ENOMEM, "hipMalloc of the live-column flags failed");
        pl->cp.allocs.push_back(p); pl->bz_flags = (unsigned*)p;
    }
    const dim3 grid(ceil_div(W, kThreads), std::min(pl->nx, 64));
    D4W_HIP(hipMemsetAsync(pl->bz_flags, 0, (size_t)W * sizeof(unsigned), st));
    D4W_LAUNCH(fkd_col_max, grid, dim3(kThreads), 0, stream, (const float*)pl->d_mask, pl->nx, W, pl->bz_flags);
    std::vector<unsigned> cm((size_t)W);
    D4W_HIP(hipMemcpyAsync(cm.data(), pl->bz_flags, (size_t)W * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    D4W_HIP(hipStreamSynchronize(st));
    float gmax = 0.f;
    for (int c = 0; c < W; ++c) { float g; memcpy(&g, &cm[c], 4); if (g < INFINITY) gmax = std::max(gmax, g); }
    FkDims dd{};
    dd.nx = pl->nx; dd.ns = pl->ns;
    const float zero_gain = (float)fk_zero_gain(dd, pl->prune_eps, (double)gmax);
    std::vector<unsigned> live((size_t)W, 0u);
    auto is_live = [&](size_t c) { float g; memcpy(&g, &cm[c], 4); return g > zero_gain; };
    for (int jq = 0; jq < nq; ++jq) {
        const bool k1zero = (pl->myq[jq] == 0);
        const int jp = pl->h_jqpart[jq];
        for (int i = 0; i < N2; ++i) {
            const int j = k1zero ? pl->h_mirror0[i] : (N2 - 1 - i);
            const size_t a = (size_t)jq * N2 + i, b = (size_t)jp * N2 + j;
            if (is_live(a) || is_live(b) || (k1zero && i == 0)) live[a] = live[b] = 1u;     // (the DC / Nyquist column: gains in d_nyq)
        }
    }
    std::vector<int> cols;
    cols.reserve((size_t)W);
    for (int c = 0; c < W; ++c) if (live[c]) cols.push_back(c);
    if ((int)cols.size() >= W) return D4W_OK;                                     // nothing to skip
    D4W_HIP(hipMemcpyAsync(pl->bz_cols, cols.data(), cols.size() * sizeof(int), hipMemcpyHostToDevice, st));
    D4W_HIP(hipMemcpyAsync(pl->bz_flags, live.data(), (size_t)W * sizeof(unsigned), hipMemcpyHostToDevice, st));
    D4W_LAUNCH(fkd_zero_dead_cols, grid, dim3(kThreads), 0, stream, pl->d_mask, pl->nx, W, (const unsigned*)pl->bz_flags);
    D4W_HIP(hipStreamSynchronize(st));                                            // (the host vectors go out of scope)
    pl->bz_nlive = (int)cols.size();
    return D4W_OK;
}

static int fkd_launch_fold(const FkdMaskSrc& src, int nx, int ns, int N1, int N2, int nq, const int* rowk, const int* q1of,
                           const int* k1, const int* k2, float* mask, float* nyq, void* stream) {
    dim3 grid(std::min(ceil_div(nq * N2, kThreads), 64), nx);
    if (src.dense)
        D4W_LAUNCH(fkd_fold_mask, grid, dim3(kThreads), 0, stream, nx, ns, N1, N2, nq, src.dense, rowk, q1of, k1, k2, mask, nyq, src.aff);
    else
        D4W_LAUNCH(fkd_fold_design, grid, dim3(kThreads), 0, stream, nx, ns, N1, N2, nq, src.A, src.mode, rowk, q1of, k1, k2,
                   mask, nyq);
    return D4W_OK;
}

static int fkd_set_mask_packed(d4w_fkd_plan* pl, const FkdMaskSrc& src, void* stream) {
    d4w_fk_plan* sp = pl->sp;
    const FkDims& d = sp->dev.d;
    const int nq = (int)pl->myq.size();
    hipStream_t st = (hipStream_t)stream;
    pl->has_mask = true;
    pl->fdev_c.pairs = pl->d_pairs_slab;
    pl->fdev_c.live = nullptr;
    pl->npairs_run = (int)pl->h_pairs_slab.size();
    pl->live_rows = d.nx;
    if (nq == 0) return D4W_OK;
    const int W = nq * d.N2;
    if (int rc = fkd_launch_fold(src, d.nx, d.ns, d.N1, d.N2, nq, (const int*)sp->d_rowk, (const int*)pl->d_q1of,
                                 (const int*)sp->d_k1, (const int*)sp->d_k2, pl->d_mask, pl->d_nyq, stream))
        return rc;
    const char* np = getenv("D4W_FK_NOPRUNE");
    if (np && atoi(np) > 0) return D4W_OK;
    // rows whose gains are all zero in the owned sub-rows (and whose Hermitian partner's are): skipped by passes
    // C, B, C' of this rank's slab, exactly as in the single-device plan
    D4W_HIP(hipMemsetAsync(pl->d_rowmax, 0, (size_t)d.nx * sizeof(unsigned), st));
    D4W_LAUNCH(fkd_row_max, dim3(d.nx), dim3(kThreads), 0, stream, (const float*)pl->d_mask, (const float*)pl->d_nyq, W,
               pl->d_rowmax);
    std::vector<unsigned> rmax(d.nx);
    D4W_HIP(hipMemcpyAsync(rmax.data(), pl->d_rowmax, (size_t)d.nx * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    D4W_HIP(hipStreamSynchronize(st));
    std::vector<char> lv(d.nx, 0);
    std::vector<int2> run;
    run.reserve(pl->h_pairs_slab.size());
    for (const int2& pr : pl->h_pairs_slab) {
        const int ra = pr.x / nq, rb = pr.y / nq;
        if (rmax[ra] || rmax[rb]) {
            lv[ra] = lv[rb] = 1;
            run.push_back(pr);
        }
    }
    int nlive = 0;
    for (int r = 0; r < d.nx; ++r) nlive += lv[r];
    if (nlive < d.nx) {
        const int RA = sp->fast->C2A, RB = sp->fast->C2B;
        std::vector<unsigned> bits((size_t)d.C1 * RA, 0u);
        for (int r = 0; r < d.nx; ++r)
            if (lv[r]) {
                const int q = r / d.C2, p2 = r % d.C2;
                bits[(size_t)q * RA + p2 / RB] |= 1u << (p2 % RB);
            }
        D4W_HIP(hipMemcpyAsync(pl->d_livebits, bits.data(), bits.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
        if (!run.empty())
            D4W_HIP(hipMemcpyAsync(pl->d_pairs_live, run.data(), run.size() * sizeof(int2), hipMemcpyHostToDevice, st));
        D4W_HIP(hipStreamSynchronize(st));
        pl->fdev_c.live = pl->d_livebits;
        pl->fdev_c.pairs = pl->d_pairs_live;
        pl->npairs_run = (int)run.size();
        pl->live_rows = nlive;
    }
    return D4W_OK;
}

static int fkd_set_mask_src(d4w_fkd_plan* pl, const FkdMaskSrc& src, void* stream) {
    if (pl->nx > 65535) return fail(D4W_EINVAL, "nx = %d exceeds the grid limit 65535", pl->nx);
    if (pl->sp) return fkd_set_mask_packed(pl, src, stream);
    const int nq = (int)pl->myq.size();
    if (nq > 0)
        if (int rc = fkd_launch_fold(src, pl->nx, pl->ns, pl->N1, pl->N2, nq, (const int*)pl->d_rowk, (const int*)pl->d_q1of,
                                     (const int*)pl->d_k1, (const int*)pl->d_k2, pl->d_mask, pl->d_nyq, stream))
            return rc;
    if (int rc = fkd_bz_live_columns(pl, stream)) return rc;
    pl->has_mask = true;
    return D4W_OK;
}

void d4w::fkd_set_prune(d4w_fkd_plan* pl, double prune_eps) { pl->prune_eps = prune_eps; }
int d4w::fkd_set_mask_dense_affine(d4w_fkd_plan* pl, const float* mask_shifted, float a, float b, int on, void* stream) {
    if (!pl || !mask_shifted || !pl->d_mask) return fail(D4W_EINVAL, "NULL argument");
    if (on && pl->sp) return fail(D4W_EINVAL, "the packed distributed plan folds no affine map");
    FkdMaskSrc src;
    src.dense = mask_shifted;
    src.aff = FkAffine{a, b, on};
    return fkd_set_mask_src(pl, src, stream);
}

static int fkd_chan_apply_packed(d4w_fkd_plan* pl, float* slab, void* stream) {
    const FkFastEntry& F = *pl->sp->fast;
    const FkDims& d = pl->sp->dev.d;
    const int nq = (int)pl->myq.size();
    if (nq == 0) return D4W_OK;
    const int W = nq * d.N2;
    const int nblkA = ceil_div(W, d.N1 * d.TA), nblkC = W / d.TC;
    const int ntA = d.C2 * nblkA, ntC = d.C1 * nblkC;
    float2* d2 = reinterpret_cast<float2*>(slab);
    const int cu = pl->num_cu;
    const dim3 gA(std::min(ntA, cu * pl->sp->wgA)), gC(std::min(ntC, cu * pl->sp->wgC)),
        gB(std::max(1, std::min(pl->npairs_run, cu * pl->sp->wgB)));
    int rc;
    // pass A MODE 2: tile u -> (c2 = u / nblkA, column block u % nblkA)
    if ((rc = launch_k(F.Ac_fwd, gA, dim3(F.thrA), F.ldsA, stream, pl->dev_c, (const float2*)d2, d2, 0, ntA, nblkA, 0, pl->geo_c))) return rc;
    if ((rc = launch_k(F.Cs_fwd, gC, dim3(F.thrC), F.ldsC, stream, pl->dev_c, pl->fdev_c, d2, 0, ntC, nblkC, 0, pl->geo_c))) return rc;
    FkGeo gb = pl->geo_c;
    gb.nq = nq;
    if (pl->npairs_run > 0 &&
        (rc = launch_k(F.Bs_mid, gB, dim3(F.thrB), F.ldsB, stream, pl->dev_c, pl->fdev_c, d2, 0, pl->npairs_run, gb))) return rc;
    if ((rc = launch_k(F.Cs_inv, gC, dim3(F.thrC), F.ldsC, stream, pl->dev_c, pl->fdev_c, d2, 0, ntC, nblkC, 0, pl->geo_c))) return rc;
    return launch_k(F.Ac_inv, gA, dim3(F.thrA), F.ldsA, stream, pl->dev_c, d2, 0, ntA, nblkA, 0, pl->geo_c, (const float2*)nullptr);
}

// time transform of the local rows as a Bluestein convolution through the scratch, a chunk of rows at a time
// (inv = 0: packed real rows -> half spectrum in natural order; inv = 1: back, x tp.dev.scale)
static int fkd_time_bluestein(d4w_fkd_plan* pl, const float2* src, float2* dst, int inv, int taper, void* stream) {
    FkDev P = pl->tp.dev;
    P.scale = 1.0f;
    const int nxl = P.d.nx, L = pl->bt_L, R = pl->bt_R;
    const int persist = pl->num_cu * 4;
    const dim3 blk(kMaxThreads);
    FkdBt Z;
    Z.chirp = pl->bt_chirp; Z.filt = pl->bt_filt; Z.win = (taper && !inv) ? pl->bt_win : nullptr;
    Z.pitch = (size_t)pl->M; Z.m = pl->M; Z.inv = inv;
    Z.scale = inv ? pl->tp.dev.scale : 1.0f;
    (void)L;
    for (int r0 = 0; r0 < nxl; r0 += R) {
        const int nr = std::min(R, nxl - r0);
        const int ntA = ceil_div(P.d.N2, P.d.TA) * nr, nsub = nr * P.d.N1;
        int rc;
        if ((rc = launch_k(pl->gen_t ? fkd_bt_passA_fwd<true> : fkd_bt_passA_fwd<false>, dim3(std::min(ntA, persist)), blk, pl->lds_t, stream, P, Z, src + (size_t)r0 * pl->M, pl->bt_S, ntA))) return rc;
        if ((rc = launch_k(pl->gen_n2 ? fkd_bt_rows<true> : fkd_bt_rows<false>, dim3(std::min(nsub, persist)), blk, pl->lds_n2, stream, P, Z, pl->bt_S, nsub))) return rc;
        if ((rc = launch_k(pl->gen_t ? fkd_bt_passA_inv<true> : fkd_bt_passA_inv<false>, dim3(std::min(ntA, persist)), blk, pl->lds_t, stream, P, Z, (const float2*)pl->bt_S, dst + (size_t)r0 * pl->M, ntA))) return rc;
    }
    return D4W_OK;
}

extern "C" {

int d4w_fkd_plan_is_packed(const d4w_fkd_plan* pl) { return (pl && pl->sp) ? 1 : 0; }

int d4w_fkd_set_mask_dense_f32(d4w_fkd_plan* pl, const float* mask_shifted, void* stream) {
    if (!pl || !mask_shifted || !pl->d_mask) return fail(D4W_EINVAL, "NULL argument");
    FkdMaskSrc src;
    src.dense = mask_shifted;
    return fkd_set_mask_src(pl, src, stream);
}

int d4w_fkd_set_mask_design_f32(d4w_fkd_plan* pl, int mode, double k_spacing, double t_spacing, const double* params8_host,
                                int i0, int i1, const double* hrow_dev, void* stream) {
    if (!pl || !params8_host || !pl->d_mask) return fail(D4W_EINVAL, "NULL argument");
    if (mode < 0 || mode > 2)
        return fail(D4W_EINVAL, "mode %d has no closed form (the Gaussian-blurred designs go through d4w_design_mask_f32)", mode);
    if (mode == 2 && !hrow_dev) return fail(D4W_EINVAL, "hybrid_ninf needs the |H|^2 row");
    FkdMaskSrc src;
    src.A = make_design_args(pl->nx, pl->ns, k_spacing, t_spacing, params8_host, i0, i1, hrow_dev);
    src.mode = mode;
    return fkd_set_mask_src(pl, src, stream);
}

/* packed path: x_loc [nxl][ns] -> packed [dest rank][nxl][nq(dest)][N2] complex (what the all-to-all sends) */
int d4w_fkd_time_fwd_packed_rows_f32(d4w_fkd_plan* pl, const float* x_loc, float* packed, int taper, int l0, int l1,
                                     void* stream) {
    if (!pl || !x_loc || !packed) return fail(D4W_EINVAL, "NULL argument");
    if (!pl->sp) return fail(D4W_EINVAL, "this shape runs the generic distributed plan: d4w_fkd_time_fwd_f32");
    const FkFastEntry& F = *pl->sp->fast;
    const FkDims& d = pl->sp->dev.d;
    const int nxl = pl->row_end - pl->row_begin;
    if (l0 < 0 || l1 > nxl || l0 > l1 || l0 % d.C1) return fail(D4W_EINVAL, "row range [%d, %d) must start at a multiple of %d inside the local block", l0, l1, d.C1);
    const int NBX = d.N2 / d.TA, t0 = (l0 / d.C1) * NBX, t1 = ceil_div(l1, d.C1) * NBX;
    if (t1 <= t0) return D4W_OK;
    FkGeo geo = pl->geo_t;
    geo.nrows = l1;                                   // rows >= l1 of the last group belong to the next chunk
    return launch_k(taper ? F.T_fwd_taper : F.T_fwd, dim3(std::min(t1 - t0, pl->num_cu * pl->sp->wgA)), dim3(F.thrA), F.ldsA, stream,
                    pl->dev_t, reinterpret_cast<const float2*>(x_loc), reinterpret_cast<float2*>(packed), t0, t1, NBX, 0, geo);
}

int d4w_fkd_time_fwd_packed_f32(d4w_fkd_plan* pl, const float* x_loc, float* packed, int taper, void* stream) {
    if (!pl) return fail(D4W_EINVAL, "NULL argument");
    return d4w_fkd_time_fwd_packed_rows_f32(pl, x_loc, packed, taper, 0, pl->row_end - pl->row_begin, stream);
}

/* packed path: packed [src rank][nxl][nq(src)][N2] (what the second all-to-all delivers) -> y_loc [nxl][ns] */
int d4w_fkd_time_inv_packed_rows_f32(d4w_fkd_plan* pl, const float* packed, float* y_loc, int l0, int l1, void* stream) {
    if (!pl || !packed || !y_loc) return fail(D4W_EINVAL, "NULL argument");
    if (!pl->sp) return fail(D4W_EINVAL, "this shape runs the generic distributed plan: d4w_fkd_time_inv_f32");
    const FkFastEntry& F = *pl->sp->fast;
    const FkDims& d = pl->sp->dev.d;
    const int nxl = pl->row_end - pl->row_begin;
    if (l0 < 0 || l1 > nxl || l0 > l1 || l0 % d.C1) return fail(D4W_EINVAL, "row range [%d, %d) must start at a multiple of %d inside the local block", l0, l1, d.C1);
    const int NBX = d.N2 / d.TA, t0 = (l0 / d.C1) * NBX, t1 = ceil_div(l1, d.C1) * NBX;
    if (t1 <= t0) return D4W_OK;
    FkGeo geo = pl->geo_t;
    geo.nrows = l1;
    return launch_k(F.T_inv, dim3(std::min(t1 - t0, pl->num_cu * pl->sp->wgA)), dim3(F.thrA), F.ldsA, stream, pl->dev_t,
                    reinterpret_cast<float2*>(y_loc), t0, t1, NBX, 0, geo, reinterpret_cast<const float2*>(packed));
}

/* ... with the row statistics of the filtered rows (mean, max|.|: what the matched filter normalises by, detect.py:157)
 * from the pass's epilogue; row_mean / row_maxabs [nxl] must be zeroed before the first chunk */
int d4w_fkd_time_inv_packed_rows_stats_f32(d4w_fkd_plan* pl, const float* packed, float* y_loc, int l0, int l1,
                                           double* row_mean, float* row_maxabs, void* stream) {
    if (!pl || !packed || !y_loc || !row_mean || !row_maxabs) return fail(D4W_EINVAL, "NULL argument");
    if (!pl->sp) return fail(D4W_EINVAL, "this shape runs the generic distributed plan");
    const FkFastEntry& F = *pl->sp->fast;
    const FkDims& d = pl->sp->dev.d;
    const int nxl = pl->row_end - pl->row_begin;
    if (l0 < 0 || l1 > nxl || l0 > l1 || l0 % d.C1) return fail(D4W_EINVAL, "row range [%d, %d) must start at a multiple of %d inside the local block", l0, l1, d.C1);
    const int NBX = d.N2 / d.TA, t0 = (l0 / d.C1) * NBX, t1 = ceil_div(l1, d.C1) * NBX;
    if (t1 <= t0) return D4W_OK;
    int run = 1;
    for (int r = 1; r <= NBX && r <= 30; ++r) if (NBX % r == 0) run = r;
    const int nruns = (t1 - t0) / run;
    FkGeo geo = pl->geo_t;
    geo.nrows = l1;
    return launch_k(F.T_inv_stats, dim3(std::min(nruns, pl->num_cu * pl->sp->wgA)), dim3(F.thrA), F.ldsA, stream, pl->dev_t,
                    reinterpret_cast<float2*>(y_loc), run, nruns, row_mean, (unsigned*)row_maxabs, NBX, 0, geo,
                    reinterpret_cast<const float2*>(packed), t0);
}

int d4w_fkd_time_inv_packed_f32(d4w_fkd_plan* pl, const float* packed, float* y_loc, void* stream) {
    if (!pl) return fail(D4W_EINVAL, "NULL argument");
    return d4w_fkd_time_inv_packed_rows_f32(pl, packed, y_loc, 0, pl->row_end - pl->row_begin, stream);
}

int d4w_fkd_time_fwd_f32(d4w_fkd_plan* pl, const float* x_loc, float* z_loc, int taper, void* stream) {
    if (!pl || !x_loc || !z_loc) return fail(D4W_EINVAL, "NULL argument");
    if (pl->sp) return fail(D4W_EINVAL, "this shape runs the packed distributed plan: d4w_fkd_time_fwd_packed_f32");
    if (pl->bt_L) return fkd_time_bluestein(pl, reinterpret_cast<const float2*>(x_loc), reinterpret_cast<float2*>(z_loc), 0, taper, stream);
    const FkDev& P = pl->tp.dev;
    const int nxl = P.d.nx;
    const int ntA = ceil_div(P.d.N2, P.d.TA) * nxl, nsub = nxl * pl->N1;
    const int persist = pl->num_cu * 4;
    const float2* src = reinterpret_cast<const float2*>(x_loc);
    float2* dst = reinterpret_cast<float2*>(z_loc);
    const dim3 blk(kMaxThreads);
    if (int rc = fk_launch_passA_fwd(taper != 0, pl->gen_t, dim3(std::min(ntA, persist)), blk, pl->lds_t, stream, P, src, dst, ntA)) return rc;
    return fkd_launch_rows_n2(false, pl->gen_n2, dim3(std::min(nsub, persist)), blk, pl->lds_n2, stream, P, dst, nsub);
}

int d4w_fkd_time_inv_f32(d4w_fkd_plan* pl, float* z_loc, void* stream) {
    if (!pl || !z_loc) return fail(D4W_EINVAL, "NULL argument");
    if (pl->sp) return fail(D4W_EINVAL, "this shape runs the packed distributed plan: d4w_fkd_time_inv_packed_f32");
    if (pl->bt_L) return fkd_time_bluestein(pl, reinterpret_cast<const float2*>(z_loc), reinterpret_cast<float2*>(z_loc), 1, 0, stream);
    const FkDev& P = pl->tp.dev;
    const int nxl = P.d.nx;
    const int ntA = ceil_div(P.d.N2, P.d.TA) * nxl, nsub = nxl * pl->N1;
    const int persist = pl->num_cu * 4;
    float2* d2 = reinterpret_cast<float2*>(z_loc);
    const dim3 blk(kMaxThreads);
    if (int rc = fkd_launch_rows_n2(true, pl->gen_n2, dim3(std::min(nsub, persist)), blk, pl->lds_n2, stream, P, d2, nsub)) return rc;
    return fk_launch_passA_inv(pl->gen_t, dim3(std::min(ntA, persist)), blk, pl->lds_t, stream, P, d2, ntA);
}

int d4w_fkd_chan_apply_f32(d4w_fkd_plan* pl, float* slab, void* stream) {
    if (!pl || (!slab && !pl->myq.empty())) return fail(D4W_EINVAL, "NULL argument");
    if (!pl->has_mask) return fail(D4W_EINVAL, "no mask set on this plan");
    if (pl->sp) return fkd_chan_apply_packed(pl, slab, stream);
    const int nq = (int)pl->myq.size();
    if (nq == 0) return D4W_OK;
    const FkDev& P = pl->cp.dev;
    const FkDims& d = P.d;
    const int ntA = ceil_div(d.N2, d.TA) * d.C2, ntC = ceil_div(d.M, d.TC) * d.C1;
    const int persist = pl->num_cu * 4;
    float2* d2 = reinterpret_cast<float2*>(slab);
    const dim3 blk(kMaxThreads);
    int rc;
    if (pl->bz_L) {
        // channel DFT, pair operation with the folded mask, inverse channel DFT -- each DFT a Bluestein convolution
        // through the scratch, a chunk of columns at a time (the columns are independent)
        if (pl->nx > 65535 || nq > 65535) return fail(D4W_EINVAL, "slab %d x %d exceeds the pair-op grid", pl->nx, nq);
        const int W = nq * pl->N2, Wc = pl->bz_W, L = pl->bz_L;
        float2* S = pl->bz_S;
        (void)L;
        // the live columns only, gathered into the scratch through the list (dead columns: zeros out of the pair op)
        const bool listed = pl->bz_nlive >= 0;
        const int Wl = listed ? pl->bz_nlive : W;
        for (int inv = 0; inv < 2; ++inv) {
            for (int c0 = 0; c0 < Wl; c0 += Wc) {
                FkdBz Z;
                Z.chirp = pl->bz_chirp; Z.filt = pl->bz_filt; Z.pitch = (size_t)W; Z.nx = pl->nx;
                Z.ncol = std::min(Wc, Wl - c0); Z.inv = inv;
                Z.scale = inv ? (float)(1.0 / ((double)pl->nx * (double)pl->M)) : 1.0f;
                Z.cols = listed ? pl->bz_cols + c0 : nullptr;
                float2* base = listed ? d2 : d2 + c0;
                if ((rc = launch_k(pl->gen_c1 ? fkd_bz_passA_fwd<true> : fkd_bz_passA_fwd<false>, dim3(std::min(ntA, persist)), blk, pl->lds_c1, stream, P, Z, (const float2*)base, S, ntA))) return rc;
                if ((rc = launch_k(pl->gen_c2 ? fkd_bz_passC<true> : fkd_bz_passC<false>, dim3(std::min(ntC, persist)), blk, pl->lds_c2, stream, P, Z, S, ntC))) return rc;
                if ((rc = launch_k(pl->gen_c1 ? fkd_bz_passA_inv<true> : fkd_bz_passA_inv<false>, dim3(std::min(ntA, persist)), blk, pl->lds_c1, stream, P, Z, (const float2*)S, base, ntA))) return rc;
            }
            if (!inv && (rc = fkd_launch_pair_slab(pl->slab, d2, stream))) return rc;
        }
        return D4W_OK;
    }
    if ((rc = fk_launch_passA_fwd(false, pl->gen_c1, dim3(std::min(ntA, persist)), blk, pl->lds_c1, stream, P, (const float2*)d2, d2, ntA))) return rc;
    if ((rc = fk_launch_passC(false, pl->gen_c2, dim3(std::min(ntC, persist)), blk, pl->lds_c2, stream, P, d2, ntC))) return rc;
    if (pl->nx > 65535 || nq > 65535) return fail(D4W_EINVAL, "slab %d x %d exceeds the pair-op grid", pl->nx, nq);
    if ((rc = fkd_launch_pair_slab(pl->slab, d2, stream))) return rc;
    if ((rc = fk_launch_passC(true, pl->gen_c2, dim3(std::min(ntC, persist)), blk, pl->lds_c2, stream, P, d2, ntC))) return rc;
    return fk_launch_passA_inv(pl->gen_c1, dim3(std::min(ntA, persist)), blk, pl->lds_c1, stream, P, d2, ntA);
}

}  // extern "C"
