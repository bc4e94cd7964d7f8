// f-k filter application on MI355X (gfx950): y = real(ifft2(fft2(x) * M')), M' = unshifted mask.
// Replaces dsp.fk_filter_filt / dsp.fk_filter_sparsefilt (reference dsp.py:725-786).
//
// Formulation (see DESIGN.md "f-k filter"):
//   * the real [nx][ns] block is reinterpreted as a complex [nx][M] block, M = ns/2
//     (z[c][m] = x[c][2m] + i x[c][2m+1]) -- no conversion pass, the bytes are the same;
//   * a 2-D complex FFT of z is computed with both axes split four-step style,
//     nx = C1*C2 (c = c1*C2 + c2) and M = N1*N2 (m = n1*N2 + n2), every 1-D sub-transform running
//     in LDS as an in-place DIF (forward) / DIT (inverse) pair, so spectra stay in digit-reversed
//     order and no transposition is ever written to HBM;
//   * because x is real, the spectrum X(k,f) of x follows from Z(k,f) and conj(Z(-k,M-f)); the
//     "pair op" in the middle pass untangles the two, applies the Hermitian-folded mask to
//     X(k,f) and X(k,f+M), and re-tangles -- so no R2C/C2R pass exists either.
//
// Five HBM passes, each reading and writing the block once, all in place on y:
//   A  fwd : tile (all c1) x (all n1) x TA contiguous n2 : 2-D FFT over (c1,n1), 4-step twiddles
//   C  fwd : tile (all c2) x TC contiguous columns       : FFT over c2
//   B  mid : two contiguous sub-rows of N2 (a row and its Hermitian partner):
//            FFT over n2 -> pair op with mask -> inverse FFT over n2
//   C' inv, A' inv (+ 1/(nx*M) scale).
// This unit: the generic pass kernels and their launchers, the mask fold kernels, the shape registry, the planner,
// mask handling and apply.  The distributed filter is fk_dist.hip; what the two share is fk_plan.h.
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <map>

#include "fk_plan.h"

namespace d4w {

// Every pass kernel is persistent (grid = 2 workgroups per CU) and software-pipelined:
//     prefetch tile i+1 (global -> registers, no wait) | FFT stages of tile i in LDS | store tile i
// The FFT stages touch only LDS (twiddles included), so the prefetch loads stay in flight across
// the whole compute phase and the stores of tile i drain under the next iteration.

// ---------------------------------------------------------------------------------------------
// pass A : (c1, n1) strided 2-D sub-transform.  tile id = c2 * ntx + bx  (bx fastest: adjacent
// workgroups touch adjacent 64/128-byte segments of the same rows)
// ---------------------------------------------------------------------------------------------
template <bool TAPER, bool GENERIC>
__global__ __launch_bounds__(kMaxThreads) void fk_passA_fwd(FkDev P, const float2* __restrict__ src,
                                                            float2* __restrict__ dst, int ntiles) {
    D4W_DYN_LDS(smem_raw);
    float2* tile = reinterpret_cast<float2*>(smem_raw);
    const FkDims& d = P.d;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int TA = d.TA;
    const int nelem = d.C1 * d.N1 * TA;
    const int ntx = (d.N2 + TA - 1) / TA;
    const FDiv dTA(TA), dN1(d.N1), dntx(ntx);
    const TwLds tw_c1 = tw_stage(P.ax_c1, tile + nelem, tid, nthr);
    const TwLds tw_n1 = tw_stage(P.ax_n1, tile + nelem + tw_lds_elems(P.ax_c1), tid, nthr);
    float2 pf[kPF];
    auto issue = [&](int t) {
        const int c2 = dntx.div(t), b0 = (t - c2 * ntx) * TA;
        const int ncol = min(TA, d.N2 - b0);
#pragma unroll
        for (int it = 0; it < kPF; ++it) {
            const int w = tid + it * nthr;
            float2 v = make_float2(0.f, 0.f);
            if (w < nelem) {
                const int seg = dTA.div(w), tt = w - seg * TA;
                const int c1 = dN1.div(seg), n1 = seg - c1 * d.N1;
                if (tt < ncol) {
                    const size_t row = (size_t)c1 * d.C2 + c2;
                    const int col = n1 * d.N2 + b0 + tt;
                    v = src[row * d.M + col];
                    if (TAPER) {
                        const float2 wv = P.win[col];
                        v.x *= wv.x;
                        v.y *= wv.y;
                    }
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
        lds_fft<false, true, GENERIC>(tile, P.ax_c1, tw_c1, d.N1 * TA, d.N1 * TA, 1, 1, 0, tid, nthr);
        lds_fft<false, true, GENERIC>(tile, P.ax_n1, tw_n1, TA, TA, 1, d.C1, d.N1 * TA, tid, nthr);
        const int c2 = dntx.div(t), b0 = (t - c2 * ntx) * TA;
        const int ncol = min(TA, d.N2 - b0);
        for (int w = tid; w < nelem; w += nthr) {
            const int seg = dTA.div(w), tt = w - seg * TA;
            const int q = dN1.div(seg), q1 = seg - q * d.N1;
            if (tt < ncol) {
                const float2 t1 = P.twc[q * d.C2 + c2];
                const float2 t2 = P.twt[q1 * d.N2 + b0 + tt];
                const size_t row = (size_t)q * d.C2 + c2;
                dst[row * d.M + q1 * d.N2 + b0 + tt] = c_mul(tile[w], c_mul(t1, t2));
            }
        }
        lds_barrier();
        t = next;
    }
}

template <bool GENERIC>
__global__ __launch_bounds__(kMaxThreads) void fk_passA_inv(FkDev P, float2* __restrict__ data, int ntiles) {
    D4W_DYN_LDS(smem_raw);
    float2* tile = reinterpret_cast<float2*>(smem_raw);
    const FkDims& d = P.d;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int TA = d.TA;
    const int nelem = d.C1 * d.N1 * TA;
    const int ntx = (d.N2 + TA - 1) / TA;
    const FDiv dTA(TA), dN1(d.N1), dntx(ntx);
    const TwLds tw_c1 = tw_stage(P.ax_c1, tile + nelem, tid, nthr);
    const TwLds tw_n1 = tw_stage(P.ax_n1, tile + nelem + tw_lds_elems(P.ax_c1), tid, nthr);
    float2 pf[kPF];
    auto issue = [&](int t) {
        const int c2 = dntx.div(t), b0 = (t - c2 * ntx) * TA;
        const int ncol = min(TA, d.N2 - b0);
#pragma unroll
        for (int it = 0; it < kPF; ++it) {
            const int w = tid + it * nthr;
            float2 v = make_float2(0.f, 0.f);
            if (w < nelem) {
                const int seg = dTA.div(w), tt = w - seg * TA;
                const int q = dN1.div(seg), q1 = seg - q * d.N1;
                if (tt < ncol) {
                    const size_t row = (size_t)q * d.C2 + c2;
                    v = data[row * d.M + q1 * d.N2 + b0 + tt];
                }
            }
            pf[it] = v;
        }
    };
    int t = blockIdx.x;
    if (t < ntiles) issue(t);
    while (t < ntiles) {
        const int c2 = dntx.div(t), b0 = (t - c2 * ntx) * TA;
        const int ncol = min(TA, d.N2 - b0);
#pragma unroll
        for (int it = 0; it < kPF; ++it) {
            const int w = tid + it * nthr;
            if (w < nelem) {
                const int seg = dTA.div(w), tt = w - seg * TA;
                const int q = dN1.div(seg), q1 = seg - q * d.N1;
                float2 v = pf[it];
                if (tt < ncol) v = c_mulc(v, c_mul(P.twc[q * d.C2 + c2], P.twt[q1 * d.N2 + b0 + tt]));
                tile[w] = v;
            }
        }
        lds_barrier();
        const int next = t + gridDim.x;
        if (next < ntiles) issue(next);
        lds_fft<true, true, GENERIC>(tile, P.ax_n1, tw_n1, TA, TA, 1, d.C1, d.N1 * TA, tid, nthr);
        lds_fft<true, true, GENERIC>(tile, P.ax_c1, tw_c1, d.N1 * TA, d.N1 * TA, 1, 1, 0, tid, nthr);
        for (int w = tid; w < nelem; w += nthr) {
            const int seg = dTA.div(w), tt = w - seg * TA;
            const int c1 = dN1.div(seg), n1 = seg - c1 * d.N1;
            if (tt < ncol) {
                const size_t row = (size_t)c1 * d.C2 + c2;
                data[row * d.M + n1 * d.N2 + b0 + tt] = c_scale(tile[w], P.scale);
            }
        }
        lds_barrier();
        t = next;
    }
}

// ---------------------------------------------------------------------------------------------
// pass C : c2 sub-transform over C2 consecutive rows, TC contiguous columns; tile id = q*ntx + bx
// ---------------------------------------------------------------------------------------------
template <bool INV, bool GENERIC>
__global__ __launch_bounds__(kMaxThreads) void fk_passC(FkDev P, float2* __restrict__ data, int ntiles) {
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
        const float2* base = data + ((size_t)q * d.C2) * d.M + p0;
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
        lds_fft<INV, true, GENERIC>(tile, P.ax_c2, tw, TC, TC, 1, 1, 0, tid, nthr);
        const int q = dntx.div(t), p0 = (t - q * ntx) * TC;
        const int ncol = min(TC, d.M - p0);
        float2* base = data + ((size_t)q * d.C2) * d.M + p0;
        for (int w = tid; w < nelem; w += nthr) {
            const int c2 = dTC.div(w), tt = w - c2 * TC;
            if (tt < ncol) base[(size_t)c2 * d.M + tt] = tile[w];
        }
        lds_barrier();
        t = next;
    }
}

// pass C when C2 has a prime factor > 31 (Bluestein): the tile holds bs_L >= 2 C2 - 1 rows per column,
//   a[n] = x[n] w[n] (n < C2, zero above), A = FFT_L(a), A *= FFT_L(conj w wrapped) / L, c = IFFT_L(A),
//   X[k] = w[k] c[k] (k < C2), w[n] = exp(-i pi n^2 / C2); the inverse transform conjugates w and the filter.
// Output in NATURAL order (the plan's c2 position -> wavenumber map is the identity).  Exact in the same
// sense as the other passes (float32 rounding), slower: twice the LDS tile and three transforms per column.
template <bool INV>
__global__ __launch_bounds__(kMaxThreads) void fk_passC_bluestein(FkDev P, float2* __restrict__ data, int ntiles) {
    D4W_DYN_LDS(smem_raw);
    float2* tile = reinterpret_cast<float2*>(smem_raw);
    const FkDims& d = P.d;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int TC = d.TC, L = P.bs_L;
    const int nelem = d.C2 * TC, ntile = L * TC;
    const int ntx = (d.M + TC - 1) / TC;
    const TwLds tw = tw_stage(P.ax_bs, tile + ntile, tid, nthr);
    // XCD-aware tile order: consecutive workgroup ids land on different XCDs (8 of them, each with its own L2), and a
    // tile reads only TC * 8 bytes of every row -- a quarter of a 64-byte sector at TC = 2.  XCD x therefore walks its own
    // contiguous eighth of the tiles, so that the neighbours sharing a tile's sectors run on the same L2.
    const int nxcd = (gridDim.x % 8 == 0 && ntiles >= 64) ? 8 : 1;
    const int xcd = blockIdx.x % nxcd, jx = blockIdx.x / nxcd, gx = gridDim.x / nxcd;
    const int t8 = (ntiles + nxcd - 1) / nxcd, tend = min(ntiles, (xcd + 1) * t8);
    for (int t = xcd * t8 + jx; t < tend; t += gx) {
        const int q = t / ntx, p0 = (t - q * ntx) * TC;
        const int ncol = min(TC, d.M - p0);
        float2* base = data + ((size_t)q * d.C2) * d.M + p0;
        for (int w = tid; w < ntile; w += nthr) {
            const int c2 = w / TC, tt = w - c2 * TC;
            float2 v = make_float2(0.f, 0.f);
            if (w < nelem && tt < ncol) {
                const float2 ch = P.bs_chirp[c2];
                v = INV ? c_mulc(base[(size_t)c2 * d.M + tt], ch) : c_mul(base[(size_t)c2 * d.M + tt], ch);
            }
            tile[w] = v;
        }
        lds_barrier();
        lds_fft<false, true, false>(tile, P.ax_bs, tw, TC, TC, 1, 1, 0, tid, nthr);
        for (int w = tid; w < ntile; w += nthr) {
            const float2 f = P.bs_filt[w / TC];
            tile[w] = INV ? c_mulc(tile[w], f) : c_mul(tile[w], f);
        }
        lds_barrier();
        lds_fft<true, true, false>(tile, P.ax_bs, tw, TC, TC, 1, 1, 0, tid, nthr);
        for (int w = tid; w < nelem; w += nthr) {
            const int c2 = w / TC, tt = w - c2 * TC;
            if (tt < ncol) {
                const float2 ch = P.bs_chirp[c2];
                base[(size_t)c2 * d.M + tt] = INV ? c_mulc(tile[w], ch) : c_mul(tile[w], ch);
            }
        }
        lds_barrier();
    }
}

// Time-first order (fk_tf.h) when the c2 axis is a Bluestein convolution: passes C and C' fused on the BAND strips of the
// compact spectrum W -- chirp, FFT_L, x filter, IFFT_L, chirp (= the c2 transform, natural order), x band mask, and the same
// backwards with conjugated tables -- one read and one write of the strip for four length-L transforms.  Tile order as
// fkf_passCm: per c1 position q the band strips of the N1 sub-row blocks, then the Nyquist strip.
__global__ __launch_bounds__(kMaxThreads) void fk_passCm_bluestein(FkDev P, FkTfDev T, int ntiles) {
    D4W_DYN_LDS(smem_raw);
    float2* tile = reinterpret_cast<float2*>(smem_raw);
    const FkDims& d = P.d;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int TC = d.TC, L = P.bs_L;
    const int nelem = d.C2 * TC, ntile = L * TC;
    const TwLds tw = tw_stage(P.ax_bs, tile + ntile, tid, nthr);
    const int nb1 = T.bw / TC, tq = d.N1 * nb1 + (T.col_nyq >= 0 ? 1 : 0);
    const size_t LC = (size_t)T.Lc;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int q = t / tq, u = t - q * tq;
        int p0;
        if (u < d.N1 * nb1) {
            const int q1 = u / nb1;
            p0 = q1 * T.RW + (u - q1 * nb1) * TC;
        } else
            p0 = T.col_nyq;
        float2* base = T.W + ((size_t)q * d.C2) * LC + p0;
        const float* mbase = T.cmask + ((size_t)q * d.C2) * LC + p0;
        for (int w = tid; w < ntile; w += nthr) {
            const int c2 = w / TC, tt = w - c2 * TC;
            tile[w] = (w < nelem) ? c_mul(base[(size_t)c2 * LC + tt], P.bs_chirp[c2]) : make_float2(0.f, 0.f);
        }
        lds_barrier();
        lds_fft<false, true, false>(tile, P.ax_bs, tw, TC, TC, 1, 1, 0, tid, nthr);
        for (int w = tid; w < ntile; w += nthr) tile[w] = c_mul(tile[w], P.bs_filt[w / TC]);
        lds_barrier();
        lds_fft<true, true, false>(tile, P.ax_bs, tw, TC, TC, 1, 1, 0, tid, nthr);
        // spectrum at wavenumber position c2 (natural order): x chirp x mask, then straight into the inverse convolution
        // (x conj chirp); everything beyond the C2 rows is the zero padding again
        for (int w = tid; w < ntile; w += nthr) {
            const int c2 = w / TC, tt = w - c2 * TC;
            float2 v = make_float2(0.f, 0.f);
            if (w < nelem) {
                const float2 ch = P.bs_chirp[c2];
                v = c_mulc(c_scale(c_mul(tile[w], ch), mbase[(size_t)c2 * LC + tt]), ch);
            }
            tile[w] = v;
        }
        lds_barrier();
        lds_fft<false, true, false>(tile, P.ax_bs, tw, TC, TC, 1, 1, 0, tid, nthr);
        for (int w = tid; w < ntile; w += nthr) tile[w] = c_mulc(tile[w], P.bs_filt[w / TC]);
        lds_barrier();
        lds_fft<true, true, false>(tile, P.ax_bs, tw, TC, TC, 1, 1, 0, tid, nthr);
        for (int w = tid; w < nelem; w += nthr) {
            const int c2 = w / TC, tt = w - c2 * TC;
            base[(size_t)c2 * LC + tt] = c_mulc(tile[w], P.bs_chirp[c2]);
        }
        lds_barrier();
    }
}

// ---------------------------------------------------------------------------------------------
// pass B : contiguous n2 transform + real-spectrum pair op + mask + inverse
//
// For packed element a = (k, f), f = k1 + N1*k2 in [0, M), with partner b = (-k, (M - f) mod M):
//   A = Z[a], B = conj(Z[b]);  E = (A+B)/2 (even-sample spectrum), O = -i (A-B)/2 (odd-sample)
//   X(k, f)   = E + W O,  X(k, f+M) = E - W O,  W = exp(-2 pi i f / ns)
//   Y+ = M_h(k, f) X(k, f),  Y- = M_h(k, f+M) X(k, f+M),  M_h(k, f+M) = M_h(-k, M-f) (Nyquist
//   column M_h(k, M) when f = 0)
//   Zy[a] = S + D,  Zy[b] = conj(S - D),  S = (Y+ + Y-)/2,  D = i conj(W) (Y+ - Y-)/2.
// Work list: P.pairs[t] = (keyA, keyB), key = row position * N1 + q1, keyA <= keyB, each
// Hermitian pair of sub-rows exactly once (keyA == keyB for the self-paired ones).
// ---------------------------------------------------------------------------------------------
template <bool GENERIC>
__global__ __launch_bounds__(kMaxThreads) void fk_passB(FkDev P, float2* __restrict__ data, int npairs) {
    D4W_DYN_LDS(smem_raw);
    float2* tile = reinterpret_cast<float2*>(smem_raw);
    const FkDims& d = P.d;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int N2 = d.N2;
    const TwLds tw = tw_stage(P.ax_n2, tile + 2 * N2, tid, nthr);
    float2 pf[kPF];
    auto issue = [&](int t) {
        const int2 pr = P.pairs[t];
        const float2* rowA = data + (size_t)pr.x * N2;
        const float2* rowB = data + (size_t)pr.y * N2;
        const int nload = (pr.x == pr.y) ? N2 : 2 * N2;
#pragma unroll
        for (int it = 0; it < kPF; ++it) {
            const int w = tid + it * nthr;
            float2 v = make_float2(0.f, 0.f);
            if (w < nload) v = (w < N2) ? rowA[w] : rowB[w - N2];
            pf[it] = v;
        }
    };
    int t = blockIdx.x;
    if (t < npairs) issue(t);
    while (t < npairs) {
        const int2 pr = P.pairs[t];
        const bool same = (pr.x == pr.y);
        const int nload = same ? N2 : 2 * N2;
#pragma unroll
        for (int it = 0; it < kPF; ++it) {
            const int w = tid + it * nthr;
            if (w < nload) tile[w] = pf[it];
        }
        lds_barrier();
        const int next = t + gridDim.x;
        if (next < npairs) issue(next);
        float2* A = tile;
        float2* B = same ? tile : tile + N2;
        const int nrows = same ? 1 : 2;
        lds_fft<false, false, GENERIC>(tile, P.ax_n2, tw, 1, nrows, N2, 1, 0, tid, nthr);

        const int r = pr.x / d.N1, q1 = pr.x - r * d.N1;
        const bool k1zero = (q1 == 0);
        const float* mA = P.mask + (size_t)pr.x * N2;
        const float* mB = P.mask + (size_t)pr.y * N2;
        const float2 wr = P.wrow[q1];
        const float nyq = P.nyq[r];
        for (int i = tid; i < N2; i += nthr) {
            const int j = k1zero ? P.mirror0[i] : (N2 - 1 - i);
            if (same && j < i) continue;
            const float2 a = A[i];
            const float2 Bc = c_conj(B[j]);
            const float ma = mA[i];
            const float mb = (k1zero && i == 0) ? nyq : mB[j];
            const float2 w = c_mul(wr, P.wcol[i]);
            const float2 E = c_scale(c_add(a, Bc), 0.5f);
            const float2 O = c_mul_mi(c_scale(c_sub(a, Bc), 0.5f));
            const float2 tO = c_mul(w, O);
            const float2 Yp = c_scale(c_add(E, tO), ma);
            const float2 Ym = c_scale(c_sub(E, tO), mb);
            const float2 S = c_scale(c_add(Yp, Ym), 0.5f);
            const float2 D = c_mul_pi(c_mulc(c_scale(c_sub(Yp, Ym), 0.5f), w));
            A[i] = c_add(S, D);
            B[j] = c_conj(c_sub(S, D));
        }
        lds_barrier();
        lds_fft<true, false, GENERIC>(tile, P.ax_n2, tw, 1, nrows, N2, 1, 0, tid, nthr);
        float2* rowA = data + (size_t)pr.x * N2;
        float2* rowB = data + (size_t)pr.y * N2;
        for (int w = tid; w < nload; w += nthr) {
            if (w < N2) rowA[w] = tile[w];
            else rowB[w - N2] = tile[w];
        }
        lds_barrier();
        t = next;
    }
}

// pass B when N2 has a prime factor > 31: the n2 sub-transforms of the row pair run as Bluestein convolutions of
// length bn_L inside the tile (see fk_passC_bluestein), spectra in NATURAL order (the plan's position -> frequency
// tables of the n2 axis are the identity, so the pair op below is fk_passB's, table for table).
__global__ __launch_bounds__(kMaxThreads) void fk_passB_bluestein(FkDev P, float2* __restrict__ data, int npairs) {
    D4W_DYN_LDS(smem_raw);
    float2* tile = reinterpret_cast<float2*>(smem_raw);
    const FkDims& d = P.d;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int N2 = d.N2, L = P.bn_L;
    const TwLds tw = tw_stage(P.ax_bn, tile + 2 * L, tid, nthr);
    for (int t = blockIdx.x; t < npairs; t += gridDim.x) {
        const int2 pr = P.pairs[t];
        const bool same = (pr.x == pr.y);
        const int nrows = same ? 1 : 2;
        float2* rowA = data + (size_t)pr.x * N2;
        float2* rowB = data + (size_t)pr.y * N2;
        for (int w = tid; w < nrows * L; w += nthr) {
            const int r = w / L, n = w - r * L;
            tile[w] = (n < N2) ? c_mul((r ? rowB : rowA)[n], P.bn_chirp[n]) : make_float2(0.f, 0.f);
        }
        lds_barrier();
        lds_fft<false, false, false>(tile, P.ax_bn, tw, 1, nrows, L, 1, 0, tid, nthr);
        for (int w = tid; w < nrows * L; w += nthr) tile[w] = c_mul(tile[w], P.bn_filt[w % L]);
        lds_barrier();
        lds_fft<true, false, false>(tile, P.ax_bn, tw, 1, nrows, L, 1, 0, tid, nthr);
        for (int w = tid; w < nrows * N2; w += nthr) {
            const int r = w / N2, k = w - r * N2;
            tile[r * L + k] = c_mul(tile[r * L + k], P.bn_chirp[k]);
        }
        lds_barrier();
        // ---- pair op x mask (fk_passB)
        float2* A = tile;
        float2* B = same ? tile : tile + L;
        const int r = pr.x / d.N1, q1 = pr.x - r * d.N1;
        const bool k1zero = (q1 == 0);
        const float* mA = P.mask + (size_t)pr.x * N2;
        const float* mB = P.mask + (size_t)pr.y * N2;
        const float2 wr = P.wrow[q1];
        const float nyq = P.nyq[r];
        for (int i = tid; i < N2; i += nthr) {
            const int j = k1zero ? P.mirror0[i] : (N2 - 1 - i);
            if (same && j < i) continue;
            const float2 a = A[i];
            const float2 Bc = c_conj(B[j]);
            const float ma = mA[i];
            const float mb = (k1zero && i == 0) ? nyq : mB[j];
            const float2 w = c_mul(wr, P.wcol[i]);
            const float2 E = c_scale(c_add(a, Bc), 0.5f);
            const float2 O = c_mul_mi(c_scale(c_sub(a, Bc), 0.5f));
            const float2 tO = c_mul(w, O);
            const float2 Yp = c_scale(c_add(E, tO), ma);
            const float2 Ym = c_scale(c_sub(E, tO), mb);
            const float2 S = c_scale(c_add(Yp, Ym), 0.5f);
            const float2 D = c_mul_pi(c_mulc(c_scale(c_sub(Yp, Ym), 0.5f), w));
            A[i] = c_add(S, D);
            B[j] = c_conj(c_sub(S, D));
        }
        lds_barrier();
        // ---- inverse n2 transforms (conjugate chirp and filter), zero padding restored first
        for (int w = tid; w < nrows * L; w += nthr) {
            const int rr = w / L, n = w - rr * L;
            tile[w] = (n < N2) ? c_mulc(tile[w], P.bn_chirp[n]) : make_float2(0.f, 0.f);
        }
        lds_barrier();
        lds_fft<false, false, false>(tile, P.ax_bn, tw, 1, nrows, L, 1, 0, tid, nthr);
        for (int w = tid; w < nrows * L; w += nthr) tile[w] = c_mulc(tile[w], P.bn_filt[w % L]);
        lds_barrier();
        lds_fft<true, false, false>(tile, P.ax_bn, tw, 1, nrows, L, 1, 0, tid, nthr);
        for (int w = tid; w < nrows * N2; w += nthr) {
            const int rr = w / N2, k = w - rr * N2;
            (rr ? rowB : rowA)[k] = c_mulc(tile[rr * L + k], P.bn_chirp[k]);
        }
        lds_barrier();
    }
}

// ---------------------------------------------------------------------------------------------
// mask fold + permutation into pass-B order (one-off per mask)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void fk_fold_mask(FkDims d, const float* __restrict__ ms,
                                                          const int* __restrict__ rowk,
                                                          const int* __restrict__ k1_of_q1,
                                                          const int* __restrict__ k2_of_i,
                                                          float* __restrict__ mask,
                                                          float* __restrict__ nyq, unsigned* __restrict__ rowmaxbits, FkAffine aff) {
    const int r = blockIdx.y;
    const int k = rowk[r];
    const int km = (d.nx - k) % d.nx;
    const int sx = d.nx / 2, st = d.ns / 2;
    const size_t rowp = (size_t)((k + sx) % d.nx) * d.ns;    // shifted-grid row of +k
    const size_t rowm = (size_t)((km + sx) % d.nx) * d.ns;   // shifted-grid row of -k
    unsigned vbits = 0u;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < d.M; p += gridDim.x * blockDim.x) {
        const int q1 = p / d.N2, i = p - q1 * d.N2;
        const int f = k1_of_q1[q1] + d.N1 * k2_of_i[i];
        const int fm = (d.ns - f) % d.ns;
        const float v = 0.5f * (aff(ms[rowp + (f + st) % d.ns]) + aff(ms[rowm + (fm + st) % d.ns]));
        mask[(size_t)r * d.M + p] = v;
        vbits = max(vbits, __float_as_uint(v) & 0x7fffffffu);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int f = d.M, fm = d.ns - d.M;
        const float v = 0.5f * (aff(ms[rowp + (f + st) % d.ns]) + aff(ms[rowm + (fm + st) % d.ns]));
        nyq[r] = v;
        vbits = max(vbits, __float_as_uint(v) & 0x7fffffffu);
    }
    if (vbits) atomicMax(rowmaxbits + r, vbits);
}

// The same fold with the mask evaluated in closed form (design_eval.h) instead of read: a reference design goes
// straight into pass-B order and no dense [nx][ns] mask exists (9.6 GB at 20 000 x 120 000).  Each of the two
// values is rounded to float32 before the average exactly as the dense design kernel stores it, so the folded
// mask is bit-identical to design + fold.
__global__ __launch_bounds__(kThreads) void fk_fold_design(FkDims d, DesignArgs A, int mode,
                                                            const int* __restrict__ rowk,
                                                            const int* __restrict__ k1_of_q1,
                                                            const int* __restrict__ k2_of_i,
                                                            float* __restrict__ mask,
                                                            float* __restrict__ nyq, unsigned* __restrict__ rowmaxbits) {
    const int r = blockIdx.y;
    const int k = rowk[r];
    const int km = (d.nx - k) % d.nx;
    const int sx = d.nx / 2, st = d.ns / 2;
    const int ip = (k + sx) % d.nx, im = (km + sx) % d.nx;
    unsigned vbits = 0u;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < d.M; p += gridDim.x * blockDim.x) {
        const int q1 = p / d.N2, i = p - q1 * d.N2;
        const int f = k1_of_q1[q1] + d.N1 * k2_of_i[i];
        const int fm = (d.ns - f) % d.ns;
        const float v = design_folded(A, mode, ip, (f + st) % d.ns, im, (fm + st) % d.ns);
        mask[(size_t)r * d.M + p] = v;
        vbits = max(vbits, __float_as_uint(v) & 0x7fffffffu);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int f = d.M, fm = d.ns - d.M;
        const float v = design_folded(A, mode, ip, (f + st) % d.ns, im, (fm + st) % d.ns);
        nyq[r] = v;
        vbits = max(vbits, __float_as_uint(v) & 0x7fffffffu);
    }
    if (vbits) atomicMax(rowmaxbits + r, vbits);
}

constexpr int kFoldThreads = 1024;   // 16 waves per workgroup: the tile's loads are latency-bound with fewer in flight
// The same fold with both sides of the permutation coalesced (the gather above reads 4 useful bytes per 64-byte
// sector: 178 GB of traffic and 23 ms at 20000 x 120000).  The first radix R0 of the n2 transform carries the LOWEST
// digit d0 of k2 and the HIGHEST of the position: k2 = d0 + R0 k2'(i'), i = d0 (N2 / R0) + i'.  So for one i' the
// frequencies f = k1 + N1 k2 over all (k1, d0) form ONE contiguous run of RL = N1 R0 samples of the mask row
// (and a reversed run of the partner row), and for one (k1, d0) the positions of IB consecutive i' are contiguous.
// Tile = (row r, all k1, all d0, IB consecutive i'): runs in, LDS transpose [RL][IB + 1], runs out.
// Also leaves max |M_h| of every row (Nyquist column included) in rowmaxbits -- liveness and the opt-in tail pruning.
__global__ __launch_bounds__(kFoldThreads) void fk_fold_mask_tiled(FkDims d, int R0, int IB, const float* __restrict__ ms,
                                                                const int* __restrict__ rowk,
                                                                const int* __restrict__ q1_of_k1,
                                                                const int* __restrict__ k2_of_i,
                                                                float* __restrict__ mask, float* __restrict__ nyq,
                                                                unsigned* __restrict__ rowmaxbits, FkAffine aff) {
    D4W_DYN_LDS(smem_raw);
    float* buf = reinterpret_cast<float*>(smem_raw);
    const int r = blockIdx.y;
    const int k = rowk[r];
    const int km = (d.nx - k) % d.nx;
    const int sx = d.nx / 2, st = d.ns / 2;
    const float* rowp = ms + (size_t)((k + sx) % d.nx) * d.ns + st;    // + f : M(+k, f),  0 <= f < M
    const float* rowm = ms + (size_t)((km + sx) % d.nx) * d.ns + st;   // - f : M(-k, -f)
    const int RL = d.N1 * R0, N2r = d.N2 / R0, pitch = IB + 1;
    const int ib0 = blockIdx.x * IB, nb = min(IB, N2r - ib0);
    // max |M_h| as the bit pattern of |v|: unsigned order = value order, and a NaN gain (above +inf) keeps its
    // row alive like NumPy would
    unsigned vbits = 0u;
    const FDiv dRL(RL);
#pragma unroll 4
    for (int w = threadIdx.x; w < RL * nb; w += blockDim.x) {
        const int j = dRL.div(w), u = w - j * RL;
        const int f = u + RL * (k2_of_i[ib0 + j] / R0);
        const float v = 0.5f * (aff(rowp[f]) + aff(rowm[-f]));
        vbits = max(vbits, __float_as_uint(v) & 0x7fffffffu);
        buf[u * pitch + j] = v;
    }
    __syncthreads();
    const FDiv dnb(nb), dN1(d.N1);
#pragma unroll 4
    for (int w = threadIdx.x; w < RL * nb; w += blockDim.x) {
        const int u = dnb.div(w), j = w - u * nb;
        const int d0 = dN1.div(u), k1 = u - d0 * d.N1;
        mask[(size_t)r * d.M + (size_t)q1_of_k1[k1] * d.N2 + d0 * N2r + ib0 + j] = buf[u * pitch + j];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const float v = 0.5f * (aff(rowp[d.M - d.ns]) + aff(rowm[d.M - d.ns]));   // f = M (Nyquist): shifted column 0 of both rows
        nyq[r] = v;
        vbits = max(vbits, __float_as_uint(v) & 0x7fffffffu);
    }
    for (int off = 32; off >= 1; off >>= 1) vbits = max(vbits, __shfl_xor(vbits, off));
    if ((threadIdx.x & 63) == 0 && vbits) atomicMax(rowmaxbits + r, vbits);
}

// Column statistics of the folded mask (time-first order, fk_tf.h): min and max over all wavenumber rows of every
// half-spectrum column, as order-preserving unsigned keys (a NaN gain lands above +inf in the max key).  One thread per
// column position (coalesced along the row), row chunks combined by atomics.
__device__ __forceinline__ unsigned fk_ord_key(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(kThreads) void fk_col_minmax(FkDims d, const float* __restrict__ mask, int rows_per_block,
                                                           unsigned* __restrict__ kmin, unsigned* __restrict__ kmax) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= d.M) return;
    const int r0 = blockIdx.y * rows_per_block, r1 = min(d.nx, r0 + rows_per_block);
    unsigned lo = 0xFFFFFFFFu, hi = 0u;
    for (int r = r0; r < r1; ++r) {
        const unsigned k = fk_ord_key(mask[(size_t)r * d.M + p]);
        lo = min(lo, k);
        hi = max(hi, k);
    }
    if (r1 > r0) {
        atomicMin(kmin + p, lo);
        atomicMax(kmax + p, hi);
    }
}

// Band columns of the folded mask in the compact column order of the time-first passes: cmask[r][col] = mask[r][src[col]]
// (src = -2: the Nyquist column nyq[r]; -1: padding).
__global__ __launch_bounds__(kThreads) void fk_gather_cmask(FkDims d, const float* __restrict__ mask, const float* __restrict__ nyq,
                                                             const int* __restrict__ src, int Lband, float* __restrict__ cmask) {
    const int r = blockIdx.y;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < Lband; c += gridDim.x * blockDim.x) {
        const int sp = src[c];
        cmask[(size_t)r * Lband + c] = (sp >= 0) ? mask[(size_t)r * d.M + sp] : (sp == -2 ? nyq[r] : 0.f);
    }
}

// Liveness words of pass Cm (fk_tf.h): for tile (q, strip p0 .. p0 + TC) and radix-RB item g, bit b = the band mask of row
// q C2 + g RB + b has a non-zero (or NaN) value in the strip.  One thread per (tile, g).
__global__ __launch_bounds__(kThreads) void fk_cm_livebits(const float* __restrict__ cmask, int Lc, int C2, int RA, int RB, int TC, int N1,
                                                            int nb1, int RW, int col_nyq, int ntiles, unsigned* __restrict__ live) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ntiles * RA) return;
    const int t = i / RA, g = i - t * RA;
    const int tq = N1 * nb1 + (col_nyq >= 0 ? 1 : 0);
    const int q = t / tq, u = t - q * tq;
    int p0;
    if (u < N1 * nb1) {
        const int q1 = u / nb1;
        p0 = q1 * RW + (u - q1 * nb1) * TC;
    } else
        p0 = col_nyq;
    unsigned bits = 0u;
    for (int b = 0; b < RB; ++b) {
        const float* mp = cmask + ((size_t)q * C2 + (size_t)g * RB + b) * Lc + p0;
        bool any = false;
        for (int c = 0; c < TC; ++c) any |= !(mp[c] == 0.f);
        if (any) bits |= 1u << b;
    }
    live[i] = bits;
}

// x[c][n] *= tukey(ns, 0.03)[n] in place (dsp.taper_data, dsp.py:705-722).  The window is exactly 1 between its two cosine
// ramps -- 1.5 % of the row at each end -- and x * 1.0f is x: only the ramps are read and written (W columns at each end,
// ramp[0 .. 2 W) = the window's first and last W values).  Rounds 1-5 multiplied the whole block: 4.5 ms per 20 000 x 120 000
// block for 0.15 ms of work.
__global__ __launch_bounds__(kThreads) void taper_ramps(float* __restrict__ x, const float* __restrict__ ramp, int nx, int ns, int W) {
    const size_t per_row = (size_t)2 * W, total = (size_t)nx * per_row;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t c = i / per_row;
        const int j = (int)(i - c * per_row);
        const int n = (j < W) ? j : ns - 2 * W + j;
        x[c * (size_t)ns + n] *= ramp[j];
    }
}

// shape-specialised kernels: fk_entry.h (FkFastEntry, fast_entry<G>) -- one table entry per instantiated shape
//                 C1  C2A C2B  N1  NA  NB  NC  TA  TC  thrA thrC thrB
// 20000 x 120000: 128-byte column strips in pass C (TC = 16) are worth 3.8 vs 6.9 ms per pass over 64-byte ones
using FkShapeBench = FkFastCfg<25, 25, 32, 25, 20, 12, 10, 16, 16, 448, 512, 256>;
// BASELINE configs[0..1] geometry and the real OOI RAPID channel count (11020 = 20 x 19 x 29: the two
// primes are register butterflies of the c2 axis)
using FkShapeC1 = FkFastCfg<20, 10, 20, 5, 10, 12, 10, 16, 16, 320, 320, 256>;      // 4000 x 12000
using FkShapeOOI = FkFastCfg<20, 19, 29, 5, 10, 12, 10, 16, 16, 320, 464, 256>;     // 11020 x 12000
// the reference notebook's channel selection on the OOI RAPID cable ([20000, 65000, 10] m -> 5510 channels;
// scripts/main_mfdetect.py's [12000, 66000, 5] m gives 13223 = 7 x 1889 channels: Bluestein pass C)
using FkShapeNB = FkFastCfg<10, 19, 29, 5, 10, 12, 10, 16, 16, 192, 464, 256>;      // 5510 x 12000
using FkShapeT1 = FkFastCfg<3, 2, 3, 2, 2, 3, 2, 2, 2, 64, 64, 64>;                 // 18 x 48    (tests)
using FkShapeT2 = FkFastCfg<2, 2, 2, 2, 8, 3, 5, 2, 2, 64, 64, 64>;                 // 8 x 480    (tests)
using FkShapeT3 = FkFastCfg<5, 4, 5, 5, 4, 3, 5, 4, 4, 64, 64, 64>;                 // 100 x 600  (tests)
using FkShapeT4 = FkFastCfg<2, 7, 11, 2, 2, 3, 2, 2, 2, 64, 64, 64>;                // 154 x 48   (tests: prime butterflies 7, 11)
using FkShapeT5 = FkFastCfg<2, 19, 29, 2, 2, 3, 2, 2, 2, 64, 64, 64>;               // 1102 x 48  (tests: the OOI shapes' radices 19, 29)

// shape configurations registered at run time (compiled on demand, das4whales_amd/fkjit.py); entries are never removed
static std::mutex g_dyn_mu;
static std::vector<FkFastEntry*>& dyn_shapes() {
    static std::vector<FkFastEntry*> v;
    return v;
}

static const std::vector<FkFastEntry>& fast_shapes() {
    static const std::vector<FkFastEntry> v = {
        fast_entry<FkShapeBench>(1, 1, 2),
        fast_entry<FkShapeC1>(2, 2, 2),
        fast_entry<FkShapeOOI>(2, 2, 2),
        fast_entry<FkShapeNB>(2, 2, 2),
        fast_entry<FkShapeT1>(2, 2, 2),
        fast_entry<FkShapeT2>(2, 2, 2),
        fast_entry<FkShapeT3>(2, 2, 2),
        fast_entry<FkShapeT4>(2, 2, 2),
        fast_entry<FkShapeT5>(2, 2, 2),
    };
    return v;
}

// ---------------------------------------------------------------------------------------------
// host launchers of the generic pass kernels (fk_plan.h): the one place that picks an instantiation.  FAST kernels
// carry only the unrolled radices; GENERIC ones add the loop-based primes.
// ---------------------------------------------------------------------------------------------
int fk_launch_passA_fwd(bool taper, bool generic, dim3 grid, dim3 blk, size_t lds, void* stream, const FkDev& P,
                        const float2* src, float2* dst, int ntiles) {
    auto k = taper ? (generic ? fk_passA_fwd<true, true> : fk_passA_fwd<true, false>)
                   : (generic ? fk_passA_fwd<false, true> : fk_passA_fwd<false, false>);
    return launch_k(k, grid, blk, lds, stream, P, src, dst, ntiles);
}

int fk_launch_passA_inv(bool generic, dim3 grid, dim3 blk, size_t lds, void* stream, const FkDev& P, float2* data, int ntiles) {
    return launch_k(generic ? fk_passA_inv<true> : fk_passA_inv<false>, grid, blk, lds, stream, P, data, ntiles);
}

int fk_launch_passC(bool inv, bool generic, dim3 grid, dim3 blk, size_t lds, void* stream, const FkDev& P, float2* data,
                    int ntiles) {
    auto k = inv ? (generic ? fk_passC<true, true> : fk_passC<true, false>)
                 : (generic ? fk_passC<false, true> : fk_passC<false, false>);
    return launch_k(k, grid, blk, lds, stream, P, data, ntiles);
}

void fk_pass_ac_lds_limit(int bytes) {
    const void* fns[] = {
        (const void*)fk_passA_fwd<true, true>, (const void*)fk_passA_fwd<true, false>,
        (const void*)fk_passA_fwd<false, true>, (const void*)fk_passA_fwd<false, false>,
        (const void*)fk_passA_inv<true>, (const void*)fk_passA_inv<false>,
        (const void*)fk_passC<false, true>, (const void*)fk_passC<false, false>,
        (const void*)fk_passC<true, true>, (const void*)fk_passC<true, false>};
    for (const void* f : fns) (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

void fk_plan_release(d4w_fk_plan* pl) {
    for (void* p : pl->allocs) (void)hipFree(p);
    if (pl->d_cmask) (void)hipFree(pl->d_cmask);
    if (pl->d_W) (void)hipFree(pl->d_W);
    if (pl->apply_done) (void)hipEventDestroy(pl->apply_done);
    if (pl->d_colsrc) (void)hipFree(pl->d_colsrc);
    if (pl->d_cmlive) (void)hipFree(pl->d_cmlive);
}

}  // namespace d4w

using namespace d4w;

extern "C" {

const char* d4w_last_error(void) { return d4w::g_err; }

const char* d4w_version(void) {
    return D4W_BUILD_TAG;
}

/* 1 when the shape runs shape-specialised kernels (built in or registered), 0 when it runs the generic passes */
int d4w_fk_shape_is_specialised(int nx, int ns) {
    for (const FkFastEntry& e : fast_shapes())
        if (e.nx == nx && e.ns == ns) return 1;
    std::lock_guard<std::mutex> lk(g_dyn_mu);
    for (const FkFastEntry* e : dyn_shapes())
        if (e->nx == nx && e->ns == ns) return 1;
    return 0;
}

/* Registers a shape configuration compiled on demand (the caller passes the FkFastEntry its own translation unit
 * built from csrc/fk_entry.h; entry_size guards against a header mismatch). */
int d4w_fk_register_shape(const void* entry, size_t entry_size) {
    if (!entry || entry_size != sizeof(FkFastEntry)) return fail(D4W_EINVAL, "shape entry of %zu bytes, expected %zu (stale build?)", entry_size, sizeof(FkFastEntry));
    FkFastEntry* e = new FkFastEntry(*static_cast<const FkFastEntry*>(entry));
    if (e->nx < 1 || e->ns < 2 || e->C2X < 1 || e->C1 * e->C2A * e->C2B * e->C2X != e->nx || (e->C2X > 1 && e->C2A * e->C2B != 1) ||
        2 * e->N1 * e->NA * e->NB * e->NC != e->ns || e->TA != e->TC) {
        delete e;
        return fail(D4W_EINVAL, "inconsistent shape entry");
    }
    std::lock_guard<std::mutex> lk(g_dyn_mu);
    dyn_shapes().push_back(e);
    return D4W_OK;
}

int d4w_fk_plan_destroy(d4w_fk_plan* pl) {
    if (pl && pl->big) { d4w_fkd_plan_destroy(pl->big); pl->big = nullptr; }
    if (!pl) return D4W_OK;
    fk_plan_release(pl);
    delete pl;
    return D4W_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// host side: planner
// ---------------------------------------------------------------------------------------------
int d4w::fk_plan_build(int nx, int ns, const int* opts, bool alloc_mask, bool fast_only, d4w_fk_plan** out) {
    if (!out) return fail(D4W_EINVAL, "plan pointer is NULL");
    *out = nullptr;
    if (nx < 1 || ns < 2) return fail(D4W_EINVAL, "bad shape %d x %d", nx, ns);
    if (ns % 2) return fail(D4W_EINVAL, "ns = %d must be even (packed real transform)", ns);
    const int M = ns / 2;
    int o[6] = {0, 0, 0, 0, 0, 0};
    if (opts) memcpy(o, opts, sizeof(o));

    // --- shape-specialised kernels (unless the caller pins a tiling or asks for the generic path
    //     with opts[0] = -1 / D4W_FK_GENERIC=1)
    const FkFastEntry* fast = nullptr;
    {
        bool pinned = false;
        for (int i = 0; i < 6; ++i) pinned |= (o[i] != 0);
        if (o[0] < 0) o[0] = 0;                      // -1 = "generic kernels, planner's tiling"
        const char* g = getenv("D4W_FK_GENERIC");
        const char* vs = getenv("D4W_FK_VARIANT");
        const int want = vs ? atoi(vs) : 0;
        if (!pinned && !(g && atoi(g) > 0)) {
            for (const FkFastEntry& e : fast_shapes())
                if (e.nx == nx && e.ns == ns && (e.variant == want || (!fast && e.variant == 0))) fast = &e;
            if (!fast) {
                std::lock_guard<std::mutex> lk(g_dyn_mu);
                for (const FkFastEntry* e : dyn_shapes())
                    if (e->nx == nx && e->ns == ns) fast = e;
            }
        }
    }
    if (fast_only && !fast) return fail(D4W_EINVAL, "no shape-specialised kernels for %d x %d", nx, ns);
    // An axis whose part with prime factors > 31 does not fit the Bluestein tiles of passes C / B: the global-memory forms
    // (fkd_bz_* / fkd_bt_*) of the generic distributed plan at world 1, behind this plan's entry points
    auto make_big = [&]() -> int {
        d4w_fkd_plan* big = nullptr;
        int rcb = fkd_plan_build(nx, ns, 1, 0, true, &big);
        if (rcb) return rcb;
        int info[12];
        (void)d4w_fkd_plan_info(big, info);
        d4w_fk_plan* bp = new d4w_fk_plan();
        memset(&bp->dev, 0, sizeof(bp->dev));
        bp->dev.d = FkDims{nx, ns, M, info[9], info[10], info[6], info[7], 1, 1};
        bp->big = big;
        bp->live_rows = nx;
        *out = bp;
        return D4W_OK;
    };
    // A prime factor > 31 of ns / 2 goes into N2, whose sub-transforms (pass B) then run as Bluestein convolutions of
    // length bn_L = 2^a 3^b 5^c >= 2 N2 - 1 inside the tile (two rows of bn_L); N1 keeps the smooth part.
    int bn_L = 0, bn_N2 = 0;
    if (!fast && rough_part(M) > 1) {
        bn_N2 = rough_part(M);
        bn_L = smooth_len_235(2L * bn_N2 - 1);
        if (2L * bn_L > kMaxTile) return make_big();
    }
    // admissible time splits: N1 | M with N2 = M / N1 fitting one LDS row pair
    int n1_min = 0;
    for (int cand = 1; cand <= M && !n1_min; ++cand)
        if (M % cand == 0 && M / cand <= kMaxTile / 2) n1_min = cand;
    if (bn_L) n1_min = M / bn_N2;
    if (!n1_min) return fail(D4W_EINVAL, "ns/2 = %d has no factorisation with N2 <= %d", M, kMaxTile / 2);
    // --- split the channel axis
    int C1 = o[0], C2 = o[1];
    if (C1 <= 0 || C2 <= 0 || C1 * C2 != nx) {
        // measured on MI355X (20000 x 120000): a long c2 axis with 64-byte column segments in
        // pass C leaves room for 128-byte segments in the 2-D pass A and wins overall
        C2 = largest_divisor_le(nx, kMaxTile / 8);
        // ... but not at the price of fewer than 8 c1 rows: pass A's tile is C1 x N1 x TA, and a tile of a few
        // dozen elements costs more than a shorter c2 axis saves (1000 x 12000: C1 = 1 1.9 ms, C1 = 10 0.47 ms)
        if (nx / C2 < 8)
            for (int cand = C2; cand >= 1; --cand)
                if (nx % cand == 0 && nx / cand >= 8) { C2 = cand; break; }
        C1 = nx / C2;
    }
    // a prime factor > 31 of nx goes into C2, whose sub-transform then runs as a Bluestein convolution of
    // length bs_L (pass C); C1 keeps the smooth part
    int bs_L = 0;
    if (fast && fast->C2X > 1) {                       // specialised passes A and B around the generic Bluestein pass C
        C2 = fast->C2X;
        C1 = nx / C2;
        bs_L = smooth_len_235(2L * C2 - 1);
        if (bs_L > kMaxTile) return fail(D4W_EINVAL, "registered configuration: Bluestein factor %d too long", C2);
    }
    if (!fast && rough_part(nx) > 1) {
        C2 = rough_part(nx);
        C1 = nx / C2;
        for (int f = 2; f <= 31 && (long)C1 * n1_min > kMaxTile; ++f)      // pass A's tile must hold C1 x N1 columns
            while (C1 % f == 0 && (long)C1 * n1_min > kMaxTile && 2L * C2 * f - 1 <= kMaxTile) { C2 *= f; C1 /= f; }
        bs_L = smooth_len_235(2L * C2 - 1);
        if (bs_L > kMaxTile) {
            // too long for the Bluestein tile of pass C: the global-memory form
            return make_big();
        }
    }
    // --- split the time axis.  Pass A's cost falls like 1 / (C1 N1) until its tile holds ~100 columns, pass B's
    //     grows with N1 (shorter rows): N1 ~ sqrt(1000 / C1), at least the smallest admissible one
    //     (measured at 1000 x 12000 and 500 x 120000 over C1 = 1..10, N1 = 2..75)
    int N1 = o[2], N2 = o[3];
    if (bn_L) {
        // smooth factors move from N1 into N2 while the Bluestein tile allows it and pass A's tile needs it
        N1 = M / bn_N2; N2 = bn_N2;
        for (int f = 2; f <= 31 && (long)C1 * N1 > kMaxTile; ++f)
            while (N1 % f == 0 && (long)C1 * N1 > kMaxTile && 2L * (2L * N2 * f - 1) <= kMaxTile) { N2 *= f; N1 /= f; }
        bn_L = smooth_len_235(2L * N2 - 1);
        if (2L * bn_L > kMaxTile || (long)C1 * N1 > kMaxTile) return make_big();
    } else if (N1 <= 0 || N2 <= 0 || N1 * N2 != M) {
        N1 = n1_min;
        const double target = sqrt(1000.0 / (double)C1);
        double best = fabs(log((double)N1 / target));
        if (target > n1_min)
            for (int cand = n1_min + 1; cand <= M && cand <= 4 * target; ++cand) {
                if (M % cand || M / cand < 64 || (long)C1 * cand * 16 > kMaxTile) continue;
                const double sc = fabs(log((double)cand / target));
                if (sc < best) { best = sc; N1 = cand; }
            }
        N2 = M / N1;
    }
    int TC = o[5] > 0 ? o[5] : 16;
    while (TC > 1 && (long)(bs_L ? bs_L : C2) * TC > (bs_L ? kMaxTileBs : kMaxTile)) TC /= 2;
    int TA = o[4] > 0 ? o[4] : 16;
    while (TA > 1 && (long)C1 * N1 * TA > kMaxTile) TA /= 2;
    std::vector<int> r_c1, r_c2, r_n1, r_n2;
    if (fast) {
        C1 = fast->C1; C2 = fast->C2A * fast->C2B * fast->C2X; N1 = fast->N1; N2 = fast->NA * fast->NB * fast->NC;
        TA = fast->TA;
        if (!bs_L) TC = fast->TC;                       // Bluestein pass C keeps its own strip width
        r_c1 = {C1}; r_c2 = {fast->C2A, fast->C2B}; r_n1 = {N1}; r_n2 = {fast->NA, fast->NB, fast->NC};
    }
    if (!fast && ((long)(bs_L ? bs_L : C2) * TC > (bs_L ? kMaxTileBs : kMaxTile) || (long)C1 * N1 * TA > kMaxTile || 2L * (bn_L ? bn_L : N2) > kMaxTile))
        return fail(D4W_EINVAL, "shape %d x %d does not fit the LDS tiling (C1=%d C2=%d N1=%d N2=%d)",
                    nx, ns, C1, C2, N1, N2);

    d4w_fk_plan* pl = new d4w_fk_plan();
    memset(&pl->dev, 0, sizeof(pl->dev));
    FkDims& d = pl->dev.d;
    d = FkDims{nx, ns, M, C1, C2, N1, N2, TA, TC};
    pl->dev.scale = (float)(1.0 / ((double)nx * (double)M));
    int rc;
    std::vector<int> f_c1, f_c2, f_n1, f_n2;
#define D4W_TRY(x) do { rc = (x); if (rc != D4W_OK) { d4w_fk_plan_destroy(pl); return rc; } } while (0)
    pl->fast = fast;
    D4W_TRY(make_axis(pl, C1, &pl->dev.ax_c1, &f_c1, fast ? &r_c1 : nullptr));
    if (bs_L) {
        std::vector<int> one, f_L;
        D4W_TRY(make_axis(pl, 1, &pl->dev.ax_c2, &one));                      // unused: pass C runs fk_passC_bluestein
        D4W_TRY(make_axis(pl, bs_L, &pl->dev.ax_bs, &f_L));
        f_c2.resize(C2);
        for (int i = 0; i < C2; ++i) f_c2[i] = i;                             // natural output order
        std::vector<float2> chirp(C2), filt(bs_L);
        std::vector<double> bre(bs_L, 0.0), bim(bs_L, 0.0);
        for (int n = 0; n < C2; ++n) {
            const double ph = M_PI * (double)(((long long)n * n) % (2LL * C2)) / (double)C2;
            chirp[n] = make_float2((float)cos(ph), (float)-sin(ph));
            bre[n] = cos(ph); bim[n] = sin(ph);                               // conj(chirp)
            if (n) { bre[bs_L - n] = cos(ph); bim[bs_L - n] = sin(ph); }
        }
        host_dft_any(bre, bim);
        for (int p = 0; p < bs_L; ++p)
            filt[p] = make_float2((float)(bre[f_L[p]] / bs_L), (float)(bim[f_L[p]] / bs_L));
        D4W_TRY(upload(pl, chirp, &pl->dev.bs_chirp));
        D4W_TRY(upload(pl, filt, &pl->dev.bs_filt));
        pl->dev.bs_L = bs_L;
    } else
        D4W_TRY(make_axis(pl, C2, &pl->dev.ax_c2, &f_c2, fast ? &r_c2 : nullptr));
    D4W_TRY(make_axis(pl, N1, &pl->dev.ax_n1, &f_n1, fast ? &r_n1 : nullptr));
    if (bn_L) {
        std::vector<int> one, f_L;
        D4W_TRY(make_axis(pl, 1, &pl->dev.ax_n2, &one));                      // unused: pass B runs fk_passB_bluestein
        D4W_TRY(make_axis(pl, bn_L, &pl->dev.ax_bn, &f_L));
        f_n2.resize(N2);
        for (int i = 0; i < N2; ++i) f_n2[i] = i;                             // natural output order
        std::vector<float2> chirp(N2), filt(bn_L);
        std::vector<double> bre(bn_L, 0.0), bim(bn_L, 0.0);
        for (int n = 0; n < N2; ++n) {
            const double ph = M_PI * (double)(((long long)n * n) % (2LL * N2)) / (double)N2;
            chirp[n] = make_float2((float)cos(ph), (float)-sin(ph));
            bre[n] = cos(ph); bim[n] = sin(ph);                               // conj(chirp)
            if (n) { bre[bn_L - n] = cos(ph); bim[bn_L - n] = sin(ph); }
        }
        host_dft_any(bre, bim);
        for (int p = 0; p < bn_L; ++p)
            filt[p] = make_float2((float)(bre[f_L[p]] / bn_L), (float)(bim[f_L[p]] / bn_L));
        D4W_TRY(upload(pl, chirp, &pl->dev.bn_chirp));
        D4W_TRY(upload(pl, filt, &pl->dev.bn_filt));
        pl->dev.bn_L = bn_L;
    } else
        D4W_TRY(make_axis(pl, N2, &pl->dev.ax_n2, &f_n2, fast ? &r_n2 : nullptr));
    if (fast) {     // exchange-stage twiddles of the specialised kernels
        const int RA = fast->C2A, RB = fast->C2B, M1 = fast->NB * fast->NC;
        std::vector<float2> twC((size_t)RA * RB), twB1(M1), twB2(M1);
        for (int a = 0; a < RA; ++a)
            for (int j = 0; j < RB; ++j) twC[(size_t)a * RB + j] = wexp((long long)j * a, C2);
        for (int j = 0; j < M1; ++j) twB1[j] = wexp(j, N2);
        for (int b = 0; b < fast->NB; ++b)
            for (int j2 = 0; j2 < fast->NC; ++j2) twB2[(size_t)b * fast->NC + j2] = wexp((long long)j2 * b, M1);
        D4W_TRY(upload(pl, twC, &pl->fdev.twC));
        D4W_TRY(upload(pl, twB1, &pl->fdev.twB1));
        D4W_TRY(upload(pl, twB2, &pl->fdev.twB2));
    }

    // inverse maps frequency -> position
    std::vector<int> p_c1(C1), p_c2(C2), p_n1(N1), p_n2(N2);
    for (int p = 0; p < C1; ++p) p_c1[f_c1[p]] = p;
    for (int p = 0; p < C2; ++p) p_c2[f_c2[p]] = p;
    for (int p = 0; p < N1; ++p) p_n1[f_n1[p]] = p;
    for (int p = 0; p < N2; ++p) p_n2[f_n2[p]] = p;

    // four-step twiddles
    std::vector<float2> twc((size_t)C1 * C2), twt((size_t)N1 * N2);
    for (int q = 0; q < C1; ++q)
        for (int c2 = 0; c2 < C2; ++c2) twc[(size_t)q * C2 + c2] = wexp((long long)c2 * f_c1[q], nx);
    for (int q1 = 0; q1 < N1; ++q1)
        for (int b = 0; b < N2; ++b) twt[(size_t)q1 * N2 + b] = wexp((long long)b * f_n1[q1], M);
    D4W_TRY(upload(pl, twc, &pl->dev.twc));
    D4W_TRY(upload(pl, twt, &pl->dev.twt));

    // Hermitian partner maps
    std::vector<int> rowk(nx), rowpart(nx), q1part(N1), mirror0(N2);
    for (int q = 0; q < C1; ++q)
        for (int p2 = 0; p2 < C2; ++p2) rowk[q * C2 + p2] = f_c1[q] + C1 * f_c2[p2];
    for (int r = 0; r < nx; ++r) {
        const int km = (nx - rowk[r]) % nx;
        rowpart[r] = p_c1[km % C1] * C2 + p_c2[km / C1];
    }
    for (int q1 = 0; q1 < N1; ++q1) q1part[q1] = p_n1[(N1 - f_n1[q1]) % N1];
    for (int i = 0; i < N2; ++i) mirror0[i] = p_n2[(N2 - f_n2[i]) % N2];
    {   // pass-B work list: every Hermitian pair of sub-rows once
        std::vector<int2> pairs;
        pairs.reserve((size_t)nx * N1 / 2 + 4);
        for (int r = 0; r < nx; ++r)
            for (int q1 = 0; q1 < N1; ++q1) {
                const long keyA = (long)r * N1 + q1, keyB = (long)rowpart[r] * N1 + q1part[q1];
                if (keyB >= keyA) pairs.push_back(make_int2((int)keyA, (int)keyB));
            }
        pl->npairs = (int)pairs.size();
        D4W_TRY(upload(pl, pairs, &pl->dev.pairs));
        pl->h_pairs = pairs;
        pl->npairs_run = pl->npairs;
        pl->live_rows = nx;
        pl->fdev.pairs = pl->dev.pairs;
        pl->fdev.live = nullptr;
        {
            void* q = nullptr;
            if (hipMalloc(&q, (size_t)nx * sizeof(unsigned)) != hipSuccess) { d4w_fk_plan_destroy(pl); return fail(D4W_ENOMEM, "hipMalloc failed"); }
            pl->allocs.push_back(q); pl->d_rowmax = (unsigned*)q;
        }
        if (fast) {
            void* q = nullptr;
            if (hipMalloc(&q, (size_t)C1 * fast->C2A * sizeof(unsigned)) != hipSuccess) { d4w_fk_plan_destroy(pl); return fail(D4W_ENOMEM, "hipMalloc failed"); }
            pl->allocs.push_back(q); pl->d_livebits = (unsigned*)q;
            if (hipMalloc(&q, pairs.size() * sizeof(int2)) != hipSuccess) { d4w_fk_plan_destroy(pl); return fail(D4W_ENOMEM, "hipMalloc failed"); }
            pl->allocs.push_back(q); pl->d_pairs_live = (int2*)q;
        }
    }
    if (fast && fast->Bt_fwd) {
        // time-first order: work list of passes Bf / Bi.  BEFORE the c2 transform the Hermitian partner of row
        // (q, c2) is (q', c2), kc1(q') = -kc1(q) (fk_tf.h); the partner sub-row is the same q1' as in pass B.
        std::vector<int2> pairsT;
        pairsT.reserve((size_t)nx * N1 / 2 + 4);
        for (int r = 0; r < nx; ++r) {
            const int q = r / C2, c2 = r - q * C2;
            const int rb = p_c1[(C1 - f_c1[q]) % C1] * C2 + c2;
            for (int q1 = 0; q1 < N1; ++q1) {
                const long keyA = (long)r * N1 + q1, keyB = (long)rb * N1 + q1part[q1];
                if (keyB >= keyA) pairsT.push_back(make_int2((int)keyA, (int)keyB));
            }
        }
        // sorted by sub-row: a workgroup's consecutive pairs then share the tail gains of their sub-row (fkf_passBt PHASE 1)
        std::stable_sort(pairsT.begin(), pairsT.end(), [N1](const int2& a, const int2& b) { return a.x % N1 < b.x % N1; });
        pl->npairsT = (int)pairsT.size();
        D4W_TRY(upload(pl, pairsT, &pl->tfdev.pairs));
        void* q = nullptr;
        const size_t nctab = (size_t)fast->NC * fast->NB;
        if (hipMalloc(&q, 2 * (size_t)M * sizeof(unsigned)) != hipSuccess) { d4w_fk_plan_destroy(pl); return fail(D4W_ENOMEM, "hipMalloc failed"); }
        pl->allocs.push_back(q); pl->d_colkeys = (unsigned*)q;
        if (hipMalloc(&q, (size_t)M * sizeof(float)) != hipSuccess) { d4w_fk_plan_destroy(pl); return fail(D4W_ENOMEM, "hipMalloc failed"); }
        pl->allocs.push_back(q); pl->d_tgain = (float*)q;
        if (hipMalloc(&q, nctab * sizeof(int2)) != hipSuccess) { d4w_fk_plan_destroy(pl); return fail(D4W_ENOMEM, "hipMalloc failed"); }
        pl->allocs.push_back(q); pl->d_ctab = (int2*)q;
    }
    D4W_TRY(upload(pl, rowpart, &pl->dev.row_partner));
    D4W_TRY(upload(pl, q1part, &pl->dev.q1_partner));
    D4W_TRY(upload(pl, mirror0, &pl->dev.mirror0));
    const int *c_rowk, *c_k1, *c_k2;
    D4W_TRY(upload(pl, rowk, &c_rowk));
    D4W_TRY(upload(pl, f_n1, &c_k1));
    D4W_TRY(upload(pl, f_n2, &c_k2));
    {
        const int* c_q1k;
        D4W_TRY(upload(pl, p_n1, &c_q1k));
        pl->d_q1_of_k1 = const_cast<int*>(c_q1k);
        // tiling of the mask fold: runs of N1 * R0 samples in, IB positions out, transposed in <= 144 KiB of LDS
        const int R0 = pl->dev.ax_n2.nstage > 0 ? pl->dev.ax_n2.radix[0] : 1;
        const long RL = (long)N1 * R0;
        int IB = (int)std::min<long>(32, 16384 / RL - 1);          // <= 64 KiB of LDS: two 1024-thread workgroups per CU
        IB = std::min(IB, N2 / R0);
        if (IB >= 1) { pl->fold_R0 = R0; pl->fold_IB = IB; }
    }
    pl->d_rowk = const_cast<int*>(c_rowk);
    pl->d_k1 = const_cast<int*>(c_k1);
    pl->d_k2 = const_cast<int*>(c_k2);

    std::vector<float2> wrow(N1), wcol(N2);
    for (int q1 = 0; q1 < N1; ++q1) wrow[q1] = wexp(f_n1[q1], ns);
    for (int i = 0; i < N2; ++i) wcol[i] = wexp((long long)N1 * f_n2[i], ns);
    D4W_TRY(upload(pl, wrow, &pl->dev.wrow));
    D4W_TRY(upload(pl, wcol, &pl->dev.wcol));

    // tukey(ns, 0.03) both flat (taper_data) and packed (pass A)
    std::vector<float> win = tukey_window(ns, 0.03);
    std::vector<float2> winp(M);
    for (int m = 0; m < M; ++m) winp[m] = make_float2(win[2 * m], win[2 * m + 1]);
    D4W_TRY(upload(pl, winp, &pl->dev.win));

    void* p = nullptr;
    if (alloc_mask) {
        if (hipMalloc(&p, (size_t)nx * M * sizeof(float)) != hipSuccess) {
            d4w_fk_plan_destroy(pl);
            return fail(D4W_ENOMEM, "hipMalloc of the %zu-byte mask failed", (size_t)nx * M * sizeof(float));
        }
        pl->allocs.push_back(p);
        pl->d_mask = (float*)p;
        pl->dev.mask = pl->d_mask;
    }
    if (hipMalloc(&p, (size_t)nx * sizeof(float)) != hipSuccess) {
        d4w_fk_plan_destroy(pl);
        return fail(D4W_ENOMEM, "hipMalloc failed");
    }
    pl->allocs.push_back(p);
    pl->d_nyq = (float*)p;
    pl->dev.nyq = pl->d_nyq;
#undef D4W_TRY

    auto needs_generic = [](const AxisDesc& ax) {
        for (int s = 0; s < ax.nstage; ++s) {
            bool fast = false;
            for (int r : kFastRadix) fast |= (r == ax.radix[s]);
            if (!fast) return true;
        }
        return false;
    };
    pl->genericA = needs_generic(pl->dev.ax_c1) || needs_generic(pl->dev.ax_n1);
    pl->genericB = needs_generic(pl->dev.ax_n2);
    pl->genericC = needs_generic(pl->dev.ax_c2);
    pl->ldsA = ((size_t)C1 * N1 * TA + 2 * kTwLo + pl->dev.ax_c1.nhi + pl->dev.ax_n1.nhi) * sizeof(float2);
    pl->ldsC = ((size_t)C2 * TC + kTwLo + pl->dev.ax_c2.nhi) * sizeof(float2);
    if (bs_L) pl->ldsC = ((size_t)bs_L * TC + kTwLo + pl->dev.ax_bs.nhi) * sizeof(float2);
    pl->ldsB = ((size_t)2 * N2 + kTwLo + pl->dev.ax_n2.nhi) * sizeof(float2);
    if (bn_L) pl->ldsB = ((size_t)2 * bn_L + kTwLo + pl->dev.ax_bn.nhi) * sizeof(float2);
    auto env_int = [](const char* name, int dflt) {
        const char* v = getenv(name);
        return (v && atoi(v) > 0) ? atoi(v) : dflt;
    };
    pl->wg_per_cu = env_int("D4W_FK_WG_PER_CU", 2048 / kMaxThreads);     // tuning knob
    if (fast) {
        pl->wgA = env_int("D4W_FK_WG_A", fast->wgA);
        pl->wgC = env_int("D4W_FK_WG_C", fast->wgC);
        pl->wgB = env_int("D4W_FK_WG_B", fast->wgB);
        pl->wgBi = pl->wgBf = pl->wgB;
        pl->slab_sw = env_int("D4W_FK_SLAB", 0);
    }
    {
        int devid = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&devid) == hipSuccess && hipGetDeviceProperties(&prop, devid) == hipSuccess)
            pl->num_cu = prop.multiProcessorCount;
        if (fast) {
            (void)hipFuncSetAttribute((const void*)fast->A_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast->ldsA);
            (void)hipFuncSetAttribute((const void*)fast->A_fwd_taper, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast->ldsA);
            (void)hipFuncSetAttribute((const void*)fast->A_inv, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast->ldsA);
            (void)hipFuncSetAttribute((const void*)fast->A_inv_stats, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast->ldsA);
            (void)hipFuncSetAttribute((const void*)fast->C_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast->ldsC);
            (void)hipFuncSetAttribute((const void*)fast->C_inv, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast->ldsC);
            (void)hipFuncSetAttribute((const void*)fast->B_mid, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast->ldsB);
            const void* fa[] = {(const void*)fast->T_fwd, (const void*)fast->T_fwd_taper, (const void*)fast->T_inv, (const void*)fast->T_inv_stats,
                                (const void*)fast->Ac_fwd, (const void*)fast->Ac_inv, (const void*)fast->T_inv_env};
            for (const void* f : fa) (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast->ldsA);
            (void)hipFuncSetAttribute((const void*)fast->Cs_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast->ldsC);
            (void)hipFuncSetAttribute((const void*)fast->Cs_inv, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast->ldsC);
            (void)hipFuncSetAttribute((const void*)fast->Bs_mid, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast->ldsB);
            (void)hipFuncSetAttribute((const void*)fast->Bs_hilb, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast->ldsB);
            if (fast->Bt_fwd) {
                (void)hipFuncSetAttribute((const void*)fast->Bt_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast->ldsBt);
                (void)hipFuncSetAttribute((const void*)fast->Bt_inv, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast->ldsBt);
                if (fast->C_mid) (void)hipFuncSetAttribute((const void*)fast->C_mid, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast->ldsC);
                // (below) resident workgroups of the pass-B forms from what their registers and LDS allow
            }
            // Pass B in its three forms is bound by VALU issue AND by what its few waves can overlap: a CU takes as many
            // workgroups of each form as that form's registers (512 per SIMD lane, granules of 8) and LDS (160 KiB) allow,
            // at most 3 (4 measured slower) -- at 20 000 x 120 000: fused B 161 VGPRs and Bi 150 -> three 4-wave workgroups
            // (Bi 3.54 -> 3.2 ms, the part's copy rate), Bf 210 -> two.  The table's wgB is the floor.
            auto resident = [&](const void* fn, size_t lds) {
                hipFuncAttributes fa;
                if (!fn || hipFuncGetAttributes(&fa, fn) != hipSuccess || fa.numRegs <= 0) return pl->wgB;
                const int waves_simd = 512 / (((int)fa.numRegs + 7) / 8 * 8);
                const int by_regs = waves_simd * 4 / std::max(1, (fast->thrB + 63) / 64);
                const int by_lds = (int)((160 * 1024) / std::max<size_t>(lds, 1));
                return std::max(pl->wgB, std::min(3, std::min(by_regs, by_lds)));
            };
            pl->wgBi = env_int("D4W_FK_WG_BI", resident((const void*)fast->Bt_inv, fast->ldsBt));
            pl->wgBf = env_int("D4W_FK_WG_BF", resident((const void*)fast->Bt_fwd, fast->ldsBt));
            if (!getenv("D4W_FK_WG_B")) pl->wgB = resident((const void*)fast->B_mid, fast->ldsB);

        }
        const size_t lds_max = std::max(pl->ldsA, std::max(pl->ldsB, pl->ldsC));
        if (!fast && lds_max > 64 * 1024) {
            // tiles are capped at 64 KiB; the twiddle tables push the request slightly above the
            // default dynamic-LDS limit
            fk_pass_ac_lds_limit(80 * 1024);
            const void* fns[] = {
                (const void*)fk_passC_bluestein<false>, (const void*)fk_passC_bluestein<true>,
                (const void*)fk_passB<true>, (const void*)fk_passB<false>, (const void*)fk_passB_bluestein};
            for (const void* f : fns)
                (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
        }
        if (bs_L) {
            (void)hipFuncSetAttribute((const void*)fk_passC_bluestein<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
            (void)hipFuncSetAttribute((const void*)fk_passC_bluestein<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
            (void)hipFuncSetAttribute((const void*)fk_passCm_bluestein, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
        }
    }
    *out = pl;
    return D4W_OK;
}

extern "C" {

int d4w_fk_plan_create_ex(int nx, int ns, const int* opts, d4w_fk_plan** out) {
    return fk_plan_build(nx, ns, opts, true, false, out);
}

int d4w_fk_plan_create(int nx, int ns, d4w_fk_plan** out) { return d4w_fk_plan_create_ex(nx, ns, nullptr, out); }

int d4w_fk_plan_info(const d4w_fk_plan* pl, int* info) {
    if (!pl || !info) return fail(D4W_EINVAL, "NULL argument");
    const FkDims& d = pl->dev.d;
    const int v[8] = {d.nx, d.ns, d.C1, d.C2, d.N1, d.N2, d.TA, d.TC};
    memcpy(info, v, sizeof(v));
    return D4W_OK;
}

}  // extern "C"

// Gains the filter treats as zero.  Opt-in: prune_eps * max|M_h| (approximate, FkPlan.set_mask(m, prune_eps=...)).
// Always: D4W_FK_ROUND_EPS (default 2^-24) / sqrt(nx ns) * max|M_h| -- what such gains add to ANY output sample is at
// most  g ||x||_F  =  2^-24 max|M_h| rms(x)  (Cauchy-Schwarz over the spectrum): half a float32 ulp of the input's RMS,
// below the rounding noise of the float32 transforms themselves, whatever the input.
double d4w::fk_zero_gain(const FkDims& d, double prune_eps, double gmax) {
    static const double round_eps = [] {
        const char* v = getenv("D4W_FK_ROUND_EPS");
        return v ? atof(v) : 5.9604644775390625e-8;
    }();
    return std::max(prune_eps, round_eps / sqrt((double)d.nx * (double)d.ns)) * gmax;
}

static inline float fk_key_value(unsigned k) {
    const unsigned b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    float v;
    memcpy(&v, &b, sizeof(v));
    return v;
}

// the time-first workspace (12 B x nx x Lc, up to 1.3x the data block) goes back to the allocator
static void fk_tf_release(d4w_fk_plan* pl) {
    if (pl->d_W) (void)hipFree(pl->d_W);
    if (pl->d_cmask) (void)hipFree(pl->d_cmask);
    if (pl->d_colsrc) (void)hipFree(pl->d_colsrc);
    if (pl->d_cmlive) (void)hipFree(pl->d_cmlive);
    pl->d_W = nullptr; pl->d_cmask = nullptr; pl->d_colsrc = nullptr; pl->d_cmlive = nullptr; pl->cap_W = 0;
}

// Time-first order for the mask just folded (fk_tf.h): classify the half-spectrum columns, lay the kept ones out,
// model the bytes of both orders; when time-first wins, build the pass tables, the compact band mask and the workspace.
static int fk_tf_setup(d4w_fk_plan* pl, double zero_gain, void* stream) {
    const FkDims& d = pl->dev.d;
    const FkFastEntry& F = *pl->fast;
    hipStream_t st = (hipStream_t)stream;
    const int NA = F.NA, NB = F.NB, NC = F.NC, N1 = d.N1, N2 = d.N2, M = d.M, TC = d.TC;
    pl->tf = false;
    pl->bytes_cf = 24.0 + 18.0 * (double)pl->live_rows / d.nx;
    pl->bytes_tf = 42.0;
    const char* ord = getenv("D4W_FK_ORDER");
    if (ord && !strcmp(ord, "cf")) return D4W_OK;
    D4W_HIP(hipMemsetAsync(pl->d_colkeys, 0xFF, (size_t)M * sizeof(unsigned), st));
    D4W_HIP(hipMemsetAsync(pl->d_colkeys + M, 0, (size_t)M * sizeof(unsigned), st));
    const int rpb = 512;
    D4W_LAUNCH(fk_col_minmax, dim3(ceil_div(M, kThreads), ceil_div(d.nx, rpb)), dim3(kThreads), 0, stream, d,
               (const float*)pl->d_mask, rpb, pl->d_colkeys, pl->d_colkeys + M);
    std::vector<unsigned> keys(2 * (size_t)M);
    std::vector<float> nyq(d.nx);
    D4W_HIP(hipMemcpyAsync(keys.data(), pl->d_colkeys, keys.size() * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    D4W_HIP(hipMemcpyAsync(nyq.data(), pl->d_nyq, (size_t)d.nx * sizeof(float), hipMemcpyDeviceToHost, st));
    D4W_HIP(hipStreamSynchronize(st));
    // column classes at the positions p = q1 N2 + e: 0 dead, 1 band, 2 tail (gain the same for every wavenumber)
    std::vector<unsigned char> ccls(M);
    std::vector<float> cgain(M);
    for (int p = 0; p < M; ++p) {
        const float lo = fk_key_value(keys[p]), hi = fk_key_value(keys[M + p]);
        const double amax = std::max(fabs((double)lo), fabs((double)hi));
        cgain[p] = 0.5f * (lo + hi);
        if (!(lo == lo) || !(hi == hi) || std::isinf(lo) || std::isinf(hi)) ccls[p] = 1;        // NaN / inf gains: as NumPy, through the product
        else if (amax <= zero_gain) ccls[p] = 0;
        else if ((double)hi - (double)lo <= zero_gain) ccls[p] = 2;
        else ccls[p] = 1;
    }
    bool nyq_live = false;
    for (int r = 0; r < d.nx; ++r) nyq_live |= !(fabs((double)nyq[r]) <= zero_gain);
    // cells (d2, d1): the strongest class of their N1 NA columns; position e = d0 NB NC + d1 NC + d2
    std::vector<int> cell(NC * NB, 0);
    for (int q1 = 0; q1 < N1; ++q1)
        for (int e = 0; e < N2; ++e) {
            const int c = ccls[(size_t)q1 * N2 + e];
            if (!c) continue;
            const int d1 = (e / NC) % NB, d2 = e % NC;
            int& cc = cell[d2 * NB + d1];
            if (c == 1) cc = 1;
            else if (cc == 0) cc = 2;
        }
    // layout of a row of W: N1 sub-row blocks of RW columns, [band cells (bw, a multiple of TC) | tail cells] each, then one
    // strip for the Nyquist column
    std::vector<int2> ctab(NC * NB);
    int rw[3] = {0, 0, 0}, ncell[3] = {0, 0, 0};
    for (int c : cell) ncell[c]++;
    const int bw = ceil_div(NA * ncell[1], TC) * TC;
    for (int d2 = 0; d2 < NC; ++d2) {
        int cnt[3] = {0, 0, 0};
        for (int d1 = 0; d1 < NB; ++d1) cnt[cell[d2 * NB + d1]]++;
        int rank[3] = {0, 0, 0};
        for (int d1 = 0; d1 < NB; ++d1) {
            const int c = cell[d2 * NB + d1];
            ctab[d2 * NB + d1] = c ? make_int2((c == 2 ? bw : 0) + rw[c] + rank[c], cnt[c] | (c << 28)) : make_int2(0, 0);
            rank[c]++;
        }
        rw[1] += NA * cnt[1];
        rw[2] += NA * cnt[2];
    }
    const int RW = std::max(TC, ceil_div(bw + rw[2], TC) * TC);
    const int Lc = ceil_div(N1 * RW + (nyq_live ? TC : 0), 16) * 16;
    pl->tf_band_cols = N1 * rw[1] + (nyq_live ? 1 : 0);
    pl->tf_tail_cols = N1 * rw[2];
    pl->bytes_tf = 24.0 + 18.0 * (double)(N1 * bw + (nyq_live ? TC : 0)) / M + 8.0 * (double)(N1 * rw[2]) / M;
    const bool force = ord && !strcmp(ord, "tf");
    // channel-first stays (it needs no workspace): what an earlier mask of this plan allocated for the other order is freed
    if ((!force && !(pl->bytes_tf < 0.97 * pl->bytes_cf)) || (size_t)Lc * sizeof(float2) >= ((size_t)1 << 31)) {   // 32-bit column offsets inside a row
        fk_tf_release(pl);
        return D4W_OK;
    }
    // tables
    std::vector<float> tgain(M, 0.f);
    std::vector<int> colsrc((size_t)Lc, -1);
    for (int q1 = 0; q1 < N1; ++q1)
        for (int e = 0; e < N2; ++e) {
            const int d0 = e / (NB * NC), d1 = (e / NC) % NB, d2 = e % NC;
            const int c = cell[d2 * NB + d1];
            const size_t p = (size_t)q1 * N2 + e;
            if (c == 1) {
                tgain[p] = 1.f;
                const int2 ct = ctab[d2 * NB + d1];
                colsrc[(size_t)q1 * RW + ct.x + d0 * (ct.y & 0x0FFFFFFF)] = (int)p;
            } else if (c == 2)
                tgain[p] = cgain[p] * (float)d.C2;      // the band columns pick up C2 from the unnormalised c2 forward + inverse of Cm
        }
    if (nyq_live) colsrc[(size_t)N1 * RW] = -2;
    const size_t need = (size_t)d.nx * Lc;
    if (need > pl->cap_W) {
        fk_tf_release(pl);
        // Not enough memory for the workspace is not an error: the channel-first order works in place in the output block
        // and gives the same result (more bytes moved).  Everything allocated so far goes back; pl->tf stays false.
        const bool ok = hipMalloc((void**)&pl->d_W, need * sizeof(float2)) == hipSuccess &&
                        hipMalloc((void**)&pl->d_cmask, need * sizeof(float)) == hipSuccess &&
                        hipMalloc((void**)&pl->d_colsrc, ((size_t)M + 64 * (size_t)N1 + 64) * sizeof(int)) == hipSuccess &&
                        // Cm tiles: at most C1 (N1 (N2 / TC + 2) + 1) whatever the mask
                        hipMalloc((void**)&pl->d_cmlive, (size_t)d.C1 * ((size_t)N1 * (N2 / TC + 2) + 1) * F.C2A * sizeof(unsigned)) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            fk_tf_release(pl);
            static bool told = false;
            if (!told && getenv("D4W_VERBOSE")) fprintf(stderr, "das4whales_amd: %zu bytes for the time-first f-k workspace not available, channel-first order kept\n", need * 12);
            told = true;
            return D4W_OK;
        }
        pl->cap_W = need;
    }
    D4W_HIP(hipMemcpyAsync(pl->d_tgain, tgain.data(), (size_t)M * sizeof(float), hipMemcpyHostToDevice, st));
    D4W_HIP(hipMemcpyAsync(pl->d_ctab, ctab.data(), ctab.size() * sizeof(int2), hipMemcpyHostToDevice, st));
    D4W_HIP(hipMemcpyAsync(pl->d_colsrc, colsrc.data(), (size_t)Lc * sizeof(int), hipMemcpyHostToDevice, st));
    D4W_HIP(hipMemsetAsync(pl->d_W, 0, need * sizeof(float2), st));        // padding columns stay finite
    if (d.nx > 65535) return fail(D4W_EINVAL, "nx = %d exceeds the grid limit 65535", d.nx);
    D4W_LAUNCH(fk_gather_cmask, dim3(std::min(ceil_div(Lc, kThreads), 64), d.nx), dim3(kThreads), 0, stream, d,
               (const float*)pl->d_mask, (const float*)pl->d_nyq, (const int*)pl->d_colsrc, Lc, pl->d_cmask);
    {
        const int nb1 = bw / TC, ntCm = (N1 * nb1 + (nyq_live ? 1 : 0)) * d.C1;
        if (ntCm > 0 && !pl->dev.bs_L)
            D4W_LAUNCH(fk_cm_livebits, dim3(ceil_div(ntCm * F.C2A, kThreads)), dim3(kThreads), 0, stream, (const float*)pl->d_cmask, Lc,
                       d.C2, F.C2A, F.C2B, TC, N1, nb1, RW, nyq_live ? N1 * RW : -1, ntCm, pl->d_cmlive);
    }
    D4W_HIP(hipStreamSynchronize(st));          // the host tables above are temporaries
    FkTfDev& T = pl->tfdev;
    T.tgain = pl->d_tgain; T.ctab = pl->d_ctab; T.cmask = pl->d_cmask; T.W = pl->d_W; T.cmlive = pl->d_cmlive;
    T.RW = RW; T.bw = bw;
    T.col_nyq = nyq_live ? N1 * RW : -1;
    T.Lc = Lc;
    pl->tf = true;
    return D4W_OK;
}

// after a fold (d_mask, d_nyq, d_rowmax written on `stream`): liveness of the wavenumber rows, order of the passes
static int fk_mask_finish(d4w_fk_plan* pl, double prune_eps, void* stream) {
    const FkDims& d = pl->dev.d;
    hipStream_t st = (hipStream_t)stream;
    pl->has_mask = true;
    pl->prune_eps = prune_eps;
    pl->npairs_run = pl->npairs;
    pl->live_rows = d.nx;
    pl->fdev.pairs = pl->dev.pairs;
    pl->fdev.live = nullptr;
    pl->tf = false;
    const char* np = getenv("D4W_FK_NOPRUNE");
    if (pl->fast && !(np && atoi(np) > 0)) {
        // Dead rows (not with a Bluestein pass C, which has no row skipping: only the pass order is chosen there): a wavenumber row whose folded gains (and whose Hermitian partner's) are all zero -- or below the
        // zero-gain threshold above: rounding level always, prune_eps * max |M_h| opt-in (the Butterworth tails of
        // hybrid_ninf_filter_design, dsp.py:348-349, never reach zero: 7.7e-7 at fmax + 14 Hz; treating them as zero
        // changes the output by at most that gain times the spectral content the input holds there)
        std::vector<unsigned> rmax(d.nx);
        D4W_HIP(hipMemcpyAsync(rmax.data(), pl->d_rowmax, (size_t)d.nx * sizeof(unsigned), hipMemcpyDeviceToHost, st));
        D4W_HIP(hipStreamSynchronize(st));
        float gmax = 0.f;
        std::vector<float> rm(d.nx);
        for (int r = 0; r < d.nx; ++r) {
            memcpy(&rm[r], &rmax[r], sizeof(float));
            if (rm[r] == rm[r] && !std::isinf(rm[r]) && rm[r] > gmax) gmax = rm[r];
        }
        const double zero_gain = fk_zero_gain(d, prune_eps, gmax);
        const float thr = (float)zero_gain;
        std::vector<int> live(d.nx);
        for (int r = 0; r < d.nx; ++r) live[r] = !(rm[r] <= thr);             // NaN rows stay alive
        const int N1 = d.N1;
        std::vector<char> lv(d.nx, 0);
        std::vector<int2> run;
        run.reserve(pl->h_pairs.size());
        for (const int2& pr : pl->h_pairs) {
            const int ra = pr.x / N1, rb = pr.y / N1;
            if (live[ra] || live[rb]) {
                lv[ra] = lv[rb] = 1;
                run.push_back(pr);
            }
        }
        int nlive = 0;
        for (int r = 0; r < d.nx; ++r) nlive += lv[r];
        if (nlive < d.nx && !pl->dev.bs_L) {
            const int RA = pl->fast->C2A, RB = pl->fast->C2B;
            std::vector<unsigned> bits((size_t)d.C1 * RA, 0u);
            for (int r = 0; r < d.nx; ++r)
                if (lv[r]) {
                    const int q = r / d.C2, p2 = r % d.C2;
                    bits[(size_t)q * RA + p2 / RB] |= 1u << (p2 % RB);
                }
            D4W_HIP(hipMemcpyAsync(pl->d_livebits, bits.data(), bits.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
            if (!run.empty())
                D4W_HIP(hipMemcpyAsync(pl->d_pairs_live, run.data(), run.size() * sizeof(int2), hipMemcpyHostToDevice, st));
            D4W_HIP(hipStreamSynchronize(st));      // bits / run are host temporaries
            pl->fdev.live = pl->d_livebits;
            pl->fdev.pairs = pl->d_pairs_live;
            pl->npairs_run = (int)run.size();
            pl->live_rows = nlive;
        }
        if (pl->fast->Bt_fwd && pl->d_colkeys) {
            int rc = fk_tf_setup(pl, zero_gain, stream);
            if (rc != D4W_OK) return rc;
        }
    }
    return D4W_OK;
}

// device-side order of the operations on one plan (see d4w_fk_plan::apply_mu); the caller holds pl->apply_mu
static int fk_plan_enter(d4w_fk_plan* pl, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (pl->apply_used && pl->apply_stream != st) D4W_HIP(hipStreamWaitEvent(st, pl->apply_done, 0));
    return D4W_OK;
}
static int fk_plan_leave(d4w_fk_plan* pl, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!pl->apply_done) D4W_HIP(hipEventCreateWithFlags(&pl->apply_done, hipEventDisableTiming));
    D4W_HIP(hipEventRecord(pl->apply_done, st));
    pl->apply_stream = st;
    pl->apply_used = true;
    return D4W_OK;
}

static int fk_set_mask_run(d4w_fk_plan* pl, const float* mask_shifted, double prune_eps, void* stream, FkAffine aff) {
    if (!(prune_eps >= 0.0 && prune_eps < 1.0)) return fail(D4W_EINVAL, "prune_eps = %g not in [0, 1)", prune_eps);
    if (pl && pl->big) {                            // (no dead-row pruning on this path: prune_eps acts on the Bluestein channel phase's columns)
        fkd_set_prune(pl->big, prune_eps);
        int rc = fkd_set_mask_dense_affine(pl->big, mask_shifted, aff.a, aff.b, aff.on, stream);
        if (rc == D4W_OK) pl->has_mask = true;
        return rc;
    }
    if (!pl || !mask_shifted || !pl->d_mask) return fail(D4W_EINVAL, "NULL argument");
    const FkDims& d = pl->dev.d;
    hipStream_t st = (hipStream_t)stream;
    D4W_HIP(hipMemsetAsync(pl->d_rowmax, 0, (size_t)d.nx * sizeof(unsigned), st));
    const char* gather = getenv("D4W_FK_FOLD_GATHER");
    if (pl->fold_IB > 0 && !(gather && atoi(gather) > 0)) {
        const int N2r = d.N2 / pl->fold_R0;
        const size_t lds = (size_t)d.N1 * pl->fold_R0 * (pl->fold_IB + 1) * sizeof(float);
        static std::once_flag once;
        std::call_once(once, [] { (void)hipFuncSetAttribute((const void*)fk_fold_mask_tiled, hipFuncAttributeMaxDynamicSharedMemorySize, 148 * 1024); });
        if (d.nx > 65535) return fail(D4W_EINVAL, "nx = %d exceeds the grid limit 65535", d.nx);
        D4W_LAUNCH(fk_fold_mask_tiled, dim3(ceil_div(N2r, pl->fold_IB), d.nx), dim3(kFoldThreads), lds, stream, d, pl->fold_R0,
                   pl->fold_IB, mask_shifted, (const int*)pl->d_rowk, (const int*)pl->d_q1_of_k1, (const int*)pl->d_k2,
                   pl->d_mask, pl->d_nyq, pl->d_rowmax, aff);
    } else {
        dim3 grid(std::min(ceil_div(d.M, kThreads), 64), d.nx);
        D4W_LAUNCH(fk_fold_mask, grid, dim3(kThreads), 0, stream, d, mask_shifted, (const int*)pl->d_rowk,
                   (const int*)pl->d_k1, (const int*)pl->d_k2, pl->d_mask, pl->d_nyq, pl->d_rowmax, aff);
    }
    return fk_mask_finish(pl, prune_eps, stream);
}

static int fk_set_mask_impl(d4w_fk_plan* pl, const float* mask_shifted, double prune_eps, void* stream, FkAffine aff = FkAffine{1.f, 0.f, 0}) {
    if (!pl) return fail(D4W_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(pl->apply_mu);
    int rc = fk_plan_enter(pl, stream);
    if (rc != D4W_OK) return rc;
    rc = fk_set_mask_run(pl, mask_shifted, prune_eps, stream, aff);
    const int rl = fk_plan_leave(pl, stream);
    return rc != D4W_OK ? rc : rl;
}

static int fk_set_mask_design_run(d4w_fk_plan* pl, int mode, double k_spacing, double t_spacing, const double* params8_host,
                                  int i0, int i1, const double* hrow_dev, double prune_eps, void* stream) {
    if (pl && pl->big) {
        if (!(prune_eps >= 0.0 && prune_eps < 1.0)) return fail(D4W_EINVAL, "prune_eps = %g not in [0, 1)", prune_eps);
        fkd_set_prune(pl->big, prune_eps);
        int rc = d4w_fkd_set_mask_design_f32(pl->big, mode, k_spacing, t_spacing, params8_host, i0, i1, hrow_dev, stream);
        if (rc == D4W_OK) pl->has_mask = true;
        return rc;
    }
    if (!pl || !params8_host || !pl->d_mask) return fail(D4W_EINVAL, "NULL argument");
    if (mode < 0 || mode > 2)
        return fail(D4W_EINVAL, "mode %d has no closed form (the Gaussian-blurred designs go through d4w_design_mask_f32)", mode);
    if (mode == 2 && !hrow_dev) return fail(D4W_EINVAL, "hybrid_ninf needs the |H|^2 row");
    if (!(prune_eps >= 0.0 && prune_eps < 1.0)) return fail(D4W_EINVAL, "prune_eps = %g not in [0, 1)", prune_eps);
    const FkDims& d = pl->dev.d;
    if (d.nx > 65535) return fail(D4W_EINVAL, "nx = %d exceeds the grid limit 65535", d.nx);
    D4W_HIP(hipMemsetAsync(pl->d_rowmax, 0, (size_t)d.nx * sizeof(unsigned), (hipStream_t)stream));
    const DesignArgs A = make_design_args(d.nx, d.ns, k_spacing, t_spacing, params8_host, i0, i1, hrow_dev);
    dim3 grid(std::min(ceil_div(d.M, kThreads), 64), d.nx);
    D4W_LAUNCH(fk_fold_design, grid, dim3(kThreads), 0, stream, d, A, mode, (const int*)pl->d_rowk, (const int*)pl->d_k1,
               (const int*)pl->d_k2, pl->d_mask, pl->d_nyq, pl->d_rowmax);
    return fk_mask_finish(pl, prune_eps, stream);
}

// Where the row statistics of a filtered block come from.  The last pass's epilogue pays where a pass-A tile is large: at
// 20 000 x 120 000 (C1 N1 = 625 points per strip column) it adds 0.2 ms to a 3.7-ms pass against 1.7 ms for a separate sweep
// of y.  At the 60-s file shapes (C1 N1 = 100) the same epilogue turned a 215-us pass into 390 us (500 us with shorter runs:
// the per-run reduction is what costs, profiles/r05d/stream_kernels.txt) against 137 us for d4w_row_stats_f32: small tiles
// on large blocks take the sweep.  Plans without the specialised kernels always sweep.
static bool fk_stats_in_epilogue(const d4w_fk_plan* pl) {
    if (!pl->fast) return false;
    const FkDims& d = pl->dev.d;
    static const int epi_env = [] { const char* v = getenv("D4W_FK_STATS_EPILOGUE"); return v ? atoi(v) : -1; }();
    return epi_env >= 0 ? epi_env > 0 : (d.C1 * d.N1 >= 256 || (long long)d.nx * d.ns < (1ll << 22));
}

static int fk_apply_run(d4w_fk_plan* pl, const float* x, float* y, int taper, void* stream, hipEvent_t* ev, double* row_mean,
                        float* row_maxabs) {
    if (!pl || !x || !y) return fail(D4W_EINVAL, "NULL argument");
    if ((row_mean == nullptr) != (row_maxabs == nullptr)) return fail(D4W_EINVAL, "row_mean and row_maxabs go together");
    if (!pl->has_mask) return fail(D4W_EINVAL, "no mask set on this plan");
    if (pl->big) {
        // time phase of all rows into y (as the packed half spectrum), channel phase on it in place, time phase back
        hipStream_t sb = (hipStream_t)stream;
        int rc;
        if (ev) D4W_HIP(hipEventRecord(ev[0], sb));
        if ((rc = d4w_fkd_time_fwd_f32(pl->big, x, y, taper, stream))) return rc;
        if (ev) { D4W_HIP(hipEventRecord(ev[1], sb)); D4W_HIP(hipEventRecord(ev[2], sb)); }
        if ((rc = d4w_fkd_chan_apply_f32(pl->big, y, stream))) return rc;
        if (ev) { D4W_HIP(hipEventRecord(ev[3], sb)); D4W_HIP(hipEventRecord(ev[4], sb)); }
        if ((rc = d4w_fkd_time_inv_f32(pl->big, y, stream))) return rc;
        if (row_mean && (rc = d4w_row_stats_f32(y, pl->dev.d.nx, pl->dev.d.ns, row_mean, row_maxabs, stream))) return rc;
        if (ev) D4W_HIP(hipEventRecord(ev[5], sb));
        return D4W_OK;
    }
    const FkDev& P = pl->dev;
    const FkDims& d = P.d;
    const float2* src = reinterpret_cast<const float2*>(x);
    float2* dst = reinterpret_cast<float2*>(y);
    const dim3 blk(pl->threads);
    const int ntA = ceil_div(d.N2, d.TA) * d.C2;
    const int ntC = ceil_div(d.M, d.TC) * d.C1;
    const int ntB = pl->npairs;
    const int persist = pl->num_cu * pl->wg_per_cu;
    const dim3 gridA(std::min(ntA, persist)), gridC(std::min(ntC, persist)), gridB(std::min(ntB, persist));
    hipStream_t st = (hipStream_t)stream;
    if (pl->fast && row_mean && !fk_stats_in_epilogue(pl)) {
        int rc = fk_apply_run(pl, x, y, taper, stream, ev, nullptr, nullptr);
        if (rc) return rc;
        return d4w_row_stats_f32(y, d.nx, d.ns, row_mean, row_maxabs, stream);
    }
    if (pl->fast) {
        const FkFastEntry& F = *pl->fast;
        const int NBX = d.N2 / d.TA, NBC = d.N2 / d.TC;
        const int fA = NBX * d.C2, fC = (d.M / d.TC) * d.C1;
        const dim3 gA(std::min(fA, pl->num_cu * pl->wgA)), gC(std::min(fC, pl->num_cu * pl->wgC)),
            gB(std::max(1, std::min(pl->npairs_run, pl->num_cu * pl->wgB)));
        int rc;
#define D4W_MARK(i) do { if (ev) D4W_HIP(hipEventRecord(ev[i], st)); } while (0)
        // row statistics in the epilogue of the last pass: tiles walked in runs of `run` (a divisor of the tiles
        // per c2 of the pass / slab, so that a run stays on the same C1 rows)
        auto stats_run = [](int per_c2, long long) {
            static const int run_env = [] { const char* v = getenv("D4W_FK_RUN_A"); return v ? atoi(v) : 30; }();
            int run = 1;
            for (int r = 1; r <= per_c2 && r <= std::max(run_env, 1); ++r) if (per_c2 % r == 0) run = r;
            return run;
        };
        if (row_mean) {
            D4W_HIP(hipMemsetAsync(row_mean, 0, (size_t)d.nx * sizeof(double), st));
            D4W_HIP(hipMemsetAsync(row_maxabs, 0, (size_t)d.nx * sizeof(float), st));
        }
        const int sw = pl->slab_sw;
        if (sw > 0 && d.TA == d.TC && NBX % sw == 0 && sw < NBX) {
            // Slab order: passes A and C run back to back on one slab of sw column blocks of every n1
            // sub-row (all channels x N1 sw TA columns), slab after slab, so that what pass A wrote is still in the
            // 256 MiB Infinity Cache when pass C reads it -- and the same for C' -> A'.  Same kernels, same tiles,
            // same arithmetic as the plain order; only the order of the tiles differs.
            const int nslab = NBX / sw, nA = d.C2 * sw, nC = d.C1 * d.N1 * sw;
            const dim3 gsA(std::min(nA, pl->num_cu * pl->wgA)), gsC(std::min(nC, pl->num_cu * pl->wgC));
            D4W_MARK(0);
            for (int sl = 0; sl < nslab; ++sl) {
                if ((rc = launch_k(taper ? F.A_fwd_taper : F.A_fwd, gsA, dim3(F.thrA), F.ldsA, stream, P, src, dst, 0, nA, sw, sl * sw, FkGeo()))) return rc;
                if ((rc = launch_k(F.C_fwd, gsC, dim3(F.thrC), F.ldsC, stream, P, pl->fdev, dst, 0, nC, sw, sl * sw, FkGeo()))) return rc;
            }
            D4W_MARK(1);
            D4W_MARK(2);
            if ((rc = launch_k(F.B_mid, gB, dim3(F.thrB), F.ldsB, stream, P, pl->fdev, dst, 0, pl->npairs_run, FkGeo()))) return rc;
            D4W_MARK(3);
            const int run = stats_run(sw, nA), nruns = nA / run;
            for (int sl = 0; sl < nslab; ++sl) {
                if ((rc = launch_k(F.C_inv, gsC, dim3(F.thrC), F.ldsC, stream, P, pl->fdev, dst, 0, nC, sw, sl * sw, FkGeo()))) return rc;
                if (row_mean) {
                    if ((rc = launch_k(F.A_inv_stats, dim3(std::min(nruns, pl->num_cu * pl->wgA)), dim3(F.thrA), F.ldsA, stream, P,
                                       dst, run, nruns, row_mean, (unsigned*)row_maxabs, sw, sl * sw, FkGeo(), (const float2*)nullptr, 0))) return rc;
                } else if ((rc = launch_k(F.A_inv, gsA, dim3(F.thrA), F.ldsA, stream, P, dst, 0, nA, sw, sl * sw, FkGeo(), (const float2*)nullptr))) return rc;
            }
            D4W_MARK(4);
            D4W_MARK(5);
            return D4W_OK;
        }
        if (pl->tf) {
            // time-first order (fk_tf.h): A, Bf (-> W), Cm (on W), Bi (W ->), A'
            const FkTfDev& T = pl->tfdev;
            const int ntCm = (d.N1 * (T.bw / d.TC) + (T.col_nyq >= 0 ? 1 : 0)) * d.C1;
            const dim3 gCm(std::max(1, std::min(ntCm, pl->num_cu * pl->wgC)));
            D4W_MARK(0);
            if ((rc = launch_k(taper ? F.A_fwd_taper : F.A_fwd, gA, dim3(F.thrA), F.ldsA, stream, P, src, dst, 0, fA, NBX, 0, FkGeo()))) return rc;
            D4W_MARK(1);
            const dim3 gBf(std::max(1, std::min(pl->npairsT, pl->num_cu * pl->wgBf)));
            if ((rc = launch_k(F.Bt_fwd, gBf, dim3(F.thrB), F.ldsBt, stream, P, pl->fdev, T, dst, 0, pl->npairsT))) return rc;
            D4W_MARK(2);
            if (ntCm > 0) {
                if (P.bs_L) rc = launch_k(fk_passCm_bluestein, dim3(std::max(1, std::min(ntCm, persist))), blk, pl->ldsC, stream, P, T, ntCm);
                else rc = launch_k(F.C_mid, gCm, dim3(F.thrC), F.ldsC, stream, P, pl->fdev, T, 0, ntCm);
                if (rc) return rc;
            }
            D4W_MARK(3);
            const dim3 gBi(std::max(1, std::min(pl->npairsT, pl->num_cu * pl->wgBi)));
            if ((rc = launch_k(F.Bt_inv, gBi, dim3(F.thrB), F.ldsBt, stream, P, pl->fdev, T, dst, 0, pl->npairsT))) return rc;
            D4W_MARK(4);
            if (row_mean) {
                const int run = stats_run(NBX, fA), nruns = fA / run;
                if ((rc = launch_k(F.A_inv_stats, dim3(std::min(nruns, pl->num_cu * pl->wgA)), dim3(F.thrA), F.ldsA, stream, P,
                                   dst, run, nruns, row_mean, (unsigned*)row_maxabs, NBX, 0, FkGeo(), (const float2*)nullptr, 0))) return rc;
            } else if ((rc = launch_k(F.A_inv, gA, dim3(F.thrA), F.ldsA, stream, P, dst, 0, fA, NBX, 0, FkGeo(), (const float2*)nullptr))) return rc;
            D4W_MARK(5);
            return D4W_OK;
        }
        D4W_MARK(0);
        if ((rc = launch_k(taper ? F.A_fwd_taper : F.A_fwd, gA, dim3(F.thrA), F.ldsA, stream, P, src, dst, 0, fA, NBX, 0, FkGeo()))) return rc;
        D4W_MARK(1);
        if (P.bs_L) rc = launch_k(fk_passC_bluestein<false>, gridC, blk, pl->ldsC, stream, P, dst, ntC);      // C2X > 1
        else rc = launch_k(F.C_fwd, gC, dim3(F.thrC), F.ldsC, stream, P, pl->fdev, dst, 0, fC, NBC, 0, FkGeo());
        if (rc) return rc;
        D4W_MARK(2);
        if ((rc = launch_k(F.B_mid, gB, dim3(F.thrB), F.ldsB, stream, P, pl->fdev, dst, 0, pl->npairs_run, FkGeo()))) return rc;
        D4W_MARK(3);
        if (P.bs_L) rc = launch_k(fk_passC_bluestein<true>, gridC, blk, pl->ldsC, stream, P, dst, ntC);
        else rc = launch_k(F.C_inv, gC, dim3(F.thrC), F.ldsC, stream, P, pl->fdev, dst, 0, fC, NBC, 0, FkGeo());
        if (rc) return rc;
        D4W_MARK(4);
        if (row_mean) {
            const int run = stats_run(NBX, fA), nruns = fA / run;
            if ((rc = launch_k(F.A_inv_stats, dim3(std::min(nruns, pl->num_cu * pl->wgA)), dim3(F.thrA), F.ldsA, stream, P,
                               dst, run, nruns, row_mean, (unsigned*)row_maxabs, NBX, 0, FkGeo(), (const float2*)nullptr, 0))) return rc;
        } else if ((rc = launch_k(F.A_inv, gA, dim3(F.thrA), F.ldsA, stream, P, dst, 0, fA, NBX, 0, FkGeo(), (const float2*)nullptr))) return rc;
        D4W_MARK(5);
#undef D4W_MARK
        return D4W_OK;
    }
    const bool gA = pl->genericA, gB = pl->genericB, gC = pl->genericC;
    int rc;
#define D4W_MARK(i) do { if (ev) D4W_HIP(hipEventRecord(ev[i], st)); } while (0)
    D4W_MARK(0);
    if ((rc = fk_launch_passA_fwd(taper != 0, gA, gridA, blk, pl->ldsA, stream, P, src, dst, ntA))) return rc;
    D4W_MARK(1);
    if (P.bs_L) rc = launch_k(fk_passC_bluestein<false>, gridC, blk, pl->ldsC, stream, P, dst, ntC);
    else rc = fk_launch_passC(false, gC, gridC, blk, pl->ldsC, stream, P, dst, ntC);
    if (rc) return rc;
    D4W_MARK(2);
    if (P.bn_L) rc = launch_k(fk_passB_bluestein, gridB, blk, pl->ldsB, stream, P, dst, ntB);
    else rc = launch_k(gB ? fk_passB<true> : fk_passB<false>, gridB, blk, pl->ldsB, stream, P, dst, ntB);
    if (rc) return rc;
    D4W_MARK(3);
    if (P.bs_L) rc = launch_k(fk_passC_bluestein<true>, gridC, blk, pl->ldsC, stream, P, dst, ntC);
    else rc = fk_launch_passC(true, gC, gridC, blk, pl->ldsC, stream, P, dst, ntC);
    if (rc) return rc;
    D4W_MARK(4);
    if ((rc = fk_launch_passA_inv(gA, gridA, blk, pl->ldsA, stream, P, dst, ntA))) return rc;
    if (row_mean && (rc = d4w_row_stats_f32(y, d.nx, d.ns, row_mean, row_maxabs, stream))) return rc;   // generic kernels: separate pass
    D4W_MARK(5);
#undef D4W_MARK
    return D4W_OK;
}

static int fk_apply_impl(d4w_fk_plan* pl, const float* x, float* y, int taper, void* stream, hipEvent_t* ev,
                         double* row_mean = nullptr, float* row_maxabs = nullptr) {
    if (!pl || !x || !y) return fail(D4W_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(pl->apply_mu);
    int rc = fk_plan_enter(pl, stream);
    if (rc != D4W_OK) return rc;
    rc = fk_apply_run(pl, x, y, taper, stream, ev, row_mean, row_maxabs);
    const int rl = fk_plan_leave(pl, stream);
    return rc != D4W_OK ? rc : rl;
}

extern "C" {

/* Order and modelled traffic of the passes for the current mask: info[0] = 1 time-first / 0 channel-first,
 * info[1] = band columns kept per row (incl. the Nyquist column), info[2] = tail columns, info[3] = ns / 2,
 * info[4] = live wavenumber rows, info[5] = nx; bytes[0], bytes[1] = modelled bytes per channel-sample of the
 * channel-first and of the time-first order. */
int d4w_fk_plan_order(const d4w_fk_plan* pl, int* info6, double* bytes2) {
    if (!pl || !info6 || !bytes2) return fail(D4W_EINVAL, "NULL argument");
    info6[0] = pl->tf ? 1 : 0; info6[1] = pl->tf_band_cols; info6[2] = pl->tf_tail_cols; info6[3] = pl->dev.d.M;
    info6[4] = pl->live_rows; info6[5] = pl->dev.d.nx;
    bytes2[0] = pl->bytes_cf; bytes2[1] = pl->bytes_tf;
    return D4W_OK;
}

int d4w_fk_set_mask_dense_f32(d4w_fk_plan* pl, const float* mask_shifted, void* stream) {
    return fk_set_mask_impl(pl, mask_shifted, 0.0, stream);
}

int d4w_fk_set_mask_dense_pruned_f32(d4w_fk_plan* pl, const float* mask_shifted, double prune_eps, void* stream) {
    return fk_set_mask_impl(pl, mask_shifted, prune_eps, stream);
}

int d4w_fk_set_mask_dense_affine_f32(d4w_fk_plan* pl, const float* mask_shifted, float scale, float offset, void* stream) {
    return fk_set_mask_impl(pl, mask_shifted, 0.0, stream, FkAffine{scale, offset, 1});
}

int d4w_fk_set_mask_design_f32(d4w_fk_plan* pl, int mode, double k_spacing, double t_spacing, const double* params8_host,
                               int i0, int i1, const double* hrow_dev, double prune_eps, void* stream) {
    if (!pl) return fail(D4W_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(pl->apply_mu);
    int rc = fk_plan_enter(pl, stream);
    if (rc != D4W_OK) return rc;
    rc = fk_set_mask_design_run(pl, mode, k_spacing, t_spacing, params8_host, i0, i1, hrow_dev, prune_eps, stream);
    const int rl = fk_plan_leave(pl, stream);
    return rc != D4W_OK ? rc : rl;
}

int d4w_fk_plan_live_rows(const d4w_fk_plan* pl) { return pl ? pl->live_rows : -1; }

int d4w_fk_apply_f32(d4w_fk_plan* pl, const float* x, float* y, int taper, void* stream) {
    return fk_apply_impl(pl, x, y, taper, stream, nullptr);
}

int d4w_fk_stats_in_epilogue(const d4w_fk_plan* pl) { return pl && fk_stats_in_epilogue(pl) ? 1 : 0; }

int d4w_fk_apply_stats_f32(d4w_fk_plan* pl, const float* x, float* y, int taper, double* row_mean, float* row_maxabs,
                           void* stream) {
    if (!row_mean || !row_maxabs) return fail(D4W_EINVAL, "NULL argument");
    return fk_apply_impl(pl, x, y, taper, stream, nullptr, row_mean, row_maxabs);
}

int d4w_fk_apply_timed_stats_f32(d4w_fk_plan* pl, const float* x, float* y, int taper, double* row_mean,
                                 float* row_maxabs, void* stream, float* ms5) {
    if (!ms5) return fail(D4W_EINVAL, "NULL argument");
    hipEvent_t ev[6];
    for (int i = 0; i < 6; ++i) D4W_HIP(hipEventCreate(&ev[i]));
    int rc = fk_apply_impl(pl, x, y, taper, stream, ev, row_mean, row_maxabs);
    if (rc == D4W_OK) {
        hipError_t e = hipEventSynchronize(ev[5]);
        if (e != hipSuccess) rc = fail(D4W_EHIP, "hipEventSynchronize: %s", hipGetErrorString(e));
        for (int i = 0; i < 5 && rc == D4W_OK; ++i) {
            e = hipEventElapsedTime(&ms5[i], ev[i], ev[i + 1]);
            if (e != hipSuccess) rc = fail(D4W_EHIP, "hipEventElapsedTime: %s", hipGetErrorString(e));
        }
    }
    for (int i = 0; i < 6; ++i) (void)hipEventDestroy(ev[i]);
    return rc;
}

int d4w_fk_apply_timed_f32(d4w_fk_plan* pl, const float* x, float* y, int taper, void* stream, float* ms5) {
    return d4w_fk_apply_timed_stats_f32(pl, x, y, taper, nullptr, nullptr, stream, ms5);
}

/* measurement aid (not in d4w.h): run ONE pass of a shape-specialised plan over the tile range
 * [t_begin, t_end) in place on `data`.  pass: 0 A, 1 C, 2 B, 3 C', 4 A'. */
int d4w_fk_debug_run_pass(d4w_fk_plan* pl, float* data, int pass, int t_begin, int t_end, void* stream) {
    if (!pl || !data || !pl->fast) return fail(D4W_EINVAL, "needs a shape-specialised plan");
    const FkFastEntry& F = *pl->fast;
    const FkDev& P = pl->dev;
    float2* d2 = reinterpret_cast<float2*>(data);
    if (pass == 2) t_end = std::min(t_end, pl->npairs_run);
    const int n = t_end - t_begin;
    if (n <= 0) return D4W_OK;
    switch (pass) {
        case 0: return launch_k(F.A_fwd, dim3(std::min(n, pl->num_cu * pl->wgA)), dim3(F.thrA), F.ldsA, stream, P, (const float2*)d2, d2, t_begin, t_end, P.d.N2 / P.d.TA, 0, FkGeo());
        case 1: return launch_k(F.C_fwd, dim3(std::min(n, pl->num_cu * pl->wgC)), dim3(F.thrC), F.ldsC, stream, P, pl->fdev, d2, t_begin, t_end, P.d.N2 / P.d.TC, 0, FkGeo());
        case 2: return launch_k(F.B_mid, dim3(std::min(n, pl->num_cu * pl->wgB)), dim3(F.thrB), F.ldsB, stream, P, pl->fdev, d2, t_begin, t_end, FkGeo());
        case 3: return launch_k(F.C_inv, dim3(std::min(n, pl->num_cu * pl->wgC)), dim3(F.thrC), F.ldsC, stream, P, pl->fdev, d2, t_begin, t_end, P.d.N2 / P.d.TC, 0, FkGeo());
        case 4: return launch_k(F.A_inv, dim3(std::min(n, pl->num_cu * pl->wgA)), dim3(F.thrA), F.ldsA, stream, P, d2, t_begin, t_end, P.d.N2 / P.d.TA, 0, FkGeo(), (const float2*)nullptr);
    }
    return fail(D4W_EINVAL, "pass %d", pass);
}

int d4w_taper_f32(float* x, int nx, int ns, void* stream) {
    if (!x || nx < 1 || ns < 1) return fail(D4W_EINVAL, "bad argument");
    // the window's ramps, per (device, ns), uploaded once and kept (a few KB): no allocation, no host synchronisation per call
    struct Ramps { float* dev; int W; };
    static std::mutex mu;
    static std::map<std::pair<int, int>, Ramps> cache;
    int devid = 0;
    D4W_HIP(hipGetDevice(&devid));
    Ramps r{nullptr, 0};
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = cache.find({devid, ns});
        if (it == cache.end()) {
            const std::vector<float> win = tukey_window(ns, 0.03);
            int W = 0;                                             // columns at each end where the window is not 1 (it is symmetric)
            for (int i = 0; i < ns; ++i)
                if (win[i] != 1.0f || win[ns - 1 - i] != 1.0f) W = std::max(W, std::min(i, ns - 1 - i) + 1);
            W = std::min(W, ns / 2);
            std::vector<float> ramp((size_t)2 * std::max(W, 1), 1.0f);
            for (int j = 0; j < W; ++j) { ramp[j] = win[j]; ramp[W + j] = win[ns - W + j]; }
            if (ns % 2 && W == ns / 2 && win[ns / 2] != 1.0f)
                return fail(D4W_EINVAL, "taper of %d samples has no flat part", ns);       // (alpha = 0.03: never)
            float* d = nullptr;
            D4W_HIP(hipMalloc((void**)&d, ramp.size() * sizeof(float)));
            hipError_t e = hipMemcpy(d, ramp.data(), ramp.size() * sizeof(float), hipMemcpyHostToDevice);
            if (e != hipSuccess) { (void)hipFree(d); return fail(D4W_EHIP, "tukey upload failed: %s", hipGetErrorString(e)); }
            it = cache.emplace(std::make_pair(devid, ns), Ramps{d, W}).first;
        }
        r = it->second;
    }
    if (r.W == 0) return D4W_OK;                                   // the window is 1 everywhere (ns <= 1)
    const size_t total = (size_t)nx * 2 * r.W;
    const int blocks = (int)std::min<size_t>((total + kThreads - 1) / kThreads, 4096);
    D4W_LAUNCH(taper_ramps, dim3(blocks), dim3(kThreads), 0, stream, x, (const float*)r.dev, nx, ns, r.W);
    return D4W_OK;
}

}  // extern "C"
