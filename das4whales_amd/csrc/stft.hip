// STFT magnitude on MI355X (gfx950) as librosa.stft is called by the reference (dsp.py:66-68 get_spectrogram,
// detect.py:382 get_sliced_nspectrogram), with the per-channel maximum the reference normalises by (dsp.py:76,
// detect.py:387).  Every transform runs in LDS (row_fft.h); HBM-streaming work, no MFMA -- the
// detector's few kept bins go to the matrix cores instead (stft_mm.hip).
#include "row_fft.h"

namespace d4w {

// ---------------------------------------------------------------------------------------------
// |librosa.stft(y, n_fft, hop_length=hop)|: periodic Hann, center=True with zero padding,
// frame t covers samples [t*hop - n_fft/2, t*hop + n_fft/2), n_frames = 1 + ns/hop, bins 0..n_fft/2
// (SURVEY.md A.1).  A workgroup owns FT consecutive frames of one channel: the samples they cover
// are staged once in LDS, two real frames ride one complex n_fft-point transform, the bins
// [b_lo, b_hi] are written as S[c][bin - b_lo][t] (t fastest) and the maximum over ALL bins and
// frames goes to rowmax[c] (the reference normalises by the full spectrogram's max before it
// slices, detect.py:387,390).
// ---------------------------------------------------------------------------------------------
struct StftDims {
    int ns, n_fft, hop, nframes, FT, b_lo, b_hi;
};

// (GENERIC, two waves per SIMD: the prime-radix stage functions it calls take their register budget from the kernels of
// their unit, and 256-thread kernels alone would leave them the whole file -- one workgroup per CU)
template <bool GENERIC>
__global__ __launch_bounds__(kSpThreads, GENERIC ? 2 : 1) void stft_mag(RowFftDev F, StftDims d, const float* __restrict__ x,
                                                       float* __restrict__ S, unsigned* __restrict__ rowmax) {
    D4W_DYN_LDS(smem_raw);
    float2* tile = reinterpret_cast<float2*>(smem_raw);
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int n_fft = d.n_fft, nb = d.FT / 2;
    // TL: LDS elements per transform -- the frame itself, or the Bluestein convolution length when n_fft has a prime factor
    // > 31 (x chirp -> FFT -> x filter -> inverse FFT -> x chirp, as row_dft; spectra in natural order then)
    const int TL = F.bs_L ? F.bs_L : n_fft;
    const AxisDesc& axt = row_tw_axis(F);
    const TwLds tw = tw_stage(axt, tile + nb * TL, tid, nthr);
    float* seg = reinterpret_cast<float*>(tile + nb * TL + tw_lds_elems(axt));
    const int seg_len = (d.FT - 1) * d.hop + n_fft;
    const int t0 = blockIdx.x * d.FT;
    const int s0 = t0 * d.hop - n_fft / 2;
    const float* xr = x + (size_t)blockIdx.y * d.ns;
    for (int j = tid; j < seg_len; j += nthr) {
        const int s = s0 + j;
        seg[j] = (s >= 0 && s < d.ns) ? xr[s] : 0.f;
    }
    lds_barrier();
    const FDiv dn(TL), dnb(nb);
    for (int w = tid; w < nb * TL; w += nthr) {
        const int b = dn.div(w), n = w - b * TL;
        float2 v = make_float2(0.f, 0.f);
        if (n < n_fft) {
            const float wn = F.hann[n];
            v = make_float2(seg[2 * b * d.hop + n] * wn, seg[(2 * b + 1) * d.hop + n] * wn);
            if (F.bs_L) v = c_mul(v, F.bs_chirp[n]);
        }
        tile[w] = v;
    }
    lds_barrier();
    if (F.bs_L) {
        lds_fft<false, false, false>(tile, F.ax_bs, tw, 1, nb, TL, 1, 0, tid, nthr);
        for (int w = tid; w < nb * TL; w += nthr) tile[w] = c_mul(tile[w], F.bs_filt[w - dn.div(w) * TL]);
        lds_barrier();
        lds_fft<true, false, false>(tile, F.ax_bs, tw, 1, nb, TL, 1, 0, tid, nthr);
        for (int w = tid; w < nb * n_fft; w += nthr) {
            const int b = w / n_fft, k = w - b * n_fft;
            tile[b * TL + k] = c_mul(tile[b * TL + k], F.bs_chirp[k]);
        }
        lds_barrier();
    } else {
        lds_fft<false, false, GENERIC>(tile, F.ax, tw, 1, nb, n_fft, 1, 0, tid, nthr);
    }
    const int nbins = n_fft / 2 + 1, nkeep = d.b_hi - d.b_lo + 1;
    float mx = 0.f;
    for (int w = tid; w < nbins * nb; w += nthr) {
        const int k = dnb.div(w), b = w - k * nb;
        const int tA = t0 + 2 * b;
        if (tA >= d.nframes) continue;
        const float2* tb = tile + b * TL;
        const float2 zk = tb[F.pos[k]], zm = c_conj(tb[F.pos[(k == 0) ? 0 : n_fft - k]]);
        const float2 A = c_scale(c_add(zk, zm), 0.5f);
        const float2 B = c_mul_mi(c_scale(c_sub(zk, zm), 0.5f));
        const float ma = sqrtf(fmaf(A.x, A.x, A.y * A.y)), mb = sqrtf(fmaf(B.x, B.x, B.y * B.y));
        const bool hasB = (tA + 1 < d.nframes);
        mx = fmaxf(mx, ma);
        if (hasB) mx = fmaxf(mx, mb);
        if (k >= d.b_lo && k <= d.b_hi) {
            float* o = S + ((size_t)blockIdx.y * nkeep + (k - d.b_lo)) * d.nframes + tA;
            o[0] = ma;
            if (hasB) o[1] = mb;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if ((tid & 63) == 0) atomicMax(rowmax + blockIdx.y, __float_as_uint(mx));   // mx >= 0: bit order = value order
}

// The same for frame lengths n_fft = RA * RB with both factors register butterflies (160 = 10 x 16, the detector's
// 0.8-s window; 128, 256, 512): one DIF split n = j + RB a, k = k1 + RA k2 --
//   S1 item (pair b, j)  : the RA windowed samples of two real frames (one complex value each), radix RA, x W_N^(j k1) -> LDS
//   S2 item (pair b, k1) : radix RB over j -> Z[k1 + RA k2], back in place
//   then the magnitudes of the kept bins (all bins when the row maximum is wanted) from Z[k] and conj Z[N - k].
// Two LDS round trips per transform instead of the generic kernel's staging pass + three runtime-radix stages:
// 5.5 -> see DESIGN.md 3.4 at 11020 x 12000, n_fft 160, hop 8.
template <int RA, int RB>
__global__ __launch_bounds__(kSpThreads) void stft_fat(RowFftDev F, StftDims d, const float* __restrict__ x,
                                                       float* __restrict__ S, unsigned* __restrict__ rowmax) {
    D4W_DYN_LDS(smem_raw);
    constexpr int N = RA * RB, PB = RB + 1, TP = RA * PB;           // LDS pitch of a k1 row / of a transform
    float2* buf = reinterpret_cast<float2*>(smem_raw);                // [nb][RA][RB + 1]
    const int tid = threadIdx.x, nb = d.FT / 2;
    float2* twl = buf + nb * TP;                                      // [RA][RB] W_N^(j k1)
    float* win = reinterpret_cast<float*>(twl + N);                   // [N]
    float* seg = win + N;
    const int seg_len = (d.FT - 1) * d.hop + N;
    const float* xr = x + (size_t)blockIdx.y * d.ns;
    for (int i = tid; i < N; i += kSpThreads) {
        const int k1 = i / RB, j = i - k1 * RB;
        twl[i] = F.wfull[(j * k1) % N];
        win[i] = F.hann[i];
    }
    float mx = 0.f;
    // a workgroup walks several frame tiles of its row: the twiddle / window tables are staged once, and a long record
    // is a few thousand workgroups instead of half a million
    const int ntiles = (d.nframes + d.FT - 1) / d.FT;
    // the samples of the NEXT tile travel in registers while this one is transformed (kSegPer per lane; longer segments --
    // large hops -- load the remainder directly)
    constexpr int kSegPer = 4;
    float nxt[kSegPer];
    auto seg_fetch = [&](int tile) {
        const int s0 = tile * d.FT * d.hop - N / 2;
#pragma unroll
        for (int k = 0; k < kSegPer; ++k) {
            const int j = tid + k * kSpThreads, sidx = s0 + j;
            nxt[k] = (j < seg_len && sidx >= 0 && sidx < d.ns) ? xr[sidx] : 0.f;
        }
    };
    if ((int)blockIdx.x < ntiles) seg_fetch(blockIdx.x);
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int t0 = tile * d.FT;
    const int s0 = t0 * d.hop - N / 2;
#pragma unroll
    for (int k = 0; k < kSegPer; ++k) {
        const int j = tid + k * kSpThreads;
        if (j < seg_len) seg[j] = nxt[k];
    }
    for (int j = tid + kSegPer * kSpThreads; j < seg_len; j += kSpThreads) {
        const int sidx = s0 + j;
        seg[j] = (sidx >= 0 && sidx < d.ns) ? xr[sidx] : 0.f;
    }
    __syncthreads();
    if (tile + (int)gridDim.x < ntiles) seg_fetch(tile + gridDim.x);
    for (int it = tid; it < nb * RB; it += kSpThreads) {              // S1
        const int b = it / RB, j = it - b * RB;
        const float* sa = seg + 2 * b * d.hop + j;
        const float* sb = sa + d.hop;
        float2 z[RA];
        static_for<RA>([&](auto aa) {
            constexpr int a = decltype(aa)::value;
            const float wn = win[j + RB * a];
            z[a] = make_float2(sa[RB * a] * wn, sb[RB * a] * wn);
        });
        dft<RA>(z);
        float2* o = buf + b * TP + j;
        static_for<RA>([&](auto kk) {
            constexpr int k1 = decltype(kk)::value;
            o[k1 * PB] = (k1 == 0) ? z[0] : c_mul(z[k1], twl[k1 * RB + j]);
        });
    }
    __syncthreads();
    for (int it = tid; it < nb * RA; it += kSpThreads) {              // S2
        const int b = it / RA, k1 = it - b * RA;
        float2* r = buf + b * TP + k1 * PB;
        float2 v[RB];
        static_for<RB>([&](auto jj) { v[decltype(jj)::value] = r[decltype(jj)::value]; });
        dft<RB>(v);
        static_for<RB>([&](auto kk) { r[decltype(kk)::value] = v[decltype(kk)::value]; });
    }
    __syncthreads();
    // Z[k] of transform b sits at buf[b][(k % RA)][k / RA]
    const int klo = rowmax ? 0 : d.b_lo, khi = rowmax ? N / 2 : d.b_hi, nk = khi - klo + 1, nkeep = d.b_hi - d.b_lo + 1;
    for (int w = tid; w < nk * nb; w += kSpThreads) {
        const int kk = w / nb, b = w - kk * nb, k = klo + kk;
        const int tA = t0 + 2 * b;
        if (tA >= d.nframes) continue;
        const float2* tb = buf + b * TP;
        const int km = (k == 0) ? 0 : N - k;
        const float2 zk = tb[(k % RA) * PB + k / RA], zm = c_conj(tb[(km % RA) * PB + km / RA]);
        const float2 A = c_scale(c_add(zk, zm), 0.5f);
        const float2 B = c_mul_mi(c_scale(c_sub(zk, zm), 0.5f));
        const float ma = sqrtf(fmaf(A.x, A.x, A.y * A.y)), mb = sqrtf(fmaf(B.x, B.x, B.y * B.y));
        const bool hasB = (tA + 1 < d.nframes);
        mx = fmaxf(mx, ma);
        if (hasB) mx = fmaxf(mx, mb);
        if (k >= d.b_lo && k <= d.b_hi) {
            float* o = S + ((size_t)blockIdx.y * nkeep + (k - d.b_lo)) * d.nframes + tA;
            o[0] = ma;
            if (hasB) o[1] = mb;
        }
    }
    __syncthreads();                                              // seg / buf are refilled by the next tile
    }
    if (rowmax) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
        if ((tid & 63) == 0) atomicMax(rowmax + blockIdx.y, __float_as_uint(mx));   // mx >= 0: bit order = value order
    }
}

// S[c][i] /= denom[c]  (mode 0, detect.py:387)   or   20 log10(S[c][i] / denom[c])  (mode 1, dsp.py:76)
__global__ __launch_bounds__(kSpThreads) void scale_rows(float* __restrict__ S, size_t per_row,
                                                         const float* __restrict__ denom, int mode) {
    float* row = S + (size_t)blockIdx.y * per_row;
    const float dv = denom[blockIdx.y];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_row; i += (size_t)gridDim.x * blockDim.x) {
        const float v = row[i] / dv;
        row[i] = mode ? 20.0f * log10f(v) : v;
    }
}

}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_stft_frames(int ns, int hop) { return (hop > 0 && ns >= 0) ? 1 + ns / hop : 0; }

int d4w_stft_mag_f32(const float* x, float* S, float* rowmax, int nx, int ns, int n_fft, int hop, int bin_lo,
                     int bin_hi, void* stream) {
    if (!x || !S || nx < 1 || ns < 1) return fail(D4W_EINVAL, "bad argument");
    // a few kept bins of a heavily overlapped transform and no row maximum wanted (the detector's call): frames x DFT rows
    // as a matrix product on the matrix cores (stft_mm.hip) instead of one FFT per frame
    if (!rowmax && d4w_stft_mm_eligible(n_fft, hop, bin_lo, bin_hi))
        return d4w_stft_mag_mm_f32(x, S, nx, ns, n_fft, hop, bin_lo, bin_hi, stream);
    if (n_fft < 2 || (n_fft & 1) || hop < 1) return fail(D4W_EINVAL, "n_fft = %d must be even and >= 2, hop = %d >= 1", n_fft, hop);
    if (bin_lo < 0 || bin_hi > n_fft / 2 || bin_lo > bin_hi) return fail(D4W_EINVAL, "bin range [%d, %d] outside 0..%d", bin_lo, bin_hi, n_fft / 2);
    if (nx > 65535) return fail(D4W_EINVAL, "nx = %d exceeds the grid limit 65535", nx);
    const RowFftHost* h = nullptr;
    int rc = row_fft_get(n_fft, &h);
    if (rc) return rc;
    StftDims d;
    d.ns = ns; d.n_fft = n_fft; d.hop = hop; d.nframes = 1 + ns / hop; d.b_lo = bin_lo; d.b_hi = bin_hi;
    const int tl = h->dev.bs_L ? h->dev.bs_L : n_fft;        // LDS elements per transform (Bluestein: the convolution length)
    int nb = std::max(1, 6144 / tl);                         // complex transforms (frame pairs) per workgroup
    // two-factor frame lengths: 16 pairs make the first stage exactly one item per thread (RB = 16) and keep the tile at
    // 22-35 KB, i.e. 16-24 waves on a CU instead of 8 (measured at 11020 x 12000: n_fft 160 kept bins 2.61 -> 1.80 ms, all bins
    // 3.98 -> 2.77 ms, n_fft 256 5.05 -> 3.70 ms)
    if (n_fft == 128 || n_fft == 160 || n_fft == 256) nb = 16;
    else if (n_fft == 512) nb = 8;
    {
        static const int nb_env = [] { const char* v = getenv("D4W_STFT_NB"); return v ? atoi(v) : 0; }();
        if (nb_env > 0) nb = nb_env;
    }
    nb = std::min(nb, std::max(1, (d.nframes + 1) / 2));
    d.FT = 2 * nb;
    // two-factor register transforms for the common frame lengths (rowmax may be NULL there: only the kept bins are formed)
    {
        static const int fat_env = [] { const char* v = getenv("D4W_STFT_FAT"); return v ? atoi(v) : 1; }();
        int RA = 0, RB = 0;
        if (n_fft == 160) { RA = 10; RB = 16; }
        else if (n_fft == 128) { RA = 8; RB = 16; }
        else if (n_fft == 256) { RA = 16; RB = 16; }
        else if (n_fft == 512) { RA = 32; RB = 16; }
        if (RA && fat_env) {
            const size_t ldsf = ((size_t)nb * RA * (RB + 1) + n_fft) * sizeof(float2) +
                                ((size_t)n_fft + (size_t)(d.FT - 1) * hop + n_fft) * sizeof(float);
            if (ldsf <= kSpLdsMax) {
                if (rowmax) D4W_HIP(hipMemsetAsync(rowmax, 0, (size_t)nx * sizeof(float), (hipStream_t)stream));
                // tiles per row walked by min(tiles, ~8192 / nx) workgroups (one per row for a whole file, all tiles in parallel
                // for a single channel)
                const int ntile = ceil_div(d.nframes, d.FT);
                const dim3 gridf(std::max(1, std::min(ntile, 8192 / std::max(nx, 1))), nx);
#define D4W_FAT(A_, B_)                                                                                             \
    do {                                                                                                            \
        allow_lds(stft_fat<A_, B_>, ldsf);                                                                          \
        D4W_LAUNCH((stft_fat<A_, B_>), gridf, dim3(kSpThreads), ldsf, stream, h->dev, d, x, S, (unsigned*)rowmax);  \
    } while (0)
                if (n_fft == 160) D4W_FAT(10, 16);
                else if (n_fft == 128) D4W_FAT(8, 16);
                else if (n_fft == 256) D4W_FAT(16, 16);
                else D4W_FAT(32, 16);
#undef D4W_FAT
                return D4W_OK;
            }
        }
    }
    if (!rowmax) return fail(D4W_EINVAL, "rowmax is NULL (only the two-factor frame lengths 128, 160, 256, 512 form the kept bins alone)");
    // nb transform tiles, one twiddle table, the staged samples
    const size_t lds = row_tile_bytes(tl) + (size_t)(nb - 1) * tl * sizeof(float2) + ((size_t)(d.FT - 1) * hop + n_fft) * sizeof(float);
    if (lds > kSpLdsMax) return fail(D4W_EINVAL, "n_fft = %d / hop = %d exceed the LDS frame tile", n_fft, hop);
    D4W_HIP(hipMemsetAsync(rowmax, 0, (size_t)nx * sizeof(float), (hipStream_t)stream));
    const dim3 grid(ceil_div(d.nframes, d.FT), nx);
    return with_flag(h->generic, [&](auto G) {
        constexpr auto kern = stft_mag<decltype(G)::value>;
        allow_lds(kern, lds);
        D4W_LAUNCH(kern, grid, dim3(kSpThreads), lds, stream, h->dev, d, x, S, (unsigned*)rowmax);
        return (int)D4W_OK;
    });
}

int d4w_scale_rows_f32(float* S, int nx, size_t per_row, const float* denom, int mode, void* stream) {
    if (!S || !denom || nx < 1 || per_row < 1) return fail(D4W_EINVAL, "bad argument");
    if (nx > 65535) return fail(D4W_EINVAL, "nx = %d exceeds the grid limit 65535", nx);
    const int bx = (int)std::min<size_t>((per_row + kSpThreads - 1) / kSpThreads, 256);
    D4W_LAUNCH(scale_rows, dim3(bx, nx), dim3(kSpThreads), 0, stream, S, per_row, denom, mode);
    return D4W_OK;
}

}  // extern "C"
