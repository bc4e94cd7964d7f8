// The transform plan of the row operators: one cached set of device tables per (device, length), shared by the analytic
// signal (analytic.hip), the STFT (stft.hip), the noise floor (noise.hip) and Welch's PSD (welch.hip), with the device
// helpers that run a single-row transform from it and the host helpers that size and launch such kernels.
#pragma once
#include <type_traits>

#include "fft_host.h"

namespace d4w {

constexpr int kSpThreads = 256;
constexpr size_t kSpLdsMax = 150 * 1024;      // dynamic LDS a single-row transform may use
constexpr int kAnMaxThreads = 512;

struct RowFftDev {
    AxisDesc ax;
    const int* pos;       // [L] frequency -> LDS position after the forward (DIF) transform
    const int* p2f;       // [L] position -> frequency
    const float2* wpack;  // [L] exp(-2 pi i f / (2L)): real-packing twiddle of a 2L-point real row
    const float* hann;    // [L] periodic Hann window (scipy get_window('hann', L, fftbins=True))
    const float2* wfull;  // [L] exp(-2 pi i m / L)
    // Bluestein form for a length with a prime factor > 31 (single-row transforms only): the L-point DFT as a
    // circular convolution of length bs_L = 2^a 3^b 5^c >= 2 L - 1 with the chirp exp(-i pi n^2 / L); pos / p2f are the
    // identity then.  bs_L = 0: the mixed-radix transform of `ax`.
    int bs_L;
    AxisDesc ax_bs;
    const float2* bs_chirp;   // [L]
    const float2* bs_filt;    // [bs_L]  FFT of the wrapped conjugate chirp / bs_L, at the DIF positions of ax_bs
};

struct RowFftHost {
    RowFftDev dev;
    bool generic;
    double sumw2;         // sum(w^2) of the float64 Hann window, SciPy's density scale (welch.hip)
    std::vector<void*> allocs;
};

// the plan of length L on the current device, built on first use and kept for the life of the process (row_fft.hip)
int row_fft_get(int L, const RowFftHost** out);
// LDS elements of a single-row transform of length L: L, or the Bluestein convolution length.  Builds no plan.
int row_fft_tile_elems(int L);

// bytes of a transform tile of `elems` complex values and the two-level twiddle table behind it (fft_host.h twiddle_table2)
inline size_t row_tile_bytes(size_t elems) { return (elems + kTwLo + (elems + kTwLo - 1) / kTwLo) * sizeof(float2); }
inline size_t row_tile_lds(const RowFftDev& F) { return row_tile_bytes(F.bs_L ? F.bs_L : F.ax.L); }

template <typename K>
inline void allow_lds(K kern, size_t bytes) {
    if (bytes > 64 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// f(std::bool_constant<b>{}): the launch of a kernel template picked by a run-time flag, written once
template <typename F>
inline int with_flag(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <typename F>
inline int with_flags(bool a, bool b, F&& f) {
    return with_flag(a, [&](auto A) { return with_flag(b, [&](auto B) { return f(A, B); }); });
}

// elements / twiddle axis of a single-row transform tile
__device__ __forceinline__ int row_tile_elems(const RowFftDev& F) { return F.bs_L ? F.bs_L : F.ax.L; }
__device__ __forceinline__ const AxisDesc& row_tw_axis(const RowFftDev& F) { return F.bs_L ? F.ax_bs : F.ax; }

// DFT (INV = false) or unnormalised inverse DFT of the F.ax.L values at the start of `tile`, in place; result at
// positions F.pos[f].  The tile is synchronised on entry and on return.  Bluestein form when F.bs_L != 0 (the tile
// then holds F.bs_L elements): x w -> FFT -> x filter -> IFFT -> x w, w = exp(-i pi n^2 / L), conjugated for INV.
template <bool INV, bool GENERIC>
__device__ __forceinline__ void row_dft(float2* tile, const RowFftDev& F, const TwLds tw, int tid, int nthr) {
    if (F.bs_L == 0) {
        lds_fft<INV, false, GENERIC>(tile, F.ax, tw, 1, 1, 0, 1, 0, tid, nthr);
        return;
    }
    const int L = F.ax.L, BL = F.bs_L;
    for (int i = tid; i < BL; i += nthr) {
        float2 v = make_float2(0.f, 0.f);
        if (i < L) v = INV ? c_mulc(tile[i], F.bs_chirp[i]) : c_mul(tile[i], F.bs_chirp[i]);
        tile[i] = v;
    }
    lds_barrier();
    lds_fft<false, false, false>(tile, F.ax_bs, tw, 1, 1, 0, 1, 0, tid, nthr);
    for (int i = tid; i < BL; i += nthr) tile[i] = INV ? c_mulc(tile[i], F.bs_filt[i]) : c_mul(tile[i], F.bs_filt[i]);
    lds_barrier();
    lds_fft<true, false, false>(tile, F.ax_bs, tw, 1, 1, 0, 1, 0, tid, nthr);
    for (int i = tid; i < L; i += nthr) tile[i] = INV ? c_mulc(tile[i], F.bs_chirp[i]) : c_mul(tile[i], F.bs_chirp[i]);
    lds_barrier();
}

}  // namespace d4w
