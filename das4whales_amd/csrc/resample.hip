// Polyphase resampling and FIR decimation along time on MI355X (gfx950): scipy.signal.resample_poly / decimate(ftype='fir')
// of every row, and the same kernel reading raw rows (the fused ingest of a file that is not at the working rate).
// DESIGN.md section 3.11.
//
// up, down are reduced by their gcd (1/1 is a copy); h = ntaps float32 taps (the caller has multiplied them by up),
// half = (ntaps - 1) / 2, n_out = ceil(ns up / down), and for every row r and output m < n_out
//
//     y[r][m] = back_r + scale * sum_i (xv[r][i] - off_r) h[m down + half - i up]
//
// over all i with 0 <= m down + half - i up < ntaps for which xv[r][i] exists: xv is x[r][i] for 0 <= i < ns,
// left[r][n_left + i] for -n_left <= i < 0 and right[r][i - ns] for ns <= i < ns + n_right.  A sample that does not exist
// contributes nothing (the zero padding follows the removal of the offset).  back_r is 0, off_r (the offset is put back as it
// was: padtype='mean'), or scale off_r sum_j h[t + j up] over the taps t of the output's phase (the record continues as the
// constant off_r beyond its ends, which is what SciPy's padtype='constant' with cval computes; the taps of a phase sum to
// 1 only within ~1e-3 for up > 1).
//
// Output m = k up + phi (phi < up) takes the samples i = k down + c_phi - j, j = 0, 1, ..., with the taps
// h[t_phi + j up], where c_phi = (phi down + half) / up and t_phi = (phi down + half) % up: for a fixed phase and tap, the
// threads that own consecutive k read samples `down` apart.  A workgroup owns kt consecutive k of one row (all phases: kt up
// consecutive outputs).  It stages the samples they reach in LDS BY RESIDUE -- the sample u places after the tile's first
// one sits at [u % down][u / down] -- so that for every (phase, tap) the lanes of a wave read consecutive words of one
// residue row (the plain layout would be a gcd(down, 32)-way bank conflict), and the taps beside them as a [phase][j] table,
// read four at a time at a wave-uniform address.  A thread owns kResPer values of k, 256 apart, walks the phases one after
// the other and sums each output alone, in ascending tap order: no atomics, and the bits of an output do not depend on where
// the tile boundaries fall (a neighbour block continues a row bit for bit).  HBM traffic: the row once (the tiles' reach
// overlaps by ntaps / up samples in kt down) and the output once.
#include <algorithm>
#include <climits>

#include "d4w_internal.h"

namespace d4w {

constexpr int kResThreads = 256;
constexpr int kResPer = 4;                         // values of k per thread
constexpr int kResTile = 10240;                    // floats of staged samples per workgroup (40 KiB: three workgroups and more per CU)
constexpr int kResMaxTaps = 2048;
constexpr int kResMaxRate = 256;                   // up and down after the reduction

struct ResDims {
    int ns, n_out, up, down, half;
    int nk, kt, ntiles;       // values of k per row, per tile, tiles per row
    int jpad;                 // taps of a phase, zero padded to a multiple of 4
    int ilo;                  // first staged sample of the tile of k = 0: half / up - (jpad - 1)
    int cspan;                // samples one k reaches over all phases
    int pitch;                // floats of a residue row (odd: consecutive samples are stored `pitch` apart)
    int hp_off;               // where the tap table starts in LDS (floats, a multiple of 4)
    int n_left, n_right;
    int c0, cstep;            // row r is row c0 + r cstep of x
    int add_back;
    size_t ld_x, ld_left, ld_right;
    double scale, off_const;
};

template <typename T, bool RAW>
__global__ __launch_bounds__(kResThreads) void resample_rows(ResDims d, const T* __restrict__ x, const float* __restrict__ left,
                                                             const float* __restrict__ right, const float* __restrict__ taps,
                                                             int ntaps, const double* __restrict__ off, float* __restrict__ y) {
    D4W_DYN_LDS(smem_raw);
    float* tile = reinterpret_cast<float*>(smem_raw);                 // [down][pitch], then kResPer x 256 floats nobody writes
    float* hp = tile + d.hp_off;                                      // [up][jpad]
    const int tid = threadIdx.x, up = d.up, down = d.down;
    const unsigned row = blockIdx.x / (unsigned)d.ntiles, t = blockIdx.x - row * (unsigned)d.ntiles;
    const int k0 = (int)t * d.kt, kt = min(d.kt, d.nk - k0);
    // the taps by phase: hp[phi][j] = h[t_phi + j up], zeros behind the last one
    for (int e = tid; e < up * d.jpad; e += kResThreads) {
        const int phi = e / d.jpad, j = e - phi * d.jpad;
        const int tap = (phi * down + d.half) % up + j * up;
        hp[e] = (tap < ntaps) ? taps[tap] : 0.f;
    }
    const double offd = off ? off[row] : d.off_const;
    Mean2 m2;
    m2.hi = (float)offd;
    m2.lo = (float)(offd - (double)m2.hi);
    const T* xr = x + ((size_t)d.c0 + (size_t)row * d.cstep) * d.ld_x;
    const float* lr = left ? left + (size_t)row * d.ld_left + d.n_left : nullptr;     // lr[i], -n_left <= i < 0
    const float* rr = right ? right + (size_t)row * d.ld_right : nullptr;             // rr[i - ns]
    const int i0 = k0 * down + d.ilo;
    const int span = (kt - 1) * down + d.cspan;
    // the offset leaves a float32 sample as (x - hi) - lo (d4w_internal.h, Mean2), a raw one in float64 before it is rounded
    auto conv = [&](T v) -> float {
        if constexpr (RAW) return (float)((double)v - offd);
        else return demean(v, m2);
    };
    auto fetch = [&](int i) -> float {
        if (i >= 0 && i < d.ns) return conv(xr[i]);
        if (i < 0) return (lr && i >= -d.n_left) ? demean(lr[i], m2) : 0.f;
        return (rr && i - d.ns < d.n_right) ? demean(rr[i - d.ns], m2) : 0.f;
    };
    // sample u of the tile goes to [u % down][u / down]; kAhead loads of a lane are in flight at once (a tile is a few loads
    // per lane: one at a time, each waited for, left the kernel at the latency of its loads, 1.5 TB/s)
    auto stage = [&](auto get) {
        constexpr int kAhead = sizeof(T) < 4 ? 16 : 8;
        const int drho = kResThreads % down, dq = kResThreads / down;
        int rho = tid % down, q = tid / down;
        for (int u0 = tid; u0 < span; u0 += kAhead * kResThreads) {
            float v[kAhead];
#pragma unroll
            for (int e = 0; e < kAhead; ++e) v[e] = get(min(u0 + e * kResThreads, span - 1));
#pragma unroll
            for (int e = 0; e < kAhead; ++e) {
                if (u0 + e * kResThreads < span) tile[rho * d.pitch + q] = v[e];
                rho += drho;
                q += dq;
                if (rho >= down) { rho -= down; ++q; }
            }
        }
    };
    if (i0 >= 0 && i0 + span <= d.ns) {                               // inside the row: plain loads, no branch between them
        const T* src = xr + i0;
        stage([&](int u) { return conv(src[u]); });
    } else {
        stage([&](int u) { return fetch(i0 + u); });
    }
    __syncthreads();
    // add_back = 2: the record continues as the constant off_r, which every phase passes with its own gain
    double* gain = reinterpret_cast<double*>(hp + up * d.jpad);       // [up]
    if (d.add_back == 2) {
        for (int phi = tid; phi < up; phi += kResThreads) {
            double g = 0.0;
            for (int j = 0; j < d.jpad; ++j) g += (double)hp[phi * d.jpad + j];
            gain[phi] = g;
        }
        __syncthreads();
    }
    float* yr = y + (size_t)row * d.n_out;
    for (int phi = 0; phi < up; ++phi) {
        const int c = (phi * down + d.half) / up;                     // the newest sample of output k up + phi is k down + c
        int rho = (c - d.ilo) % down, qo = (c - d.ilo) / down;
        const float4* w4 = reinterpret_cast<const float4*>(hp + phi * d.jpad);
        const double back = d.add_back == 2 ? d.scale * offd * gain[phi] : d.add_back ? offd : 0.0;
        float acc[kResPer];
#pragma unroll
        for (int s = 0; s < kResPer; ++s) acc[s] = 0.f;
        // a thread whose k lies beyond the tile reads what nobody wrote (inside the allocation) and stores nothing
        for (int j4 = 0; j4 < d.jpad / 4; ++j4) {
            const float4 w = w4[j4];
            const float wj[4] = {w.x, w.y, w.z, w.w};
            float v[4][kResPer];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float* src = tile + rho * d.pitch + qo + tid;
#pragma unroll
                for (int s = 0; s < kResPer; ++s) v[e][s] = src[s * kResThreads];
                if (--rho < 0) { rho = down - 1; --qo; }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int s = 0; s < kResPer; ++s) acc[s] = fmaf(v[e][s], wj[e], acc[s]);
        }
#pragma unroll
        for (int s = 0; s < kResPer; ++s) {
            const int kl = tid + s * kResThreads;
            const long long m = (long long)(k0 + kl) * up + phi;
            if (kl < kt && m < d.n_out) yr[m] = (float)((double)acc[s] * d.scale + back);
        }
    }
}

__global__ __launch_bounds__(kResThreads) void resample_copy(const float* __restrict__ x, size_t ld_x, int ns, float* __restrict__ y) {
    const float* s = x + (size_t)blockIdx.y * ld_x;
    float* o = y + (size_t)blockIdx.y * ns;
    for (int c = blockIdx.x * kResThreads + threadIdx.x; c < ns; c += gridDim.x * kResThreads) o[c] = s[c];
}

// mean[r] of raw row c0 + r cstep as float64: integers are summed as integers (exact), floats in float64
template <typename T, typename Acc>
__global__ __launch_bounds__(kResThreads) void raw_row_mean(const T* __restrict__ raw, int ns, int c0, int cstep, double* __restrict__ mean) {
    __shared__ Acc red[kResThreads / 64];
    const T* row = raw + ((size_t)c0 + (size_t)blockIdx.x * cstep) * ns;
    const int tid = threadIdx.x;
    Acc s = 0;
    constexpr int kAhead = 8;
    for (int i0 = tid; i0 < ns; i0 += kAhead * kResThreads) {
        T v[kAhead];
#pragma unroll
        for (int e = 0; e < kAhead; ++e) {
            const int i = i0 + e * kResThreads;
            v[e] = (i < ns) ? row[i] : (T)0;
        }
#pragma unroll
        for (int e = 0; e < kAhead; ++e) s += (Acc)v[e];
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        Acc tsum = red[0];
        for (int w = 1; w < kResThreads / 64; ++w) tsum += red[w];
        mean[blockIdx.x] = (double)tsum / (double)ns;
    }
}

static int res_gcd(int a, int b) {
    while (b) { const int r = a % b; a = b; b = r; }
    return a;
}

// everything the kernel needs of (ns, ntaps, up, down), after the reduction; D4W_EINVAL beyond the limits
static int res_dims(int nx, int ns, int ntaps, int up, int down, ResDims* out) {
    if (nx < 1 || ns < 1) return fail(D4W_EINVAL, "bad argument");
    if (up < 1 || down < 1) return fail(D4W_EINVAL, "up = %d and down = %d must be positive", up, down);
    const int g = res_gcd(up, down);
    up /= g;
    down /= g;
    if (up > kResMaxRate || down > kResMaxRate)
        return fail(D4W_EINVAL, "up / down = %d / %d beyond %d after the reduction", up, down, kResMaxRate);
    if (ntaps < 1 || ntaps > kResMaxTaps) return fail(D4W_EINVAL, "%d taps outside 1..%d", ntaps, kResMaxTaps);
    const long long n_out = ((long long)ns * up + down - 1) / down;
    if (n_out > INT_MAX - 2 * kResTile || ns > INT_MAX - 2 * kResTile) return fail(D4W_EINVAL, "row of %d samples too long", ns);
    ResDims d;
    memset(&d, 0, sizeof(d));
    d.ns = ns; d.n_out = (int)n_out; d.up = up; d.down = down; d.half = (ntaps - 1) / 2;
    d.jpad = (ceil_div(ntaps, up) + 3) & ~3;
    d.ilo = d.half / up - (d.jpad - 1);
    d.cspan = ((up - 1) * down + d.half) / up - d.ilo + 1;
    d.nk = ceil_div(d.n_out, up);
    d.kt = std::min(kResPer * kResThreads, (kResTile - d.cspan) / down + 1);
    d.ntiles = ceil_div(d.nk, d.kt);
    if ((long long)nx * d.ntiles > 0x7FFFFFFFLL) return fail(D4W_EINVAL, "nx x tiles = %d x %d exceeds the grid limit", nx, d.ntiles);
    d.pitch = ceil_div((d.kt - 1) * down + d.cspan, down) | 1;
    d.hp_off = (down * d.pitch + kResPer * kResThreads + 3) & ~3;
    d.cstep = 1;
    d.scale = 1.0;
    *out = d;
    return D4W_OK;
}

static size_t res_lds_bytes(const ResDims& d) { return (size_t)(d.hp_off + d.up * d.jpad) * sizeof(float) + (size_t)d.up * sizeof(double); }

}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_resample_max_taps(void) { return kResMaxTaps; }

int d4w_resample_out_len(int ns, int up, int down) {
    if (ns < 1 || up < 1 || down < 1) return 0;
    const long long n = ((long long)ns * up + down - 1) / down;
    return n > INT_MAX ? 0 : (int)n;
}

int d4w_resample_reach(int ntaps, int up, int down, int* n_left, int* n_right) {
    if (!n_left || !n_right || ntaps < 1 || up < 1 || down < 1) return fail(D4W_EINVAL, "bad argument");
    const int g = res_gcd(up, down);
    up /= g;
    down /= g;
    const int half = (ntaps - 1) / 2;
    *n_left = (ntaps - 1 - half) / up;                                 // output 0 ends on tap ntaps - 1
    *n_right = (half >= down) ? (half - down) / up + 1 : 0;            // output ns up / down - 1 starts on tap (half - down) % up
    return D4W_OK;
}

int d4w_resample_f32(const float* x, size_t ld_x, int nx, int ns, const float* left, size_t ld_left, int n_left,
                     const float* right, size_t ld_right, int n_right, const float* taps, int ntaps, int up, int down,
                     const double* off, double off_const, double scale, int add_back, float* y, void* stream) {
    if (!x || !y || !taps || ld_x < (size_t)std::max(ns, 0)) return fail(D4W_EINVAL, "bad argument");
    ResDims d;
    int rc = res_dims(nx, ns, ntaps, up, down, &d);
    if (rc) return rc;
    if (!left) n_left = 0;
    if (!right) n_right = 0;
    if (add_back < 0 || add_back > 2) return fail(D4W_EINVAL, "add_back = %d (0 nothing, 1 the offset, 2 the offset through the filter)", add_back);
    if (n_left < 0 || n_right < 0 || ld_left < (size_t)n_left || ld_right < (size_t)n_right) return fail(D4W_EINVAL, "bad neighbour block");
    if ((n_left || n_right) && ((long long)ns * d.up) % d.down != 0)
        return fail(D4W_EINVAL, "neighbours need ns up = %d x %d to be a multiple of down = %d: the output grids of consecutive blocks do not line up",
                    ns, d.up, d.down);
    if (d.up == 1 && d.down == 1) {
        D4W_LAUNCH(resample_copy, dim3((unsigned)std::min(ceil_div(ns, kResThreads), 64), (unsigned)std::min(nx, 65535)), dim3(kResThreads), 0, stream, x, ld_x, ns, y);
        for (int r0 = 65535; r0 < nx; r0 += 65535)
            D4W_LAUNCH(resample_copy, dim3((unsigned)std::min(ceil_div(ns, kResThreads), 64), (unsigned)std::min(nx - r0, 65535)), dim3(kResThreads), 0, stream,
                       x + (size_t)r0 * ld_x, ld_x, ns, y + (size_t)r0 * ns);
        return D4W_OK;
    }
    d.ld_x = ld_x; d.ld_left = ld_left; d.ld_right = ld_right;
    d.n_left = n_left; d.n_right = n_right;
    d.scale = scale; d.off_const = off_const; d.add_back = add_back;
    D4W_LAUNCH((resample_rows<float, false>), dim3((unsigned)((long long)nx * d.ntiles)), dim3(kResThreads), res_lds_bytes(d), stream, d, x,
               n_left ? left : nullptr, n_right ? right : nullptr, taps, ntaps, off, y);
    return D4W_OK;
}

int d4w_resample_raw_f32(const void* raw, int raw_dtype, int ns, int c0, int cstep, int nx_out, const float* taps, int ntaps,
                         int up, int down, const double* mean, double scale, float* y, void* stream) {
    if (!raw || !y || !taps || !mean || c0 < 0 || cstep < 1) return fail(D4W_EINVAL, "bad argument");
    ResDims d;
    int rc = res_dims(nx_out, ns, ntaps, up, down, &d);
    if (rc) return rc;
    if (d.up == 1 && d.down == 1) return fail(D4W_EINVAL, "up / down = 1: d4w_raw2strain_f32 converts raw rows at their own rate");
    d.ld_x = (size_t)ns; d.c0 = c0; d.cstep = cstep; d.scale = scale;
    const dim3 grid((unsigned)((long long)nx_out * d.ntiles)), block(kResThreads);
    const size_t lds = res_lds_bytes(d);
    const float* none = nullptr;
    switch (raw_dtype) {
        case 0: D4W_LAUNCH((resample_rows<int32_t, true>), grid, block, lds, stream, d, (const int32_t*)raw, none, none, taps, ntaps, mean, y); break;
        case 1: D4W_LAUNCH((resample_rows<int16_t, true>), grid, block, lds, stream, d, (const int16_t*)raw, none, none, taps, ntaps, mean, y); break;
        case 2: D4W_LAUNCH((resample_rows<float, true>), grid, block, lds, stream, d, (const float*)raw, none, none, taps, ntaps, mean, y); break;
        case 3: D4W_LAUNCH((resample_rows<double, true>), grid, block, lds, stream, d, (const double*)raw, none, none, taps, ntaps, mean, y); break;
        default: return fail(D4W_EINVAL, "raw_dtype = %d (0 int32, 1 int16, 2 float32, 3 float64)", raw_dtype);
    }
    return D4W_OK;
}

int d4w_raw_row_mean_f64(const void* raw, int raw_dtype, int ns, int c0, int cstep, int nx_out, double* mean, void* stream) {
    if (!raw || !mean || ns < 1 || nx_out < 1 || c0 < 0 || cstep < 1) return fail(D4W_EINVAL, "bad argument");
    const dim3 grid((unsigned)nx_out), block(kResThreads);
    switch (raw_dtype) {
        case 0: D4W_LAUNCH((raw_row_mean<int32_t, long long>), grid, block, 0, stream, (const int32_t*)raw, ns, c0, cstep, mean); break;
        case 1: D4W_LAUNCH((raw_row_mean<int16_t, long long>), grid, block, 0, stream, (const int16_t*)raw, ns, c0, cstep, mean); break;
        case 2: D4W_LAUNCH((raw_row_mean<float, double>), grid, block, 0, stream, (const float*)raw, ns, c0, cstep, mean); break;
        case 3: D4W_LAUNCH((raw_row_mean<double, double>), grid, block, 0, stream, (const double*)raw, ns, c0, cstep, mean); break;
        default: return fail(D4W_EINVAL, "raw_dtype = %d (0 int32, 1 int16, 2 float32, 3 float64)", raw_dtype);
    }
    return D4W_OK;
}

}  // extern "C"
