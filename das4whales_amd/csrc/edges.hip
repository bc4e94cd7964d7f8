// Edge stencils, Gaussian blur and bilateral filter on MI355X (gfx950) -- the image operators of the reference's
// improcess.py that the Gabor detector does not use:
//
//   gradient_oriented        improcess.py:143-169   three-point oriented difference (slices)
//   detect_diagonal_edges    improcess.py:172-226   two 5 x 5 kernels, scipy.signal.fftconvolve(mode='same'), summed
//   diagonal_edge_detection  improcess.py:229-266   two 3 x 3 kernels, torch conv2d(padding=1), summed
//   gaussian_filter          improcess.py:370-392   cv2.GaussianBlur(img, (size, size), sigma)
//   bilateral_filter         improcess.py:319-344   cv2.bilateralFilter(img, d, sigma_color, sigma_space)
//
// All kernels: float32 [h][w] row-major in and out, every output element written by exactly one thread in a fixed
// summation order (run-to-run bit-identical), no atomics.
//
// stencil_zero_tile: correlation with a host-supplied kernel of at most 7 x 7, ZEROS outside the image (what
//   fftconvolve 'same' and conv2d's padding do; d4w_filter2d_f32 reflects instead).  The kernel arrives zero-padded to 7 x 7 as a
//   kernel argument (49 SGPRs), so the tap loops are compile-time: 49 FMAs per pixel whatever the kernel's size, which at
//   the file shape is still below the time of the HBM pass.  A 64 x 32 output tile is staged in LDS with its 6-pixel halo (one
//   HBM read per pixel, the halo re-reads hit L2); a thread owns 8 consecutive rows of one column and walks down the column
//   once per kernel column, so one LDS read feeds up to 7 FMAs (14 reads per 8 x 7 taps).  LDS, not a register sliding
//   window across lanes: the window in x would need cross-lane moves per tap, the LDS column walk needs none.
// gradient_oriented: two or three reads per output of a cropped window; one thread per output element.
// gauss_tile: separable blur, BORDER_REFLECT_101, rows then columns in ONE launch through LDS for taps of <= 31: the
//   (32 + ky - 1) x (64 + kx - 1) input patch, then the row-filtered (32 + ky - 1) x 64 patch, then the column pass writes
//   the 32 x 64 tile.  Larger kernels: gauss_axis twice through a workspace image (one thread per pixel, taps in the workspace).
// bilateral_tile: out = I(p) + sum_q w (I(q) - I(p)) / sum_q w, w = space_w[q - p] exp(-(I(q) - I(p))^2 / (2 sigma_color^2)),
//   the same value as sum w I(q) / sum w but with float32 rounding relative to the local contrast instead of the pixel level
//   (a constant image comes back exactly).  space_w is the host's table over the (2 r + 1)^2 square, 0 outside the circle;
//   zero entries are skipped (wave-uniform branch).  64 x 16 tile + r-pixel halo in LDS for r <= 15, reflect-101; larger
//   radii read global memory directly (bilateral_direct).  The range weight uses the hardware exp2 (__expf): its relative
//   error, ~1e-7 (1 + |argument|), is far inside the 1e-5 bar because large arguments are negligible weights.
#include <algorithm>

#include "d4w_internal.h"

namespace d4w {

constexpr int kEdThreads = 256;
constexpr int kStMax = 7;                        // largest stencil
constexpr int kStTileW = 64, kStTileH = 32, kStRows = 8;
constexpr int kStPW = kStTileW + kStMax - 1, kStPH = kStTileH + kStMax - 1;
constexpr int kGsMax = 31;                       // largest fused Gaussian
constexpr int kGsTileW = 64, kGsTileH = 32, kGsRows = 8;
constexpr int kBlMaxR = 15;                      // largest tiled bilateral radius
constexpr int kBlTileW = 64, kBlTileH = 16, kBlRows = 4;

struct StencilTaps { float k[kStMax * kStMax]; };            // [7][7], zero-padded below and to the right
struct GaussTaps { float y[kGsMax]; float x[kGsMax]; };

__device__ __forceinline__ int ed_reflect101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = (i < 0) ? -i : 2 * (n - 1) - i;
    return i;
}

// out[y][x] = sum_ij K[i][j] img[y + i - ay][x + j - ax], zeros outside.  grid (ceil(w / 64), ceil(h / 32))
__global__ __launch_bounds__(kEdThreads) void stencil_zero_tile(const float* __restrict__ img, int h, int w, StencilTaps taps,
                                                                int ay, int ax, float* __restrict__ out) {
    __shared__ float tile[kStPH * kStPW];
    const int x0 = blockIdx.x * kStTileW - ax, y0 = blockIdx.y * kStTileH - ay;
    for (int e = threadIdx.x; e < kStPH * kStPW; e += kEdThreads) {
        const int gy = y0 + e / kStPW, gx = x0 + e % kStPW;
        tile[e] = ((unsigned)gy < (unsigned)h && (unsigned)gx < (unsigned)w) ? img[(size_t)gy * w + gx] : 0.f;
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, ty = (threadIdx.x >> 6) * kStRows;
    float acc[kStRows];
#pragma unroll
    for (int r = 0; r < kStRows; ++r) acc[r] = 0.f;
#pragma unroll
    for (int j = 0; j < kStMax; ++j) {
#pragma unroll
        for (int rr = 0; rr < kStRows + kStMax - 1; ++rr) {
            const float v = tile[(ty + rr) * kStPW + tx + j];
#pragma unroll
            for (int r = 0; r < kStRows; ++r)
                if (rr - r >= 0 && rr - r < kStMax) acc[r] = fmaf(taps.k[(rr - r) * kStMax + j], v, acc[r]);
        }
    }
    const int ox = blockIdx.x * kStTileW + tx;
    if (ox >= w) return;
#pragma unroll
    for (int r = 0; r < kStRows; ++r) {
        const int oy = blockIdx.y * kStTileH + ty + r;
        if (oy < h) out[(size_t)oy * w + ox] = acc[r];
    }
}

// mode 0 (dfx = 0): out[y][x] = -(img[y][x] - img[y][x + dft])                                            [h][w - dft]
// mode 1 (dft = 0): out[y][x] = -(img[y + dfx][x] - img[y][x])                                            [h - dfx][w]
// mode 2:           out[y][x] = -(img[y + dfx][x] - 0.5 img[y + 2 dfx][x + dft] - 0.5 img[y][x + dft])    [h - 2 dfx][w - dft]
// grid (ceil(ow / 256), min(oh, 65535))
__global__ __launch_bounds__(kEdThreads) void gradient_oriented(const float* __restrict__ img, int w, int mode, int dft, int dfx,
                                                                float* __restrict__ out, int oh, int ow) {
    const int x = blockIdx.x * kEdThreads + threadIdx.x;
    if (x >= ow) return;
    for (int y = blockIdx.y; y < oh; y += gridDim.y) {
        const float* p = img + (size_t)y * w + x;
        float g;
        if (mode == 0) g = -(p[0] - p[dft]);
        else if (mode == 1) g = -(p[(size_t)dfx * w] - p[0]);
        else g = -(p[(size_t)dfx * w] - 0.5f * p[(size_t)2 * dfx * w + dft] - 0.5f * p[dft]);
        out[(size_t)y * ow + x] = g;
    }
}

// rows then columns through LDS, ky, kx <= 31.  grid (ceil(w / 64), ceil(h / 32)); LDS (ph pw + ph 64) floats
__global__ __launch_bounds__(kEdThreads) void gauss_tile(const float* __restrict__ img, int h, int w, GaussTaps taps, int ky, int kx,
                                                         float* __restrict__ out) {
    D4W_DYN_LDS(smem_raw);
    const int pw = kGsTileW + kx - 1, ph = kGsTileH + ky - 1;
    float* in = reinterpret_cast<float*>(smem_raw);
    float* mid = in + ph * pw;
    const int x0 = blockIdx.x * kGsTileW - kx / 2, y0 = blockIdx.y * kGsTileH - ky / 2;
    for (int e = threadIdx.x; e < ph * pw; e += kEdThreads) {
        const int ty = e / pw, tx = e % pw;
        in[e] = img[(size_t)ed_reflect101(y0 + ty, h) * w + ed_reflect101(x0 + tx, w)];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < ph * kGsTileW; e += kEdThreads) {
        const float* p = in + (e >> 6) * pw + (e & 63);
        float s = 0.f;
        for (int t = 0; t < kx; ++t) s = fmaf(taps.x[t], p[t], s);
        mid[e] = s;
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, ty = (threadIdx.x >> 6) * kGsRows;
    const int ox = blockIdx.x * kGsTileW + tx;
    if (ox >= w) return;
    for (int r = 0; r < kGsRows; ++r) {
        const int oy = blockIdx.y * kGsTileH + ty + r;
        if (oy >= h) break;
        const float* p = mid + (ty + r) * kGsTileW + tx;
        float s = 0.f;
        for (int t = 0; t < ky; ++t) s = fmaf(taps.y[t], p[t * kGsTileW], s);
        out[(size_t)oy * w + ox] = s;
    }
}

// one axis of the blur for kernels beyond the fused form: out[y][x] = sum_t taps[t] img[..reflect101(. + t - k / 2)..]
// grid (ceil(w / 256), min(h, 65535)); taps = DEVICE [k]
__global__ __launch_bounds__(kEdThreads) void gauss_axis(const float* __restrict__ img, int h, int w, const float* __restrict__ taps,
                                                         int k, int vertical, float* __restrict__ out) {
    const int x = blockIdx.x * kEdThreads + threadIdx.x;
    if (x >= w) return;
    for (int y = blockIdx.y; y < h; y += gridDim.y) {
        float s = 0.f;
        if (vertical)
            for (int t = 0; t < k; ++t) s = fmaf(taps[t], img[(size_t)ed_reflect101(y + t - k / 2, h) * w + x], s);
        else
            for (int t = 0; t < k; ++t) s = fmaf(taps[t], img[(size_t)y * w + ed_reflect101(x + t - k / 2, w)], s);
        out[(size_t)y * w + x] = s;
    }
}

// space_w = DEVICE [(2 r + 1)^2], 0 outside the circle; gc = -1 / (2 sigma_color^2).  grid (ceil(w / 64), ceil(h / 16));
// LDS (16 + 2 r)(64 + 2 r) floats
__global__ __launch_bounds__(kEdThreads) void bilateral_tile(const float* __restrict__ img, int h, int w, int r,
                                                             const float* __restrict__ space_w, float gc, float* __restrict__ out) {
    D4W_DYN_LDS(smem_raw);
    float* tile = reinterpret_cast<float*>(smem_raw);
    const int pw = kBlTileW + 2 * r, ph = kBlTileH + 2 * r, d = 2 * r + 1;
    const int x0 = blockIdx.x * kBlTileW - r, y0 = blockIdx.y * kBlTileH - r;
    for (int e = threadIdx.x; e < ph * pw; e += kEdThreads) {
        const int ty = e / pw, tx = e % pw;
        tile[e] = img[(size_t)ed_reflect101(y0 + ty, h) * w + ed_reflect101(x0 + tx, w)];
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, ty = (threadIdx.x >> 6) * kBlRows;
    const float* base = tile + ty * pw + tx;              // tap (dy, dx) of row q: base[(q + dy + r) pw + dx + r]
    float ctr[kBlRows], num[kBlRows], den[kBlRows];
#pragma unroll
    for (int q = 0; q < kBlRows; ++q) {
        ctr[q] = base[(q + r) * pw + r];
        num[q] = 0.f;
        den[q] = 0.f;
    }
    for (int i = 0; i < d; ++i) {
        for (int j = 0; j < d; ++j) {
            const float sw = space_w[i * d + j];
            if (sw == 0.f) continue;
#pragma unroll
            for (int q = 0; q < kBlRows; ++q) {
                const float dv = base[(q + i) * pw + j] - ctr[q];
                const float wt = sw * d4w_expf(dv * dv * gc);
                num[q] = fmaf(wt, dv, num[q]);
                den[q] += wt;
            }
        }
    }
    const int ox = blockIdx.x * kBlTileW + tx;
    if (ox >= w) return;
#pragma unroll
    for (int q = 0; q < kBlRows; ++q) {
        const int oy = blockIdx.y * kBlTileH + ty + q;
        if (oy < h) out[(size_t)oy * w + ox] = ctr[q] + num[q] / den[q];
    }
}

// the same sum straight from global memory, any radius.  grid (ceil(w / 256), min(h, 65535))
__global__ __launch_bounds__(kEdThreads) void bilateral_direct(const float* __restrict__ img, int h, int w, int r,
                                                               const float* __restrict__ space_w, float gc, float* __restrict__ out) {
    const int x = blockIdx.x * kEdThreads + threadIdx.x;
    if (x >= w) return;
    const int d = 2 * r + 1;
    for (int y = blockIdx.y; y < h; y += gridDim.y) {
        const float ctr = img[(size_t)y * w + x];
        float num = 0.f, den = 0.f;
        for (int i = 0; i < d; ++i) {
            const float* row = img + (size_t)ed_reflect101(y + i - r, h) * w;
            for (int j = 0; j < d; ++j) {
                const float sw = space_w[i * d + j];
                if (sw == 0.f) continue;
                const float dv = row[ed_reflect101(x + j - r, w)] - ctr;
                const float wt = sw * d4w_expf(dv * dv * gc);
                num = fmaf(wt, dv, num);
                den += wt;
            }
        }
        out[(size_t)y * w + x] = ctr + num / den;
    }
}

static bool ed_dims_ok(int h, int w) { return h >= 1 && w >= 1 && (int64_t)h * w <= (int64_t)INT32_MAX; }

static bool ed_taps_ok(const double* t, int k) {
    if (!t || k < 1 || !(k & 1)) return false;
    for (int i = 0; i < k; ++i)
        if (!std::isfinite(t[i])) return false;
    return true;
}

static size_t ed_align(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_stencil_zero_f32(const float* img, int h, int w, const double* kernel, int kh, int kw, int anchor_y, int anchor_x,
                         float* out, void* stream) {
    if (!img || !out || !kernel || img == out) return fail(D4W_EINVAL, "bad argument");
    if (!ed_dims_ok(h, w)) return fail(D4W_EINVAL, "stencil: image %d x %d is empty or too large", h, w);
    if (kh < 1 || kw < 1 || kh > kStMax || kw > kStMax)
        return fail(D4W_EINVAL, "stencil: kernel %d x %d is not within 1 x 1 .. %d x %d", kh, kw, kStMax, kStMax);
    if (anchor_y < 0 || anchor_y >= kh || anchor_x < 0 || anchor_x >= kw)
        return fail(D4W_EINVAL, "stencil: anchor (%d, %d) lies outside the %d x %d kernel", anchor_y, anchor_x, kh, kw);
    const dim3 grid(ceil_div(w, kStTileW), ceil_div(h, kStTileH));
    if (grid.y > 65535) return fail(D4W_EINVAL, "stencil: image height %d exceeds the grid limit", h);
    StencilTaps taps;
    for (int i = 0; i < kStMax; ++i)
        for (int j = 0; j < kStMax; ++j) {
            const double v = (i < kh && j < kw) ? kernel[i * kw + j] : 0.0;
            if (!std::isfinite(v)) return fail(D4W_EINVAL, "stencil: kernel[%d][%d] is not finite", i, j);
            taps.k[i * kStMax + j] = (float)v;
        }
    D4W_LAUNCH(stencil_zero_tile, grid, dim3(kEdThreads), 0, stream, img, h, w, taps, anchor_y, anchor_x, out);
    return D4W_OK;
}

int d4w_gradient_oriented_f32(const float* img, int h, int w, int dft, int dfx, float* out, void* stream) {
    if (!img || img == out) return fail(D4W_EINVAL, "bad argument");
    if (!ed_dims_ok(h, w)) return fail(D4W_EINVAL, "gradient_oriented: image %d x %d is empty or too large", h, w);
    if (dft < 0 || dfx < 0) return fail(D4W_EINVAL, "gradient_oriented: direction (%d, %d) must be non-negative", dft, dfx);
    const int mode = dfx == 0 ? 0 : dft == 0 ? 1 : 2;
    const int64_t oh = mode == 0 ? h : mode == 1 ? (int64_t)h - dfx : (int64_t)h - 2 * (int64_t)dfx;
    const int64_t ow = (dft == 0 && mode == 0) ? 0 : (int64_t)w - dft;         // (0, 0): the reference's empty [h, 0]
    if (oh <= 0 || ow <= 0) return D4W_OK;                                      // nothing to write
    if (!out) return fail(D4W_EINVAL, "bad argument");
    const dim3 grid(ceil_div((int)ow, kEdThreads), (unsigned)std::min<int64_t>(oh, 65535));
    D4W_LAUNCH(gradient_oriented, grid, dim3(kEdThreads), 0, stream, img, w, mode, dft, dfx, out, (int)oh, (int)ow);
    return D4W_OK;
}

size_t d4w_gaussian_blur_ws_bytes(int h, int w, int ky, int kx) {
    if (!ed_dims_ok(h, w) || ky < 1 || kx < 1) return 0;
    if (ky <= kGsMax && kx <= kGsMax) return 0;
    return ed_align((size_t)ky * sizeof(float)) + ed_align((size_t)kx * sizeof(float)) + (size_t)h * w * sizeof(float);
}

int d4w_gaussian_blur_f32(const float* img, int h, int w, const double* taps_y, const double* taps_x, int ky, int kx, float* out,
                          void* ws, void* stream) {
    if (!img || !out || img == out) return fail(D4W_EINVAL, "bad argument");
    if (!ed_dims_ok(h, w)) return fail(D4W_EINVAL, "gaussian_blur: image %d x %d is empty or too large", h, w);
    if (!ed_taps_ok(taps_y, ky) || !ed_taps_ok(taps_x, kx))
        return fail(D4W_EINVAL, "gaussian_blur: taps must be finite and of odd length (%d, %d)", ky, kx);
    if (ky > (1 << 20) || kx > (1 << 20)) return fail(D4W_EINVAL, "gaussian_blur: kernel %d x %d is too large", ky, kx);
    if (ky <= kGsMax && kx <= kGsMax) {
        GaussTaps taps;
        for (int t = 0; t < kGsMax; ++t) {
            taps.y[t] = t < ky ? (float)taps_y[t] : 0.f;
            taps.x[t] = t < kx ? (float)taps_x[t] : 0.f;
        }
        const dim3 grid(ceil_div(w, kGsTileW), ceil_div(h, kGsTileH));
        if (grid.y > 65535) return fail(D4W_EINVAL, "gaussian_blur: image height %d exceeds the grid limit", h);
        const size_t lds = (size_t)(kGsTileH + ky - 1) * (kGsTileW + kx - 1 + kGsTileW) * sizeof(float);
        D4W_LAUNCH(gauss_tile, grid, dim3(kEdThreads), lds, stream, img, h, w, taps, ky, kx, out);
        return D4W_OK;
    }
    if (!ws) return fail(D4W_EINVAL, "gaussian_blur: kernel %d x %d needs the workspace", ky, kx);
    std::vector<float> ty(taps_y, taps_y + ky), tx(taps_x, taps_x + kx);
    float* dty = (float*)ws;
    float* dtx = (float*)((char*)ws + ed_align((size_t)ky * sizeof(float)));
    float* mid = (float*)((char*)dtx + ed_align((size_t)kx * sizeof(float)));
    // (pageable sources: the runtime has taken the bytes when the calls return)
    D4W_HIP(hipMemcpyAsync(dty, ty.data(), (size_t)ky * sizeof(float), hipMemcpyHostToDevice, (hipStream_t)stream));
    D4W_HIP(hipMemcpyAsync(dtx, tx.data(), (size_t)kx * sizeof(float), hipMemcpyHostToDevice, (hipStream_t)stream));
    const dim3 grid(ceil_div(w, kEdThreads), std::min(h, 65535));
    D4W_LAUNCH(gauss_axis, grid, dim3(kEdThreads), 0, stream, img, h, w, (const float*)dtx, kx, 0, mid);
    D4W_LAUNCH(gauss_axis, grid, dim3(kEdThreads), 0, stream, (const float*)mid, h, w, (const float*)dty, ky, 1, out);
    return D4W_OK;
}

int d4w_bilateral_max_tiled_radius(void) { return kBlMaxR; }

int d4w_bilateral_f32(const float* img, int h, int w, int radius, const float* space_w, double sigma_color, float* out,
                      void* stream) {
    if (!img || !out || !space_w || img == out) return fail(D4W_EINVAL, "bad argument");
    if (!ed_dims_ok(h, w)) return fail(D4W_EINVAL, "bilateral: image %d x %d is empty or too large", h, w);
    if (radius < 0 || radius > 1024) return fail(D4W_EINVAL, "bilateral: radius %d is not within 0 .. 1024", radius);
    if (!(sigma_color > 0.0) || !std::isfinite(sigma_color)) return fail(D4W_EINVAL, "bilateral: sigma_color must be positive");
    // (finite: the centre tap evaluates 0 * gc)
    const float gc = (float)std::max(-0.5 / (sigma_color * sigma_color), -3.0e38);
    if (radius <= kBlMaxR) {
        const dim3 grid(ceil_div(w, kBlTileW), ceil_div(h, kBlTileH));
        if (grid.y > 65535) return fail(D4W_EINVAL, "bilateral: image height %d exceeds the grid limit", h);
        const size_t lds = (size_t)(kBlTileH + 2 * radius) * (kBlTileW + 2 * radius) * sizeof(float);
        D4W_LAUNCH(bilateral_tile, grid, dim3(kEdThreads), lds, stream, img, h, w, radius, space_w, gc, out);
        return D4W_OK;
    }
    const dim3 grid(ceil_div(w, kEdThreads), std::min(h, 65535));
    D4W_LAUNCH(bilateral_direct, grid, dim3(kEdThreads), 0, stream, img, h, w, radius, space_w, gc, out);
    return D4W_OK;
}

}  // extern "C"
