// Radon transform on MI355X (gfx950) -- improcess.compute_radon_transform (improcess.py:347-367), which is
// skimage.transform.radon(image, theta, circle=False):
//
//   P = ceil(sqrt(2) max(h, w)); the image is zero-padded to P x P with pad_before[d] = (s_d + P - s_d) / 2 - s_d / 2,
//   c0 = P / 2, and for every angle a = deg2rad(theta[i]) and output pixel (r, c) of the P x P grid
//       x = cos a c + sin a r - c0 (cos a + sin a - 1)      (padded column)
//       y = -sin a c + cos a r - c0 (cos a - sin a - 1)     (padded row)
//   is sampled bilinearly (floor / ceil neighbours, 0 outside); out[c][i] = sum_r sample(r, c).
//
// Form: one thread per (ray c, angle i), neighbouring lanes = neighbouring rays of one angle.  Each thread walks r over
// the range where its ray meets the image plus one pixel of bilinear support (found analytically, widened by one step
// on either side; the per-neighbour bounds checks inside the loop decide what is read, so the clip only skips zeros).
// The padded P x P square is never built: the unpadded image is read with the pad_before offsets.
//
// Precision: the sample point is formed in float64 from the ray's start, x = X0 + r sin a, y = Y0 + r cos a (two FMAs per
// sample; gfx950 runs float64 FMA at half the float32 rate and the loop is bound by its four gathers).  A float32 point
// of magnitude ~P loses the interpolation weights' low bits (2.6-8.6e-6 of max|sinogram| at 1102 x 1200 in a model of that
// form); float64 points keep them, and only the weights (float32 from the float64 fraction), the bilinear blend (float32)
// and the pixels are float32.  The ray sum is accumulated in float64 and rounded once.  cos / sin come from the host in
// float64 (the reference's np.cos / np.sin of np.deg2rad), in the workspace.  Every output element is written by exactly
// one thread in a fixed order: run-to-run bit-identical.
#include <algorithm>
#include <cmath>

#include "d4w_internal.h"

namespace d4w {

constexpr int kRadonThreads = 256;

// r range (inclusive, within [0, P - 1]) over which lo < x0 + r * s < hi can hold, widened by one step on either side
__device__ __forceinline__ void radon_clip(double x0, double s, double lo, double hi, double& rlo, double& rhi) {
    if (fabs(s) < 1e-12) {
        if (!(x0 > lo - 1.0 && x0 < hi + 1.0)) { rlo = 1.0; rhi = 0.0; }   // never within reach: empty
        return;
    }
    double a = (lo - x0) / s, b = (hi - x0) / s;
    if (a > b) { const double t = a; a = b; b = t; }
    rlo = fmax(rlo, floor(a) - 1.0);
    rhi = fmin(rhi, ceil(b) + 1.0);
}

__device__ __forceinline__ float radon_px(const float* __restrict__ img, int h, int w, int iy, int ix) {
    return ((unsigned)iy < (unsigned)h && (unsigned)ix < (unsigned)w) ? img[iy * w + ix] : 0.0f;
}

// grid (ceil(P / 256), min(ntheta, 65535)); cs = DEVICE [ntheta][2] {cos, sin} per angle
__global__ __launch_bounds__(kRadonThreads) void radon_rays(const float* __restrict__ img, int h, int w, int P, int pb0,
                                                             int pb1, const double* __restrict__ cs, int ntheta,
                                                             float* __restrict__ out) {
    const int c = blockIdx.x * kRadonThreads + threadIdx.x;
    if (c >= P) return;
    const double c0 = (double)(P / 2);
    for (int i = blockIdx.y; i < ntheta; i += gridDim.y) {
        const double ca = cs[2 * i], sa = cs[2 * i + 1];
        // image coordinates of the sample at step r: X = X0 + r sa (column), Y = Y0 + r ca (row)
        const double X0 = ca * (double)c - c0 * (ca + sa - 1.0) - (double)pb1;
        const double Y0 = -sa * (double)c - c0 * (ca - sa - 1.0) - (double)pb0;
        // a sample reads a pixel only where -1 < X < w and -1 < Y < h
        double rlo = 0.0, rhi = (double)(P - 1);
        radon_clip(X0, sa, -1.0, (double)w, rlo, rhi);
        radon_clip(Y0, ca, -1.0, (double)h, rlo, rhi);
        const int r0 = (int)fmin(rlo, (double)P), r1 = (int)fmax(rhi, -1.0);
        double acc = 0.0;
        for (int r = r0; r <= r1; ++r) {
            const double X = fma((double)r, sa, X0), Y = fma((double)r, ca, Y0);
            const double fx = floor(X), fy = floor(Y);
            const int ix0 = (int)fx, iy0 = (int)fy, ix1 = (int)ceil(X), iy1 = (int)ceil(Y);
            const float dx = (float)(X - fx), dy = (float)(Y - fy);
            const float tl = radon_px(img, h, w, iy0, ix0), tr = radon_px(img, h, w, iy0, ix1);
            const float bl = radon_px(img, h, w, iy1, ix0), br = radon_px(img, h, w, iy1, ix1);
            const float top = (1.0f - dx) * tl + dx * tr, bot = (1.0f - dx) * bl + dx * br;
            acc += (double)((1.0f - dy) * top + dy * bot);
        }
        out[(size_t)c * ntheta + i] = (float)acc;
    }
}

static bool radon_dims_ok(int h, int w) {
    return h >= 1 && w >= 1 && h <= (1 << 24) && w <= (1 << 24) && (int64_t)h * w <= (int64_t)INT32_MAX;
}

static int radon_size(int h, int w) { return (int)std::ceil(std::sqrt(2.0) * (double)std::max(h, w)); }

}  // namespace d4w

using namespace d4w;

extern "C" {

int d4w_radon_size(int h, int w) {
    if (!radon_dims_ok(h, w)) return fail(D4W_EINVAL, "radon: image %d x %d is empty or too large", h, w);
    return radon_size(h, w);
}

size_t d4w_radon_ws_bytes(int h, int w, int ntheta) {
    if (!radon_dims_ok(h, w) || ntheta < 1) return 0;
    return ((size_t)ntheta * 2 * sizeof(double) + 255) & ~(size_t)255;
}

int d4w_radon_f32(const float* img, int h, int w, const double* theta_deg, int ntheta, float* out, void* ws, void* stream) {
    if (!radon_dims_ok(h, w)) return fail(D4W_EINVAL, "radon: image %d x %d is empty or too large", h, w);
    if (!img || !out || ntheta < 0) return fail(D4W_EINVAL, "bad argument");
    if (ntheta == 0) return D4W_OK;                              // (P, 0): nothing to write
    if (!theta_deg || !ws) return fail(D4W_EINVAL, "bad argument");
    const int P = radon_size(h, w);
    if ((int64_t)P * ntheta > (int64_t)INT32_MAX) return fail(D4W_EINVAL, "radon: output %d x %d is too large", P, ntheta);
    // cos / sin in float64 as numpy computes them: np.deg2rad(theta) = theta * (pi / 180)
    std::vector<double> cs((size_t)ntheta * 2);
    for (int i = 0; i < ntheta; ++i) {
        if (!std::isfinite(theta_deg[i])) return fail(D4W_EINVAL, "radon: theta[%d] is not finite", i);
        const double a = theta_deg[i] * (M_PI / 180.0);
        cs[2 * (size_t)i] = std::cos(a);
        cs[2 * (size_t)i + 1] = std::sin(a);
    }
    // (pageable source: the runtime has taken the bytes when the call returns)
    D4W_HIP(hipMemcpyAsync(ws, cs.data(), cs.size() * sizeof(double), hipMemcpyHostToDevice, (hipStream_t)stream));
    const int pb0 = P / 2 - h / 2, pb1 = P / 2 - w / 2;         // (s + pad) // 2 - s // 2 with s + pad = P
    const dim3 grid((P + kRadonThreads - 1) / kRadonThreads, std::min(ntheta, 65535));
    D4W_LAUNCH(radon_rays, grid, dim3(kRadonThreads), 0, stream, img, h, w, P, pb0, pb1, (const double*)ws, ntheta, out);
    return D4W_OK;
}

}  // extern "C"
