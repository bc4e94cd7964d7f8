/* ------------------------------------------------------------------------------------------
 * Analytic signal of rows too long for one workgroup's LDS (e.g. 120 000 samples): the four-step
 * time phase of the distributed plan over ALL rows (world = 1), the Hilbert pair op on the packed
 * spectrum, the inverse time phase, and one elementwise combine with x.  Same modes as
 * d4w_analytic_f32 (analytic.hip).  ws: [nx][ns] float32 scratch.
 * ------------------------------------------------------------------------------------------ */
#include <cmath>
#include <map>
#include <tuple>

#include "fk_plan.h"

namespace d4w {
// Imaginary part of the analytic signal at sample i: a plane of its own (the Hilbert transform, even ns), or the .y of the
// complex plane z (odd ns).  The real part is always the sample itself (x), not its transformed-and-back copy in z (off by
// ~1e-7 max|x|, which is the whole signal of a row that is mostly offset).
__device__ __forceinline__ float analytic_im(const float* h, size_t i) { return h[i]; }
__device__ __forceinline__ float analytic_im(const float2* z, size_t i) { return z[i].y; }

template <typename H>
__global__ __launch_bounds__(kThreads) void analytic_combine(const float* __restrict__ x, const H* __restrict__ h,
                                                              float* __restrict__ y, int ns, int mode,
                                                              const float* __restrict__ var, float fscale) {
    const size_t base = (size_t)blockIdx.y * ns;
    const int nout = (mode == 3) ? ns - 1 : ns;
    float* yr = y + (size_t)blockIdx.y * nout;
    const float inv_var = (mode == 2 || mode == 4) ? 1.0f / var[blockIdx.y] : 0.f;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nout; i += gridDim.x * blockDim.x) {
        const float re = x[base + i], im = analytic_im(h, base + i);
        float v;
        if (mode == 0) v = sqrtf(fmaf(re, re, im * im));
        else if (mode == 1) v = im;
        else if (mode == 2) v = 10.0f * log10f(fmaf(re, re, im * im) * inv_var);
        else if (mode == 4) v = sqrtf(fmaf(re, re, im * im) * inv_var);
        else {
            const float2 p = c_mulc(make_float2(x[base + i + 1], analytic_im(h, base + i + 1)), make_float2(re, im));
            v = atan2f(p.y, p.x) * fscale;
        }
        yr[i] = v;
    }
}
// Odd row lengths on the long-row path: the row as a COMPLEX sequence of its own length (no packing), the one-sided
// multiplier of scipy.signal.hilbert on its spectrum, the inverse transform = the analytic signal itself.
__global__ __launch_bounds__(kThreads) void analytic_widen(const float* __restrict__ x, float2* __restrict__ z, int ns) {
    const size_t base = (size_t)blockIdx.y * ns;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += gridDim.x * blockDim.x)
        z[base + i] = make_float2(x[base + i], 0.f);
}

// Z[row][q1][i] holds frequency k1[q1] + N1 k2[i]: x 1 at f = 0, x 2 for 0 < f <= (ns - 1) / 2, x 0 above (odd ns)
__global__ __launch_bounds__(kThreads) void analytic_onesided(float2* __restrict__ z, int ns, int N1, int N2,
                                                               const int* __restrict__ k1, const int* __restrict__ k2) {
    const size_t base = (size_t)blockIdx.y * ns;
    const int half = (ns - 1) / 2;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < ns; p += gridDim.x * blockDim.x) {
        const int q1 = p / N2, i = p - q1 * N2;
        const int f = k1[q1] + N1 * k2[i];
        const float g = (f == 0) ? 1.f : (f <= half ? 2.f : 0.f);
        z[base + p] = c_scale(z[base + p], g);
    }
}

}  // namespace d4w

using namespace d4w;

using LongKey = std::tuple<int, int, int>;      // (device, nx, ns; -ns: the complex rows of an odd length)
using LongCache = std::map<LongKey, d4w_fkd_plan*>;
static std::mutex g_long_mu;
static LongCache g_long_plans;
static LongCache g_long_fast;     // packed plans of specialised shapes (successes only)
constexpr size_t kLongPlansMax = 16;   // a stream of varying channel selections must not keep adding device tables

// drop every cached long-row plan (g_long_mu held): kernels still in flight may read their tables, so the device drains first
static void long_plans_drop_locked() {
    (void)hipDeviceSynchronize();
    for (auto& kv : g_long_plans) if (kv.second) d4w_fkd_plan_destroy(kv.second);
    for (auto& kv : g_long_fast) if (kv.second) d4w_fkd_plan_destroy(kv.second);
    g_long_plans.clear();
    g_long_fast.clear();
}

// The cached plan of `key`, or the one build(&plan) makes: found or built under g_long_mu, every cached plan dropped first
// once kLongPlansMax are held.  Only successes are remembered; a failed build leaves *out NULL and the caches as they were.
template <typename Build>
static int long_plan_get(LongCache& cache, const LongKey& key, Build build, d4w_fkd_plan** out) {
    std::lock_guard<std::mutex> lk(g_long_mu);
    *out = nullptr;
    auto it = cache.find(key);
    if (it == cache.end()) {
        d4w_fkd_plan* pl = nullptr;
        if (int rc = build(&pl)) return rc;
        if (g_long_plans.size() + g_long_fast.size() >= kLongPlansMax) long_plans_drop_locked();
        it = cache.emplace(key, pl).first;
    }
    *out = it->second;
    return D4W_OK;
}

// the packed plan of a specialised shape with the work list "sub-row q1 of a row pairs with sub-row N1 - q1 of the SAME row"
static int long_fast_build(int nx, int ns, d4w_fkd_plan** out) {
    d4w_fkd_plan* fp = nullptr;
    if (int rc = fkd_plan_build_packed(nx, ns, 1, 0, false, &fp, true)) return rc;
    const int N1 = fp->N1;
    std::vector<int2> ps;
    ps.reserve((size_t)nx * (N1 / 2 + 1));
    for (int r = 0; r < nx; ++r)
        for (int q1 = 0; q1 <= N1 / 2; ++q1)       // single-radix n1: position = frequency digit
            ps.push_back(make_int2(r * N1 + q1, r * N1 + (N1 - q1) % N1));
    void* q = nullptr;
    if (hipMalloc(&q, ps.size() * sizeof(int2)) != hipSuccess ||
        hipMemcpy(q, ps.data(), ps.size() * sizeof(int2), hipMemcpyHostToDevice) != hipSuccess) {
        if (q) (void)hipFree(q);
        d4w_fkd_plan_destroy(fp);
        return fail(D4W_ENOMEM, "hipMalloc of the self-pair list failed");
    }
    fp->sp->allocs.push_back(q);
    fp->d_pairs_self = (int2*)q;
    fp->npairs_self = (int)ps.size();
    *out = fp;
    return D4W_OK;
}

extern "C" {

/* Frees the plans d4w_analytic_long_f32 caches per (device, nx, ns) (synchronises the device).  They are also dropped
 * automatically once more than 16 shapes have been seen. */
int d4w_analytic_long_clear(void) {
    std::lock_guard<std::mutex> lk(g_long_mu);
    long_plans_drop_locked();
    return D4W_OK;
}

/* even ns: [nx][ns] float32 (the Hilbert transform); odd ns: [nx][ns] complex (the row as a complex sequence) */
size_t d4w_analytic_long_ws_bytes(int nx, int ns) {
    return (nx > 0 && ns > 0) ? (size_t)nx * ns * sizeof(float) * ((ns & 1) ? 2 : 1) : 0;
}

int d4w_analytic_long_f32(const float* x, float* y, int nx, int ns, int mode, const float* var, double fs,
                          void* ws, void* stream) {
    if (!x || !y || !ws || nx < 1 || ns < 2) return fail(D4W_EINVAL, "bad argument");
    if (mode < 0 || mode > 4) return fail(D4W_EINVAL, "mode = %d not in 0..4", mode);
    if ((mode == 2 || mode == 4) && !var) return fail(D4W_EINVAL, "modes 2 and 4 need the row variances");
    if (nx > 65535) return fail(D4W_EINVAL, "nx = %d exceeds the grid limit 65535", nx);
    int devid = 0;
    D4W_HIP(hipGetDevice(&devid));
    float* h = (float*)ws;
    if (ns & 1) {
        // odd rows: "packed rows" of 2 ns floats = complex rows of length ns through the time phase of the generic plan
        // (any length: a prime factor > 31 of ns runs the global-memory Bluestein form)
        d4w_fkd_plan* pl = nullptr;
        if (int rc = long_plan_get(g_long_plans, LongKey(devid, nx, -ns), [&](d4w_fkd_plan** out) {
                int rcb = fkd_plan_build(nx, 2 * ns, 1, 0, false, out);
                if (!rcb) (*out)->tp.dev.scale = (float)(1.0 / (double)ns);
                return rcb;
            }, &pl)) return rc;
        float2* z = reinterpret_cast<float2*>(ws);
        const dim3 grid(std::min(ceil_div(ns, kThreads), 128), nx);
        D4W_LAUNCH(analytic_widen, grid, dim3(kThreads), 0, stream, x, z, ns);
        int rc = d4w_fkd_time_fwd_f32(pl, h, h, 0, stream);
        if (rc) return rc;
        D4W_LAUNCH(analytic_onesided, grid, dim3(kThreads), 0, stream, z, ns, pl->N1, pl->N2, (const int*)pl->d_k1, (const int*)pl->d_k2);
        if ((rc = d4w_fkd_time_inv_f32(pl, h, stream))) return rc;
        D4W_LAUNCH(analytic_combine<float2>, grid, dim3(kThreads), 0, stream, x, (const float2*)z, y, ns, mode, var, (float)(fs / (2.0 * M_PI)));
        return D4W_OK;
    }
    // Shapes with specialised f-k kernels: the time phase of the packed plan (pass A MODE 1: n1 transform of the real rows),
    // pass B with the Hilbert pair operation on the self-pair work list
    // (long_fast_build), the inverse time phase in place, the combine pass -- 36 B per sample on the fast kernels instead of 52 through
    // the generic ones.  D4W_LONG_FAST=0 keeps the generic path.
    {
        static const int fast_env = [] { const char* v = getenv("D4W_LONG_FAST"); return v ? atoi(v) : 1; }();
        d4w_fkd_plan* fp = nullptr;
        // only successes are remembered: a shape registered later (d4w_fk_register_shape, fkjit) is picked up by the next
        // call; the failed attempt costs a table lookup
        if (fast_env)
            (void)long_plan_get(g_long_fast, LongKey(devid, nx, ns), [&](d4w_fkd_plan** out) { return long_fast_build(nx, ns, out); }, &fp);
        if (fp) {
            const FkFastEntry& F = *fp->sp->fast;
            const FkDims& d = fp->sp->dev.d;
            const int NBX = d.N2 / d.TA, nt = ceil_div(nx, d.C1) * NBX;
            FkGeo geo = fp->geo_t;
            geo.nrows = nx;
            FkDev dv = fp->dev_t;
            dv.scale = (float)(1.0 / (double)d.M);               // forward / inverse pair of the packed rows
            dv.mask = nullptr;
            dv.nyq = nullptr;
            float2* h2 = reinterpret_cast<float2*>(h);
            const dim3 gA(std::min(nt, fp->num_cu * fp->sp->wgA));
            int rc = launch_k(F.T_fwd, gA, dim3(F.thrA), F.ldsA, stream, fp->dev_t, reinterpret_cast<const float2*>(x), h2, 0, nt, NBX, 0, geo);
            if (rc) return rc;
            FkFastDev fd = fp->fdev_c;
            fd.pairs = fp->d_pairs_self;
            fd.live = nullptr;
            FkGeo gb = fp->geo_c;
            gb.nq = d.N1;
            const dim3 gB(std::max(1, std::min(fp->npairs_self, fp->num_cu * fp->sp->wgB)));
            if ((rc = launch_k(F.Bs_hilb, gB, dim3(F.thrB), F.ldsB, stream, dv, fd, h2, 0, fp->npairs_self, gb))) return rc;
            static const int fuse_env = [] { const char* v = getenv("D4W_LONG_FUSE"); return v ? atoi(v) : 1; }();
            if (mode == 1)                                         // H[x] itself: the inverse pass writes it where it belongs
                return launch_k(F.T_inv, gA, dim3(F.thrA), F.ldsA, stream, dv, reinterpret_cast<float2*>(y), 0, nt, NBX, 0, geo, (const float2*)h2);
            if (mode != 3 && fuse_env)                             // |z|, SNR, |z| / std: formed in the inverse pass's epilogue (28 B / sample)
                return launch_k(F.T_inv_env, gA, dim3(F.thrA), F.ldsA, stream, dv, reinterpret_cast<float2*>(y), 0, nt, NBX, 0, geo,
                                (const float2*)h2, reinterpret_cast<const float2*>(x), mode, var);
            if ((rc = launch_k(F.T_inv, gA, dim3(F.thrA), F.ldsA, stream, dv, h2, 0, nt, NBX, 0, geo, (const float2*)h2))) return rc;
            const float fscale = (float)(fs / (2.0 * M_PI));
            D4W_LAUNCH(analytic_combine<float>, dim3(std::min(ceil_div(ns, kThreads), 128), nx), dim3(kThreads), 0, stream, x,
                       (const float*)h, y, ns, mode, var, fscale);
            return D4W_OK;
        }
    }
    d4w_fkd_plan* pl = nullptr;
    if (int rc = long_plan_get(g_long_plans, LongKey(devid, nx, ns), [&](d4w_fkd_plan** out) {
            int rcb = fkd_plan_build(nx, ns, 1, 0, false, out);
            if (!rcb) {
                (*out)->slab.hilbert = 1;
                (*out)->tp.dev.scale = (float)(1.0 / (double)(*out)->M);     // forward / inverse pair of the packed rows
            }
            return rcb;
        }, &pl)) return rc;
    int rc = d4w_fkd_time_fwd_f32(pl, x, h, 0, stream);
    if (rc) return rc;
    if ((rc = fkd_launch_pair_slab(pl->slab, reinterpret_cast<float2*>(h), stream))) return rc;
    if ((rc = d4w_fkd_time_inv_f32(pl, h, stream))) return rc;
    const float fscale = (float)(fs / (2.0 * M_PI));
    D4W_LAUNCH(analytic_combine<float>, dim3(std::min(ceil_div(ns, kThreads), 128), nx), dim3(kThreads), 0, stream, x,
               (const float*)h, y, ns, mode, var, fscale);
    return D4W_OK;
}

}  // extern "C"
