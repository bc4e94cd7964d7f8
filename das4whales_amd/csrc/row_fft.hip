// The one cache of row-transform plans (row_fft.h): per-(device, length) tables, kept for the life of the process.
#include <map>
#include <mutex>

#include "row_fft.h"

namespace d4w {

static std::mutex g_rowfft_mu;
static std::map<std::pair<int, int>, RowFftHost*> g_rowfft;

template <typename T>
static int sp_upload(RowFftHost* h, const std::vector<T>& v, const T** out) {
    void* p = nullptr;
    D4W_HIP(hipMalloc(&p, std::max<size_t>(v.size(), 1) * sizeof(T)));
    h->allocs.push_back(p);
    D4W_HIP(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = (const T*)p;
    return D4W_OK;
}

int row_fft_tile_elems(int L) {
    std::vector<int> rad;
    return factor_radices(L, rad) ? L : smooth_len_235(2L * L - 1);
}

int row_fft_get(int L, const RowFftHost** out) {
    int devid = 0;
    D4W_HIP(hipGetDevice(&devid));
    std::lock_guard<std::mutex> lk(g_rowfft_mu);
    auto it = g_rowfft.find({devid, L});
    if (it != g_rowfft.end()) { *out = it->second; return D4W_OK; }
    std::vector<int> rad;
    const bool bluestein = !factor_radices(L, rad);
    int bs_L = 0;
    if (bluestein) {
        bs_L = row_fft_tile_elems(L);
        if (row_tile_bytes(bs_L) > kSpLdsMax)
            return fail(D4W_EINVAL, "transform length %d has a prime factor > 31 and is too long for the Bluestein form "
                        "(dsp.supported_length(n) gives the nearest shorter length with a direct kernel)", L);
        rad.clear();
    }
    RowFftHost* h = new RowFftHost();
    memset(&h->dev, 0, sizeof(h->dev));
    AxisDesc& ax = h->dev.ax;
    ax.L = L;
    ax.nstage = (L == 1) ? 0 : (int)rad.size();
    for (int i = 0; i < kMaxStages; ++i) ax.radix[i] = (i < (int)rad.size() && L > 1) ? rad[i] : 1;
    if (L == 1) rad.clear();
    std::vector<int> p2f = pos_to_freq(L, rad);
    if (bluestein)
        for (int i = 0; i < L; ++i) p2f[i] = i;                   // natural order
    std::vector<int> pos(L);
    for (int p = 0; p < L; ++p) pos[p2f[p]] = p;
    std::vector<float2> wp(L);
    for (int f = 0; f < L; ++f) wp[f] = wexp(f, 2LL * L);
    std::vector<float> hann(L);
    h->sumw2 = 0.0;
    for (int n = 0; n < L; ++n) {
        const double w = 0.5 - 0.5 * cos(2.0 * M_PI * (double)n / (double)L);
        hann[n] = (float)w;
        h->sumw2 += w * w;
    }
    int rc = sp_upload(h, twiddle_table2(L, &ax.nhi), &ax.tw2);
    if (!rc && bluestein) {
        std::vector<int> radL;
        factor_radices(bs_L, radL);
        AxisDesc& ab = h->dev.ax_bs;
        ab.L = bs_L;
        ab.nstage = (int)radL.size();
        for (int i = 0; i < kMaxStages; ++i) ab.radix[i] = (i < (int)radL.size()) ? radL[i] : 1;
        const std::vector<int> fL = pos_to_freq(bs_L, radL);
        std::vector<float2> chirp(L), filt(bs_L);
        std::vector<double> bre(bs_L, 0.0), bim(bs_L, 0.0);
        for (int n = 0; n < L; ++n) {
            const double ph = M_PI * (double)(((long long)n * n) % (2LL * L)) / (double)L;
            chirp[n] = make_float2((float)cos(ph), (float)-sin(ph));
            bre[n] = cos(ph); bim[n] = sin(ph);
            if (n) { bre[bs_L - n] = cos(ph); bim[bs_L - n] = sin(ph); }
        }
        host_dft_any(bre, bim);
        for (int q = 0; q < bs_L; ++q) filt[q] = make_float2((float)(bre[fL[q]] / bs_L), (float)(bim[fL[q]] / bs_L));
        rc = sp_upload(h, twiddle_table2(bs_L, &ab.nhi), &ab.tw2);
        if (!rc) rc = sp_upload(h, chirp, &h->dev.bs_chirp);
        if (!rc) rc = sp_upload(h, filt, &h->dev.bs_filt);
        h->dev.bs_L = bs_L;
    }
    if (!rc) rc = sp_upload(h, pos, &h->dev.pos);
    if (!rc) rc = sp_upload(h, p2f, &h->dev.p2f);
    if (!rc) rc = sp_upload(h, wp, &h->dev.wpack);
    if (!rc) rc = sp_upload(h, hann, &h->dev.hann);
    {
        std::vector<float2> wf(L);
        for (int m = 0; m < L; ++m) wf[m] = wexp(m, L);
        if (!rc) rc = sp_upload(h, wf, &h->dev.wfull);
    }
    if (rc) {
        for (void* p : h->allocs) (void)hipFree(p);
        delete h;
        return rc;
    }
    h->generic = !bluestein && axis_needs_generic(ax);
    g_rowfft[{devid, L}] = h;
    *out = h;
    return D4W_OK;
}

}  // namespace d4w
