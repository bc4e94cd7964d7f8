// What the beam and its transpose share beyond the travel time (beam.hip, project.hip; levels.hip for the window; align.hip
// for the clamp): the interpolation coefficients of a fractional delay, the description of a window of a row of the record
// and the clamp of a call's first sample.  One text each, so that "the exact transpose of the beam's taps", "the same window
// rule" and "the same clamp" are properties of this header.
#pragma once
#include "moveout.h"

#ifndef D4W_EMU
#pragma clang fp contract(off)
#endif

namespace d4w {

// weight x interpolation coefficient of the taps kLo .. kHi of order 0 (nearest sample: l[0] = w), 1 (linear, taps 0, 1) and
// 3 (four-point Lagrange, taps -1 .. 2), formed in float32 from the fraction f in [0, 1).  w = 1.f multiplies exactly.
template <int ORDER>
__device__ __forceinline__ void delay_taps(float w, float f, float (&l)[ORDER + 1]) {
    if constexpr (ORDER == 0) {
        l[0] = w;
    } else if constexpr (ORDER == 1) {
        l[0] = w * (1.f - f);
        l[1] = w * f;
    } else {
        const float fp = f + 1.f, fm = f - 1.f, fmm = f - 2.f;
        l[0] = w * (-(f * fm * fmm) * (1.f / 6.f));
        l[1] = w * ((fp * fm * fmm) * 0.5f);
        l[2] = w * (-(fp * f * fmm) * 0.5f);
        l[3] = w * ((fp * f * fm) * (1.f / 6.f));
    }
}

// the channels one thread of the beam sums from 0 (beam.hip says why 128): the beam and the sums of coherence.hip split the
// channels in the same fixed segments, so that the latter's b plane is the beam bit for bit
constexpr int kBeamSegment = 128;

// a window of len samples: sample i is pa[i] for i < split, pb[i - split] after; len = 0: not valid, never read
struct LevelWindow {
    const float* pa;
    const float* pb;
    int split, len;
};

// the window [q0, q0 + len) of a row (row / rown: the block's and the next block's), valid iff it lies inside the record
__device__ __forceinline__ LevelWindow level_window(const float* row, const float* rown, long long q0, int len, long long ns, long long ntot) {
    LevelWindow w{nullptr, nullptr, 0, 0};
    if (len < 1 || q0 < 0 || q0 + len > ntot) return w;
    w.len = len;
    if (q0 >= ns) {
        w.pa = rown + (q0 - ns);
        w.split = len;
    } else {
        w.pa = row + q0;
        w.pb = rown;
        w.split = (int)min((long long)len, ns - q0);
    }
    return w;
}

// the first emission sample of a call, clamped so that the sums of it, a delay and a length cannot overflow (beam.hip,
// align.hip, levels.hip, project.hip)
constexpr long long kStartMax = 1ll << 62;

__device__ __forceinline__ long long clamp_start(long long start) { return min(max(start, -kStartMax), kStartMax); }

}  // namespace d4w
