// The travel time between a channel and a position: the one definition the localisation units share (loc.hip, assoc.hip,
// stack.hip, beam.hip).  Nothing else in those units turns two positions into a distance or a delay, so "the same bits as
// the other unit's table" (stack_grid's column and the order-0 beam, the vote and the select of one round) is a property of
// this header and not of four texts kept alike by hand.
//
// float64, differences first, the three squares added left to right, the correctly rounded square root.  No contraction
// (pragma below, set here so that it travels with the functions into whatever kernel inlines them): the distance is the
// same sequence of roundings everywhere, and the one NumPy makes.
//
// Two forms of "divided by c0" exist and stay apart.  loc.hip mirrors the reference and divides, dist / c0, at its call
// sites; the vote, the stack and the beam multiply by a reciprocal formed once on the host (moveout_samples, and assoc.hip's
// dist * inv_c0).  The two differ in the last bit, tests pin each, and neither is to be turned into the other.
#pragma once
#include "d4w_internal.h"

#ifndef D4W_EMU
#pragma clang fp contract(off)
#endif

namespace d4w {

constexpr int kMoveoutDelayMax = 1 << 30;        // the cap of a delay in samples; column ranges stay within +- it

// |(cx, cy, cz) - (px, py, pz)|
__device__ __forceinline__ double moveout_dist(double cx, double cy, double cz, double px, double py, double pz) {
    const double dx = cx - px, dy = cy - py, dz = cz - pz;
    return sqrt(dx * dx + dy * dy + dz * dz);
}

// the travel time in samples, inv_c0 = 1 / c0 formed on the host
__device__ __forceinline__ double moveout_samples(double cx, double cy, double cz, double px, double py, double pz, double inv_c0, double fs) {
    return moveout_dist(cx, cy, cz, px, py, pz) * inv_c0 * fs;
}

// tau rounded half up, capped; a NaN lands on the cap as well
__device__ __forceinline__ int moveout_round(double tau) {
    const double q = floor(tau + 0.5);
    return q < (double)kMoveoutDelayMax ? (int)q : kMoveoutDelayMax;
}

// k = floor(tau), capped like moveout_round, and f = float32(tau - k) with 0 <= f < 1: a fraction that rounds to 1.0f is carried
__device__ __forceinline__ void moveout_split(double tau, int& k, float& f) {
    const double q = floor(tau);
    k = kMoveoutDelayMax;
    f = 0.f;
    if (q < (double)kMoveoutDelayMax) {
        k = (int)q;
        f = (float)(tau - q);
        if (f >= 1.0f) {
            k += 1;
            f = 0.f;
        }
    }
}

// host side: the checks of c0, fs, dt, of a [nch x ns] block with its row pitch and of a record that every entry point makes
static inline bool positive_finite(double v) { return std::isfinite(v) && v > 0.0; }

static inline int check_block(const char* who, int nch, int ns, long long pitch) {
    if (nch < 1 || ns < 1) return fail(D4W_EINVAL, "%s: the block %d x %d is empty", who, nch, ns);
    if (pitch < ns) return fail(D4W_EINVAL, "%s: the row pitch %lld is below the %d samples of a row", who, pitch, ns);
    return D4W_OK;
}

// a record: the block and, behind it, the optional next block of the same channels (beam, align, levels, project)
static inline int check_record(const char* who, int nch, int ns, long long pitch, const void* xnext, int ns_next, long long pitch_next) {
    const int rc = check_block(who, nch, ns, pitch);
    if (rc) return rc;
    if (xnext) return check_block((std::string(who) + ", next block").c_str(), nch, ns_next, pitch_next);
    if (ns_next != 0) return fail(D4W_EINVAL, "%s: %d samples of a next block that is not given", who, ns_next);
    return D4W_OK;
}

}  // namespace d4w
