// automation.h — the arithmetic and the schedule of breakpoint automation (automation.hip, elemhip_automation_set).
//
// A lane is a sorted list of breakpoints {frame, value, curve} bound to one engine input channel; its value is a pure function of the
// ABSOLUTE engine frame t (the call's sampleTime + the frame's index in the call), so a render does not depend on how it is cut and
// nothing is carried, on either side. With i the LAST point whose frame is <= t:
//   no such point (t before the first)      the first point's value
//   i is the last point                     its value
//   curve_i = kHold, or t == frame_i        value_i, bit for bit
//   curve_i = kLinear                       in double: u = (double)(t - f_i) / (double)(f_{i+1} - f_i); y = a + (b - a) * u with
//                                           a = value_i, b = value_{i+1} widened; these operations in this order, no FMA (the units
//                                           that include this header are built with -ffp-contract=off, and the pragma below says it
//                                           again); rounded once to float32
// Several points on one frame make a jump: the last of them is the value from that frame on (it is point i there), the first of them
// is what a ramp into that frame aims at (it is point i + 1 of the segment in front), any between the two have no effect. A segment
// between two points on one frame is never evaluated, so no difference of frames that is divided by is zero.
//
// A linear segment is at most 2^52 frames long: t - f_i and f_{i+1} - f_i are then exact in double.
//
// The kernel's schedule — one workgroup per (block of the set, lane channel), a thread per span of kSpan consecutive frames of the row:
// segment_at for the span's first frame, then along the span one comparison per frame and a search among the points behind the current
// one only where that comparison says a point was reached — is Cursor below; value_host() is the scalar loop the engine itself runs
// where a render's inputs are on the host (engine_host_blocks.cpp), through the same Cursor.
#ifndef ELEMHIP_AUTOMATION_H
#define ELEMHIP_AUTOMATION_H
#include <stdint.h>
#include <stddef.h>
#include "pcm_pack.h"

namespace automation {

constexpr uint32_t kHold = 0, kLinear = 1;
constexpr uint32_t kMaxChannels = 32;                // lanes bind to engine input channels 0 .. 31
constexpr size_t   kMaxPoints = (size_t)1 << 20;
constexpr uint64_t kMaxSegment = (uint64_t)1 << 52;  // frames of a linear segment at most
constexpr uint32_t kSpan = 4;                        // frames per thread and step: one 16-byte store
constexpr uint32_t kThreads = 256;

struct Point { int64_t frame; float value; uint32_t curve; };
static_assert(sizeof(Point) == 16, "the table's stride");

// a lane that is refused changes nothing (elemhip_automation_set answers kInvalidPropertyValue)
inline bool lane_ok(const Point* p, size_t count) {
    if (!p || count == 0 || count > kMaxPoints) return false;
    for (size_t i = 0; i < count; ++i) {
        if (!pcm_pack::finite_bits(pcm_pack::float_bits(p[i].value)) || p[i].curve > kLinear) return false;
        if (i + 1 < count) {
            if (p[i + 1].frame < p[i].frame) return false;
            if (p[i].curve == kLinear && (uint64_t)p[i + 1].frame - (uint64_t)p[i].frame > kMaxSegment) return false;
        }
    }
    return true;
}

// the index of the last point whose frame is <= t; -1 where t lies before the first
PCM_FD int64_t segment_at(const Point* p, size_t count, int64_t t) {
    size_t lo = 0, hi = count;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (p[mid].frame <= t) lo = mid + 1; else hi = mid;
    }
    return (int64_t)lo - 1;
}

// the value at t, given i = segment_at(p, count, t); count >= 1
PCM_FD float value_in(const Point* p, size_t count, int64_t i, int64_t t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (i < 0) return p[0].value;
    const Point a = p[i];
    if ((size_t)i + 1 >= count || a.curve == kHold || t == a.frame) return a.value;
    const Point b = p[i + 1];
    const double u = (double)(t - a.frame) / (double)(b.frame - a.frame);
    const double d = (double)b.value - (double)a.value;
    const double m = d * u;
    const double y = (double)a.value + m;
    return (float)y;
}

// a walk along consecutive frames: at(t) for non-decreasing t
struct Cursor {
    const Point* p; size_t count; int64_t i;
    PCM_FD Cursor(const Point* points, size_t n, int64_t t) : p(points), count(n), i(segment_at(points, n, t)) {}
    PCM_FD float at(int64_t t) {
        const size_t next = (size_t)(i + 1);
        if (next < count && p[next].frame <= t) i = (int64_t)next + segment_at(p + next, count - next, t);      // (the points in front stay behind)
        return value_in(p, count, i, t);
    }
};

// the scalar twin: out[k] = the lane's value at t0 + k, k < n
inline void value_host(const Point* p, size_t count, int64_t t0, size_t n, float* out) {
    if (n == 0) return;
    Cursor c(p, count, t0);
    for (size_t k = 0; k < n; ++k) out[k] = c.at(t0 + (int64_t)k);
}

} // namespace automation
#endif
