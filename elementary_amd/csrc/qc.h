// qc.h — the definitions and the arithmetic of the inspector (qc.hip, elemhip_qc_set): technical QC of what an offline render delivers —
// silence at the head and the tail, digital-silence dropouts, runs of clipped samples, DC, energy, the phase of channel pairs and a
// min / max overview — read where the launch set's output lies in HBM, behind the converter and the limiter, before any quantisation.
//
// The programme is the concatenation of the frames DELIVERED by inspected calls, in call order (not the zero padding of a call's last
// block), less the first `skip` of them and cut after `limit` (0: unbounded); programme frame 0 is the first frame after a reset. A
// non-finite sample is counted and then inspected as 0.0. A frame is QUIET iff |x| <= silenceLevel and CLIPPED iff |x| >= clipLevel.
//
// Findings are runs, and a run may start in one lane's stretch and end in another wave, launch set or call. So a stretch of frames is
// described by a summary with an associative combine (Runs): its length, the run at its head, the run at its tail (both the whole
// length when every frame is set) and the CLOSED runs inside it of at least `minRun` frames — count, the longest (ties: the earliest)
// and the first. combine(a, b) closes a.tail + b.head into one run when neither side is all set; a side that is all set passes through
// and keeps growing. A dropout is a closed quiet run of the programme's summary (it has a non-quiet frame on either side); a clip event
// is any clipped run of at least clipRun frames, the head and the open tail run included (report()). Everything here is integer or
// comparison arithmetic: exact, the same in any tree.
//
// The float64 sums (x, x^2, x_a x_b: the products are exact in double) follow one order that depends on programme frame indices alone:
// leaves of kLeaf programme frames (frame / kLeaf), each summed in frame order from 0.0; leaves are added to the total in leaf order;
// the open leaf's partial is carried; a read returns total + partial (Sums, sums_add, fold_leaves). No atomics, the same bits however
// the render is cut.
//
// The overview (bucket > 0): min and max of every complete run of `bucket` programme frames; min keeps the earliest of equals, so it
// too is the same in any in-order tree.
//
// Plain C++ for host and device alike: tests/native/qc_host.cpp runs the kernels' phases with these functions lane by lane against
// channel_host() / pair_host() below, the scalar twin, which the engine uses where a render's floats are already on the host.
#ifndef ELEMHIP_QC_H
#define ELEMHIP_QC_H
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define QC_FD __host__ __device__ __forceinline__
#else
#define QC_FD inline
#endif

namespace qc {

constexpr uint32_t kLeaf = 64;                          // programme frames per leaf of the float64 sums
constexpr uint32_t kTileLeaves = 128;                   // leaves one workgroup walks, one lane each
constexpr uint32_t kTileFrames = kLeaf * kTileLeaves;   // tiles are aligned in the PROGRAMME: tile = frame / kTileFrames
constexpr uint32_t kRowStride = kLeaf + 1;              // a leaf's row in LDS, padded: lane l reads bank (l + j) % 64
constexpr uint32_t kThreads = 128;
constexpr uint32_t kPairLeaves = 64;                    // the pair kernel stages two channels: half a tile of each
constexpr uint32_t kMaxPairs = 128;
constexpr uint32_t kMaxClipRun = 65535, kMinBucket = 16, kMaxBucket = 1048576;

struct Spec { float silenceLevel, clipLevel; uint32_t clipRun, dropoutFrames, bucket, numPairs; };

QC_FD bool spec_ok(float silenceLevel, float clipLevel, uint32_t clipRun, uint32_t dropoutFrames, uint32_t bucket, uint32_t numPairs) {
    return silenceLevel >= 0.0f && silenceLevel <= 3.4028234e38f && clipLevel > 0.0f && clipLevel <= 3.4028234e38f && clipRun >= 1u && clipRun <= kMaxClipRun &&
           dropoutFrames >= 1u && dropoutFrames <= 0x7FFFFFFFu && (bucket == 0u || (bucket >= kMinBucket && bucket <= kMaxBucket)) && numPairs <= kMaxPairs;
}

// ---- a frame -------------------------------------------------------------------------------------------------------------------------
struct Frame { float x; bool nonfinite, quiet, clipped; };
QC_FD Frame classify(float raw, const Spec& sp) {
    uint32_t u; memcpy(&u, &raw, 4);
    Frame f;
    f.nonfinite = (u & 0x7F800000u) == 0x7F800000u;
    f.x = f.nonfinite ? 0.0f : raw;
    const float a = fabsf(f.x);
    f.quiet = a <= sp.silenceLevel; f.clipped = a >= sp.clipLevel;
    return f;
}

// ---- runs of a flag over a stretch (U: uint32_t inside a launch set, uint64_t for the programme) ---------------------------------------
template <class U> QC_FD U none() { return (U) ~(U)0; }
template <class U> struct Runs {
    U len, head, tail;                    // frames; the set run at the start; the set run at the end (both = len when all are set)
    U count, longest, longestAt, firstAt; // the closed runs inside of at least minRun frames; positions: none() when there is none
};
template <class U> QC_FD Runs<U> runs_empty() { return Runs<U>{0, 0, 0, 0, 0, none<U>(), none<U>()}; }
template <class U> QC_FD void runs_close(Runs<U>& r, U length, U at) {      // (in position order: the earliest of equals stays the longest)
    r.count += 1;
    if (length > r.longest) { r.longest = length; r.longestAt = at; }
    if (r.firstAt == none<U>()) r.firstAt = at;
}
// the frame at `pos` behind the stretch
template <class U> QC_FD void runs_push(Runs<U>& r, bool set, U pos, U minRun) {
    if (set) { if (r.head == r.len) r.head += 1; r.tail += 1; }
    else {
        if (r.head != r.len && r.tail >= minRun && r.tail > 0) runs_close(r, r.tail, (U)(pos - r.tail));
        r.tail = 0;
    }
    r.len += 1;
}
// b lies behind a and starts at position bStart
template <class U> QC_FD Runs<U> runs_combine(const Runs<U>& a, const Runs<U>& b, U bStart, U minRun) {
    const bool aAll = a.head == a.len, bAll = b.head == b.len;
    Runs<U> r = a;
    r.len = a.len + b.len;
    r.head = aAll ? a.len + b.head : a.head;
    r.tail = bAll ? b.len + a.tail : b.tail;
    if (!aAll && !bAll) {
        const U run = a.tail + b.head;
        if (run > 0 && run >= minRun) runs_close(r, run, (U)(bStart - a.tail));
    }
    r.count += b.count;
    if (b.longest > r.longest) { r.longest = b.longest; r.longestAt = b.longestAt; }
    if (r.firstAt == none<U>()) r.firstAt = b.firstAt;
    return r;
}

// ---- everything exact about a stretch of one channel ----------------------------------------------------------------------------------
template <class U> struct Stretch {
    Runs<U> quiet, clip;
    U nonfinite, quietFrames, clippedFrames, peakAt;
    float mn, mx, peakAbs; uint32_t pad;
};
template <class U> QC_FD Stretch<U> stretch_empty() {
    Stretch<U> s;
    s.quiet = runs_empty<U>(); s.clip = runs_empty<U>();
    s.nonfinite = s.quietFrames = s.clippedFrames = 0; s.peakAt = none<U>();
    s.mn = INFINITY; s.mx = -INFINITY; s.peakAbs = -1.0f; s.pad = 0u;
    return s;
}
template <class U> QC_FD void stretch_push(Stretch<U>& s, const Frame& f, U pos, const Spec& sp) {
    runs_push<U>(s.quiet, f.quiet, pos, (U)sp.dropoutFrames);
    runs_push<U>(s.clip, f.clipped, pos, (U)sp.clipRun);
    s.nonfinite += f.nonfinite ? 1 : 0; s.quietFrames += f.quiet ? 1 : 0; s.clippedFrames += f.clipped ? 1 : 0;
    const float a = fabsf(f.x);
    if (a > s.peakAbs) { s.peakAbs = a; s.peakAt = pos; }
    if (f.x < s.mn) s.mn = f.x;
    if (f.x > s.mx) s.mx = f.x;
}
template <class U> QC_FD Stretch<U> stretch_combine(const Stretch<U>& a, const Stretch<U>& b, U bStart, const Spec& sp) {
    Stretch<U> r;
    r.quiet = runs_combine<U>(a.quiet, b.quiet, bStart, (U)sp.dropoutFrames);
    r.clip = runs_combine<U>(a.clip, b.clip, bStart, (U)sp.clipRun);
    r.nonfinite = a.nonfinite + b.nonfinite; r.quietFrames = a.quietFrames + b.quietFrames; r.clippedFrames = a.clippedFrames + b.clippedFrames;
    const bool later = b.peakAbs > a.peakAbs;
    r.peakAbs = later ? b.peakAbs : a.peakAbs; r.peakAt = later ? b.peakAt : a.peakAt;
    r.mn = b.mn < a.mn ? b.mn : a.mn;
    r.mx = b.mx > a.mx ? b.mx : a.mx;
    r.pad = 0u;
    return r;
}
// a launch set's summary, positions counted from the set's first programme frame p0, as the programme counts them
QC_FD uint64_t widen_at(uint32_t at, uint64_t p0) { return at == none<uint32_t>() ? none<uint64_t>() : p0 + at; }
QC_FD Runs<uint64_t> widen(const Runs<uint32_t>& r, uint64_t p0) {
    return Runs<uint64_t>{r.len, r.head, r.tail, r.count, r.longest, widen_at(r.longestAt, p0), widen_at(r.firstAt, p0)};
}
QC_FD Stretch<uint64_t> widen(const Stretch<uint32_t>& s, uint64_t p0) {
    Stretch<uint64_t> r;
    r.quiet = widen(s.quiet, p0); r.clip = widen(s.clip, p0);
    r.nonfinite = s.nonfinite; r.quietFrames = s.quietFrames; r.clippedFrames = s.clippedFrames; r.peakAt = widen_at(s.peakAt, p0);
    r.mn = s.mn; r.mx = s.mx; r.peakAbs = s.peakAbs; r.pad = 0u;
    return r;
}

// ---- the float64 sums ----------------------------------------------------------------------------------------------------------------
struct Sums { double total, partial; };
QC_FD void sums_add(Sums& s, double term, uint64_t pos) {       // the term of programme frame `pos`
    s.partial += term;
    if ((pos & (kLeaf - 1u)) == kLeaf - 1u) { s.total += s.partial; s.partial = 0.0; }
}
QC_FD double sums_value(const Sums& s) { return s.total + s.partial; }
QC_FD uint32_t leaf_count(uint64_t p0, uint32_t count) { return count ? (uint32_t)((p0 + count + kLeaf - 1u) / kLeaf - p0 / kLeaf) : 0u; }
QC_FD uint32_t tile_count(uint64_t p0, uint32_t count) { return count ? (uint32_t)((p0 + count + kTileFrames - 1u) / kTileFrames - p0 / kTileFrames) : 0u; }
// leaf i of a stretch of `count` frames from p0 on: `value` is its sum — begun from the carried partial where the leaf began before p0
QC_FD void fold_leaf(Sums& s, double value, uint32_t i, uint64_t p0, uint32_t count) {
    const uint64_t end = (p0 / kLeaf + i + 1u) * kLeaf;
    if (end <= p0 + count) { s.total += value; s.partial = 0.0; } else s.partial = value;
}

// ---- what is carried per channel and per pair, device-resident (and mirrored on the host where the floats are) -----------------------
struct ChannelState {
    Stretch<uint64_t> s;
    Sums sum, sq;
    float bMin, bMax; uint32_t bCount, pad;       // the open bucket of the overview
};
typedef Sums PairState;
QC_FD ChannelState state_empty() {
    ChannelState st;
    st.s = stretch_empty<uint64_t>(); st.sum = Sums{0.0, 0.0}; st.sq = Sums{0.0, 0.0};
    st.bMin = INFINITY; st.bMax = -INFINITY; st.bCount = 0u; st.pad = 0u;
    return st;
}

// ---- the overview: a piece is a bucket's part inside a tile's range ---------------------------------------------------------------------
QC_FD void minmax_fold(float& mn, float& mx, float bmn, float bmx) { if (bmn < mn) mn = bmn; if (bmx > mx) mx = bmx; }
// the pieces of tile range [lo, hi) that are no whole bucket: the first bucket's ("lead") and, where it is another, the last one's ("trail")
QC_FD bool has_lead(uint64_t lo, uint64_t hi, uint32_t B) { const uint64_t g = lo / B; return !(g * B == lo && (g + 1u) * B <= hi); }
QC_FD bool has_trail(uint64_t lo, uint64_t hi, uint32_t B) { const uint64_t g = (hi - 1u) / B; return g != lo / B && (g + 1u) * B > hi; }
// the open bucket takes a piece of `frames` frames that ends in bucket g; a bucket it completes goes to out[g - g0]
QC_FD void bucket_merge(ChannelState& st, float mn, float mx, uint32_t frames, uint32_t B, uint64_t g, uint64_t g0, float* out, size_t outStride) {
    minmax_fold(st.bMin, st.bMax, mn, mx);
    st.bCount += frames;
    if (st.bCount == B) {
        out[(size_t)(g - g0) * outStride] = st.bMin; out[(size_t)(g - g0) * outStride + 1u] = st.bMax;
        st.bMin = INFINITY; st.bMax = -INFINITY; st.bCount = 0u;
    }
}
QC_FD uint32_t buckets_complete(uint64_t p0, uint32_t count, uint32_t B) { return B ? (uint32_t)((p0 + count) / B - p0 / B) : 0u; }

// ---- the scalar twin ----------------------------------------------------------------------------------------------------------------
// `n` frames of one channel behind programme frame p0; complete buckets go to out[2 k], out[2 k + 1], k counted from bucket p0 / bucket
inline void channel_host(const Spec& sp, ChannelState& st, const float* x, size_t n, uint64_t p0, float* out) {
    const uint64_t g0 = sp.bucket ? p0 / sp.bucket : 0u;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t pos = p0 + i;
        const Frame f = classify(x[i], sp);
        stretch_push<uint64_t>(st.s, f, pos, sp);
        const double d = (double)f.x;
        sums_add(st.sum, d, pos);
        sums_add(st.sq, d * d, pos);
        if (sp.bucket) bucket_merge(st, f.x, f.x, 1u, sp.bucket, pos / sp.bucket, g0, out, 2u);
    }
}
inline void pair_host(PairState& st, const float* a, const float* b, size_t n, uint64_t p0, const Spec& sp) {
    for (size_t i = 0; i < n; ++i) sums_add(st, (double)classify(a[i], sp).x * (double)classify(b[i], sp).x, p0 + i);
}

// ---- what a read returns per channel -------------------------------------------------------------------------------------------------
struct RunReport { uint64_t count, longest, longestAt, firstAt; };
struct ChannelReport {
    uint64_t frames, nonfinite, quietFrames, clippedFrames, peakAt, headSilence, tailSilence;
    RunReport dropouts, clipEvents;
    double sum, sumSq;
    float mn, mx, bucketMin, bucketMax; uint32_t bucketFrames, pad;
};
inline ChannelReport report(const Spec& sp, const ChannelState& st) {
    const Stretch<uint64_t>& s = st.s;
    ChannelReport r{};
    r.frames = s.quiet.len; r.nonfinite = s.nonfinite; r.quietFrames = s.quietFrames; r.clippedFrames = s.clippedFrames; r.peakAt = s.peakAt;
    r.headSilence = s.quiet.head; r.tailSilence = s.quiet.tail;
    r.dropouts = RunReport{s.quiet.count, s.quiet.longest, s.quiet.longestAt, s.quiet.firstAt};
    // clip events: the run at frame 0 in front of the closed ones, the open run at the end behind them
    Runs<uint64_t> c = runs_empty<uint64_t>();
    if (s.clip.head >= sp.clipRun) runs_close<uint64_t>(c, s.clip.head, 0u);
    c.count += s.clip.count;
    if (s.clip.longest > c.longest) { c.longest = s.clip.longest; c.longestAt = s.clip.longestAt; }
    if (c.firstAt == none<uint64_t>()) c.firstAt = s.clip.firstAt;
    if (s.clip.head != s.clip.len && s.clip.tail >= sp.clipRun) runs_close<uint64_t>(c, s.clip.tail, s.clip.len - s.clip.tail);
    r.clipEvents = RunReport{c.count, c.longest, c.longestAt, c.firstAt};
    r.sum = sums_value(st.sum); r.sumSq = sums_value(st.sq);
    r.mn = r.frames ? s.mn : 0.0f; r.mx = r.frames ? s.mx : 0.0f;
    r.bucketMin = st.bCount ? st.bMin : 0.0f; r.bucketMax = st.bCount ? st.bMax : 0.0f; r.bucketFrames = st.bCount; r.pad = 0u;
    return r;
}

// the part of `valid` delivered frames that enters the programme: `delivered` frames were delivered before them, `frames` entered
struct Window { uint32_t q0, count; };
QC_FD Window window(uint64_t delivered, uint64_t frames, uint64_t skip, uint64_t limit, uint64_t valid) {
    const uint64_t lead = delivered < skip ? (skip - delivered < valid ? skip - delivered : valid) : 0u;
    uint64_t count = valid - lead;
    if (limit) { const uint64_t room = limit > frames ? limit - frames : 0u; if (count > room) count = room; }
    return Window{(uint32_t)lead, (uint32_t)count};
}

} // namespace qc
#endif
