// limiter.h — the arithmetic and the lane schedule of the true-peak limiter (limiter.hip, Engine option "limiter"): a static gain
// followed by a look-ahead limiter on the frames an offline render delivers, where the launch set's output lies in HBM, behind the
// delivery-rate converter and in front of the pack kernel and the meter.
//
// The programme is the concatenation of the frames DELIVERED by the host-buffer render calls since the last reset, n = 0, 1, ...;
// silence lies in front of it. Channels are linked in groups of `link` consecutive channels (0: all of them), one gain per group.
// Everything is double, no contraction (the build has -ffp-contract=off). G = 10^(gain_db / 20), C = 10^(ceiling_dbtp / 20), D the
// look-ahead and R the release in frames, s = 1 / R:
//   x'_c[n] = G clean(x_c[n])                                       a non-finite sample detects as 0 (loudness::clean)
//   p[n]    = max over the group of loudness::peak_at(x'_c[n - 11 .. n])     the meter's 12-tap phases: the detector
//   a[n]    = 1 - min(1, C / p[n])                                  the reduction the peak at n asks for (p = 0: 0)
//   dm[n]   = max a[n - D - 6 .. n]                                 hold
//   M[n]    = max(M[n - 1], dm[n] + n s), M[-1] = -inf              release, linear in gain at s per frame, with ABSOLUTE indices:
//   d[n]    = max(dm[n], M[n] - n s)                                a pure prefix maximum — max is the only cross-frame operation
//   g[n]    = 1 - (sum over k = 0 .. D ascending of d[n - k]) / (D + 1)      attack smoothing
//   y_c[n]  = (float)((g[n] G) (double)x_c[n - D - 6])              the RAW sample: NaN and inf still reach the pack kernel's count
// Latency D + 6 frames, frames in = frames out. g[n] is at most the gain the peaks at n - D - 6 .. n - D ask for — the delayed sample
// and the interpolated points on either side of it (the interpolator's centre lies 6 frames back) — so the delivered SAMPLE peak
// stays under C (one float rounding). The METERED true peak of the output does not: the gain moves inside the interpolator's span.
//
// `max` is exact and associative and the sum runs in one fixed order per frame, so neither the cut into calls and launch sets nor the
// shape of a scan changes a bit. Carried from set to set, per programme: the last D + 17 raw frames of every channel (D + 6 to
// delay, 11 more for the detector's window at the oldest frame the hold looks back to), per group the last D values of d, and M.
// The reductions a in front of a set are recomputed from the carried frames — the same bits — rather than carried.
//
// A set of `valid` frames at programme frame n0, scratch in double per group: [frame] and [tile].
//   detect   workgroup <-> tile of 256 frames of one group: per channel the tile's stretch with D + 17 frames in front is staged in an
//            LDS row (unit stride from lane to lane: ds_read_b32 banks are (address / 4) mod 32, 32 consecutive floats hit 32 banks,
//            no padding needed; the doubles likewise at ds_read_b64), every slot of the D + 6 + 256 reductions is one lane's; the
//            sliding maximum by doubling (m[i] = max(m[i], m[i - w]), w = 1, 2, 4 ... up to the largest power of two P <= D + 7,
//            then two overlapping windows of P). Writes dm, and the tile's maximum of dm + n s.
//   scan     wave <-> group: exclusive prefix maximum over the tiles, seeded with the carried M; leaves the next M.
//   release  workgroup <-> tile: in-tile prefix maximum, d over dm in place; the largest d (atomicMax on the bit pattern).
//   apply    workgroup <-> tile: the tile's d with D in front (carried ones where the set begins) in LDS, the sum, g, the delayed
//            samples of the group's channels times g G; counts the frames with g < 1.
//   history  thread <-> carried value, into the OTHER of two copies; the host flips them.
//
// Plain C++ for host and device alike: tests/native/limiter_host.cpp runs the kernels' schedule with these functions workgroup by
// workgroup and lane by lane against limiter_host(), the scalar loop's production twin, which the engine uses where a render's
// floats are already on the host.
#ifndef ELEMHIP_LIMITER_H
#define ELEMHIP_LIMITER_H
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <math.h>
#include <vector>

#include "loudness.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define LM_FD __host__ __device__ __forceinline__
#else
#define LM_FD inline
#endif

namespace limiter {

constexpr uint32_t kTile = 256;           // frames per workgroup: one lane each
constexpr uint32_t kMaxD = 1024;          // look-ahead frames at most (the tile's stretch in LDS)
constexpr uint32_t kCentre = 6;           // the interpolator's centre lies this many frames behind its newest tap
constexpr uint32_t kWindow = loudness::kPhaseTaps;

struct Plan { double G, C, s; uint32_t D, R, link, pad; };
struct GroupStats { unsigned long long maxBits, limited; };      // largest d (bit pattern of a non-negative double), frames with g < 1

LM_FD uint32_t latency(const Plan& p) { return p.D + kCentre; }
LM_FD uint32_t hist_frames(const Plan& p) { return p.D + kCentre + kWindow - 1u; }       // D + 17
LM_FD uint32_t ext_frames(const Plan& p) { return kTile + p.D + kCentre; }                 // reductions a tile's holds look at
LM_FD uint32_t row_frames(const Plan& p) { return kTile + hist_frames(p); }
LM_FD uint32_t group_width(const Plan& p, uint32_t nCh) { return p.link ? p.link : nCh; }
LM_FD uint32_t group_count(const Plan& p, uint32_t nCh) { return p.link ? nCh / p.link : (nCh ? 1u : 0u); }
LM_FD bool channels_ok(const Plan& p, uint32_t nCh) { return nCh != 0u && (p.link == 0u || nCh % p.link == 0u); }

// ---- the plan (host) ----------------------------------------------------------------------------------------------------------------
inline uint32_t frames_of(double ms, double rate) { const double f = floor(ms * rate / 1000.0 + 0.5); return f >= 0.0 && f < 4294967295.0 ? (uint32_t)f : 0xFFFFFFFFu; }
// refused (false, p untouched): a ceiling outside -40 .. 0 dBTP, a gain outside -60 .. 60 dB, D outside 1 .. kMaxD, R < 1
inline bool make_plan(double rate, double ceilingDb, double gainDb, double lookaheadMs, double releaseMs, double link, Plan& p) {
    if (!(rate >= 1.0) || !(ceilingDb >= -40.0 && ceilingDb <= 0.0) || !(gainDb >= -60.0 && gainDb <= 60.0)) return false;
    if (!(lookaheadMs >= 0.0) || !(releaseMs >= 0.0) || !(link >= 0.0 && link <= 65536.0) || link != floor(link)) return false;
    const uint32_t D = frames_of(lookaheadMs, rate), R = frames_of(releaseMs, rate);
    if (D < 1u || D > kMaxD || R < 1u || R == 0xFFFFFFFFu) return false;
    p.G = pow(10.0, gainDb / 20.0); p.C = pow(10.0, ceilingDb / 20.0); p.s = 1.0 / (double)R;
    p.D = D; p.R = R; p.link = (uint32_t)link; p.pad = 0u;
    return true;
}

// ---- a frame ------------------------------------------------------------------------------------------------------------------------
LM_FD double dmax(double a, double b) { return a > b ? a : b; }
// x(m) = the channel's raw sample m frames back: the largest of the four interpolated magnitudes of G clean(x)
template <class Fetch>
LM_FD double detect(const loudness::Plan& lp, const Plan& p, Fetch x) {
    double w[kWindow];
    for (uint32_t m = 0; m < kWindow; ++m) w[m] = p.G * loudness::clean(x(m));
    return loudness::peak_at(lp, w);
}
LM_FD double reduction(const Plan& p, double peak) {
    if (!(peak > 0.0)) return 0.0;
    const double q = p.C / peak;
    return 1.0 - (q < 1.0 ? q : 1.0);
}
LM_FD double ramp(const Plan& p, uint64_t n) { return (double)n * p.s; }
LM_FD double release(double dm, double M, double ns) { return dmax(dm, M - ns); }
// d(k) = d[n - k]
template <class Fetch>
LM_FD double gain(const Plan& p, Fetch d) {
    double sum = 0.0;
    for (uint32_t k = 0; k <= p.D; ++k) sum += d(k);
    return 1.0 - sum / (double)(p.D + 1u);
}
LM_FD float apply(const Plan& p, double g, float x) { return (float)((g * p.G) * (double)x); }

// ---- a launch set: [block][channel][blockSize] in, the same layout out ---------------------------------------------------------------
// the set's frame `rel` of channel c (raw): from the set, or from the H = hist_frames carried in front of it (oldest first)
LM_FD float input_at(const float* src, uint32_t bs, uint32_t nCh, uint32_t c, uint32_t valid, const float* hist, uint32_t H, int64_t rel) {
    if (rel >= 0) {
        const uint32_t f = (uint32_t)rel;
        return rel < (int64_t)valid ? src[((size_t)(f / bs) * nCh + c) * bs + f % bs] : 0.0f;
    }
    return rel + (int64_t)H >= 0 ? hist[(int64_t)H + rel] : 0.0f;
}
LM_FD float history_next(const float* src, uint32_t bs, uint32_t nCh, uint32_t c, const float* old, uint32_t valid, uint32_t H, uint32_t j) {
    const uint64_t at = (uint64_t)valid + j;
    if (at >= H) { const uint32_t f = (uint32_t)(at - H); return src[((size_t)(f / bs) * nCh + c) * bs + f % bs]; }
    return old[at];
}
// d of the set's frame `rel`: from the group's scratch, or from the D carried values in front of the set
LM_FD double d_at(const double* d, uint32_t valid, const double* hist, uint32_t D, int64_t rel) {
    if (rel >= 0) return rel < (int64_t)valid ? d[rel] : 0.0;
    return rel + (int64_t)D >= 0 ? hist[(int64_t)D + rel] : 0.0;
}
LM_FD double d_history_next(const double* d, const double* old, uint32_t valid, uint32_t D, uint32_t j) {
    const uint64_t at = (uint64_t)valid + j;
    return at >= D ? d[at - D] : old[at];
}
LM_FD uint32_t tile_count(uint32_t valid) { return (valid + kTile - 1u) / kTile; }

// ---- the carried state: one block per copy — M[groups] | d[groups][D] | frames[channels][D + 17] -------------------------------------
LM_FD size_t state_off_d(const Plan&, uint32_t groups) { return (size_t)groups * sizeof(double); }
LM_FD size_t state_off_hist(const Plan& p, uint32_t groups) { return (size_t)groups * (1u + p.D) * sizeof(double); }
LM_FD size_t state_bytes(const Plan& p, uint32_t nCh) { return state_off_hist(p, group_count(p, nCh)) + (size_t)nCh * hist_frames(p) * sizeof(float); }
inline void state_reset(const Plan& p, uint32_t nCh, unsigned char* st) {
    memset(st, 0, state_bytes(p, nCh));
    const double minusInf = -INFINITY;
    for (uint32_t g = 0; g < group_count(p, nCh); ++g) memcpy(st + (size_t)g * sizeof(double), &minusInf, sizeof(double));
}

// ---- the detect tile, lane by lane (every function is one lane's share between two barriers) ------------------------------------------
// row slot j <-> the set's frame fFirst - (D + 17) + j; reduction slot i <-> frame fFirst - (D + 6) + i, whose window is row[i + 11 - m]
LM_FD void tile_stage(const Plan& p, const float* src, uint32_t bs, uint32_t nCh, uint32_t c, uint32_t valid, const float* hist, uint32_t fFirst, uint32_t lane, float* row) {
    const uint32_t H = hist_frames(p), X = row_frames(p);
    for (uint32_t j = lane; j < X; j += kTile) row[j] = input_at(src, bs, nCh, c, valid, hist, H, (int64_t)fFirst - (int64_t)H + (int64_t)j);
}
LM_FD void tile_detect(const loudness::Plan& lp, const Plan& p, const float* row, bool first, uint32_t lane, double* m) {
    const uint32_t E = ext_frames(p);
    for (uint32_t i = lane; i < E; i += kTile) {
        const double v = detect(lp, p, [&](uint32_t k) { return row[i + kWindow - 1u - k]; });
        m[i] = first ? v : dmax(m[i], v);
    }
}
LM_FD void tile_reduce(const Plan& p, uint32_t lane, double* m) {
    const uint32_t E = ext_frames(p);
    for (uint32_t i = lane; i < E; i += kTile) m[i] = reduction(p, m[i]);
}
// the largest power of two <= the hold's width D + 7
LM_FD uint32_t hold_pow2(const Plan& p) { uint32_t P = 1u; while (2u * P <= p.D + kCentre + 1u) P *= 2u; return P; }
LM_FD void tile_double(const Plan& p, const double* from, double* to, uint32_t w, uint32_t lane) {
    const uint32_t E = ext_frames(p);
    for (uint32_t i = lane; i < E; i += kTile) to[i] = i >= w ? dmax(from[i], from[i - w]) : from[i];
}
// m holds the maxima over P slots ending at each slot: the hold of the lane's frame, D + 7 slots ending at lane + D + 6
LM_FD double tile_hold(const Plan& p, const double* m, uint32_t P, uint32_t lane) {
    const uint32_t i = lane + p.D + kCentre;
    return dmax(m[i], m[i - (p.D + kCentre + 1u - P)]);
}
// an inclusive prefix-maximum step over the tile's lanes
LM_FD void scan_step(const double* from, double* to, uint32_t w, uint32_t lane) { to[lane] = lane >= w ? dmax(from[lane], from[lane - w]) : from[lane]; }
// the apply tile: slot i <-> the set's frame fFirst - D + i
LM_FD void tile_window(const Plan& p, const double* d, uint32_t valid, const double* hist, uint32_t fFirst, uint32_t lane, double* win) {
    for (uint32_t i = lane; i < kTile + p.D; i += kTile) win[i] = d_at(d, valid, hist, p.D, (int64_t)fFirst - (int64_t)p.D + (int64_t)i);
}
LM_FD double tile_gain(const Plan& p, const double* win, uint32_t lane) { return gain(p, [&](uint32_t k) { return win[lane + p.D - k]; }); }

// ---- the scalar loop ----------------------------------------------------------------------------------------------------------------
// x[c * xStride + f]: the programme's frames [n0, n0 + n) of nCh channels; `state` one copy of the carried state (state_reset at a new
// programme), advanced to n0 + n on return; y (not x) receives n frames per channel; stats[group] accumulate.
inline void limiter_host(const loudness::Plan& lp, const Plan& p, uint32_t nCh, unsigned char* state, GroupStats* stats, const float* x, size_t xStride,
                         size_t n, uint64_t n0, float* y, size_t yStride) {
    const uint32_t groups = group_count(p, nCh), width = group_width(p, nCh), H = hist_frames(p), D = p.D, hold = D + kCentre;
    double* M = reinterpret_cast<double*>(state);
    double* dHistAll = reinterpret_cast<double*>(state + state_off_d(p, groups));
    float* histAll = reinterpret_cast<float*>(state + state_off_hist(p, groups));
    std::vector<float> xe((size_t)width * (H + n));
    std::vector<double> a(hold + n), d(D + n);
    for (uint32_t g = 0; g < groups; ++g) {
        for (uint32_t k = 0; k < width; ++k) {
            const uint32_t c = g * width + k;
            float* e = xe.data() + (size_t)k * (H + n);
            memcpy(e, histAll + (size_t)c * H, H * sizeof(float));
            if (n) memcpy(e + H, x + (size_t)c * xStride, n * sizeof(float));
        }
        // slot i of a <-> frame n0 - hold + i, slot j of xe <-> frame n0 - H + j = slot i + 11
        for (size_t i = 0; i < hold + n; ++i) {
            double peak = 0.0;
            for (uint32_t k = 0; k < width; ++k) {
                const float* e = xe.data() + (size_t)k * (H + n);
                peak = dmax(peak, detect(lp, p, [&](uint32_t m) { return e[i + kWindow - 1u - m]; }));
            }
            a[i] = reduction(p, peak);
        }
        double* dh = dHistAll + (size_t)g * D;
        memcpy(d.data(), dh, D * sizeof(double));
        double Mg = M[g], top = loudness::bits_double(stats[g].maxBits);
        for (size_t f = 0; f < n; ++f) {
            double dm = 0.0;
            for (uint32_t k = 0; k <= hold; ++k) dm = dmax(dm, a[f + k]);
            const double ns = ramp(p, n0 + f);
            Mg = dmax(Mg, dm + ns);
            const double df = release(dm, Mg, ns);
            d[D + f] = df;
            top = dmax(top, df);
            const double gn = gain(p, [&](uint32_t k) { return d[D + f - k]; });
            if (gn < 1.0) ++stats[g].limited;
            for (uint32_t k = 0; k < width; ++k) y[(size_t)(g * width + k) * yStride + f] = apply(p, gn, xe[(size_t)k * (H + n) + H + f - hold]);
        }
        M[g] = Mg; stats[g].maxBits = loudness::double_bits(top);
        memcpy(dh, d.data() + n, D * sizeof(double));
        for (uint32_t k = 0; k < width; ++k) memcpy(histAll + (size_t)(g * width + k) * H, xe.data() + (size_t)k * (H + n) + n, H * sizeof(float));
    }
}

} // namespace limiter

#endif // ELEMHIP_LIMITER_H
