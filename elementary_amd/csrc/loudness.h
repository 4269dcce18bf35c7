// loudness.h — the arithmetic and the lane schedule of the loudness meter (loudness.hip, Engine option "loudness_meter"):
// ITU-R BS.1770-4 K-weighted mean squares per 100 ms sub-block and the 4x-oversampled true peak of every output channel of an
// offline render, measured where the launch set's output lies in HBM, and the EBU R 128 gating over the sub-block series.
//
// The programme is the concatenation of the frames DELIVERED by metered calls, in call order (not the zero padding of a call's
// last block); programme time starts at 0 at a reset. A non-finite sample meters as 0.0.
//
// K-weighting is a cascade of two biquads in double, each in transposed direct form II: four states per channel, an affine map
// s' = A s + B x per frame. A launch set's stretch of a channel is cut into segments of L frames, one lane each:
//   pass one   every lane runs its segment from zero state: the segment's zero-state end state z_k
//   scan       s_{k+1} = A^L s_k + z_k along the channel, 64 segments per wave step (Hillis-Steele with the host's A^(L 2^i)),
//              seeded with the state the previous set left
//   pass two   every lane reruns its segment from its true start state and sums the squared output into the (at most two, L <= hop)
//              sub-blocks it straddles; the last lane leaves the state for the next set
//   combine    sub-block j of the set = the carried partial sum (j = 0) + its segments' sums in segment order: no atomics, the
//              same bits every run
// The interpolator is written causally: y[4n + p] = sum_m h[p + 4m] x[n - m], m = 0 .. 11, over the "full" convolution n = 0 ..
// N + 11. The maximum over all of y does not depend on how y is indexed, so a set needs the 11 frames in front of it (carried) and
// none behind it: no lag. The zero-padded tail n = N .. N + 10 is evaluated at a read from a copy of the carried frames.
//
// Plain C++ for host and device alike: tests/native/loudness_host.cpp runs the passes with these functions lane by lane against
// meter_host() below, the scalar loop's production twin, which the engine uses where a render's floats are already on the host.
#ifndef ELEMHIP_LOUDNESS_H
#define ELEMHIP_LOUDNESS_H
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define LD_FD __host__ __device__ __forceinline__
#else
#define LD_FD inline
#endif

namespace loudness {

constexpr uint32_t kSegment = 96;         // L at most (L = min(kSegment, hop))
constexpr uint32_t kHistory = 12;         // frames carried in front of a set (the interpolator reads 11 of them)
constexpr uint32_t kPhaseTaps = 12;       // taps of each of the three interpolating phases (phase 0 is the identity)
constexpr uint32_t kScanSteps = 6;        // log2 of a wave
constexpr uint32_t kThreads = 256;

struct Biquad { double b0, b1, b2, a1, a2; };

// what the host computes once per sample rate and the kernels take by value
struct Plan {
    Biquad shelf, highpass;
    double power[kScanSteps][16];         // A^(L 2^i), row-major: the cascade's transition over L, 2L, ... 32L frames
    double fir[3][kPhaseTaps];            // phase p = 1 .. 3: fir[p - 1][m] = h[p + 4m] / (the phase's sum)
    uint32_t hop, L;
};

// everything carried per channel, device-resident (and mirrored on the host where the floats are)
struct ChannelState {
    double s[4];                          // shelf s1, s2, high-pass s1, s2
    double partial;                       // squared output summed over the open sub-block
    unsigned long long truePeakBits;      // bit pattern of a non-negative double: orders like the double
    float hist[kHistory];                 // the programme's last frames, oldest first, non-finite ones as 0
    uint32_t samplePeakBits, pad;
};

LD_FD double clean(float x) {
    uint32_t u; memcpy(&u, &x, 4);
    return (u & 0x7F800000u) != 0x7F800000u ? (double)x : 0.0;
}
LD_FD double biquad(const Biquad& q, double& s1, double& s2, double x) {
    const double y = q.b0 * x + s1;
    s1 = q.b1 * x - q.a1 * y + s2;
    s2 = q.b2 * x - q.a2 * y;
    return y;
}
LD_FD double k_step(const Plan& p, double* s, double x) { return biquad(p.highpass, s[2], s[3], biquad(p.shelf, s[0], s[1], x)); }

LD_FD unsigned long long double_bits(double x) { unsigned long long u; memcpy(&u, &x, 8); return u; }
LD_FD double bits_double(unsigned long long u) { double x; memcpy(&x, &u, 8); return x; }

// ---- a channel's frames in a launch set: [block][channel][blockSize] -------------------------------------------------------------
struct Cursor {
    const float* p; uint32_t left; size_t skip;          // frames left in the row; floats from a row's end to the channel's next row
    LD_FD float next() {
        const float x = *p++;
        if (--left == 0u) { p += skip; left = rowLen; }
        return x;
    }
    uint32_t rowLen;
};
LD_FD Cursor cursor_at(const float* src, uint32_t bs, uint32_t nCh, uint32_t c, uint32_t f) {
    const uint32_t b = f / bs, o = f % bs;
    Cursor k;
    k.p = src + ((size_t)b * nCh + c) * bs + o; k.left = bs - o; k.skip = (size_t)(nCh - 1u) * bs; k.rowLen = bs;
    return k;
}
LD_FD float frame_at(const float* src, uint32_t bs, uint32_t nCh, uint32_t c, uint32_t f) {
    return src[((size_t)(f / bs) * nCh + c) * bs + f % bs];
}

// ---- segments ----------------------------------------------------------------------------------------------------------------------
LD_FD uint32_t segment_count(uint32_t valid, uint32_t L) { return (valid + L - 1u) / L; }
LD_FD uint32_t segment_frames(uint32_t k, uint32_t valid, uint32_t L) { return valid - k * L < L ? valid - k * L : L; }
// frames of segment k that fall into the sub-block its first frame lies in (`q0`: the programme's frame count mod hop at the set's start)
LD_FD uint32_t segment_first(uint32_t k, uint32_t q0, uint32_t hop, uint32_t L) { return hop - (q0 + k * L) % hop; }

LD_FD void pass_one(const Plan& p, Cursor cur, uint32_t n, double* z) {
    z[0] = z[1] = z[2] = z[3] = 0.0;
    for (uint32_t i = 0; i < n; ++i) (void)k_step(p, z, clean(cur.next()));
}
// v += P o (a scan step: `o` is the value 2^i lanes below, P = A^(L 2^i))
LD_FD void scan_fold(const double* P, double* v, const double* o) {
    double r[4];
    for (int i = 0; i < 4; ++i) r[i] = v[i] + (((P[4 * i] * o[0] + P[4 * i + 1] * o[1]) + P[4 * i + 2] * o[2]) + P[4 * i + 3] * o[3]);
    v[0] = r[0]; v[1] = r[1]; v[2] = r[2]; v[3] = r[3];
}
LD_FD void pass_two(const Plan& p, Cursor cur, uint32_t n, uint32_t first, double* s, double* e) {
    double e0 = 0.0, e1 = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
        const double y = k_step(p, s, clean(cur.next()));
        if (i < first) e0 += y * y; else e1 += y * y;
    }
    e[0] = e0; e[1] = e1;
}
// set-local sub-block j (frame f of the set lies in (q0 + f) / hop) from the segments' sums [segment][2], in segment order
LD_FD uint32_t subblocks_touched(uint32_t q0, uint32_t valid, uint32_t hop) { return (q0 + valid + hop - 1u) / hop; }
LD_FD uint32_t subblocks_complete(uint32_t q0, uint32_t valid, uint32_t hop) { return (q0 + valid) / hop; }
LD_FD double subblock_sum(const double* e, uint32_t j, double carried, uint32_t q0, uint32_t valid, uint32_t hop, uint32_t L) {
    const uint32_t lo = j * hop > q0 ? j * hop - q0 : 0u, hiAll = (j + 1u) * hop - q0, hi = hiAll < valid ? hiAll : valid;
    double sum = j == 0u ? carried : 0.0;
    if (hi <= lo) return sum;
    for (uint32_t k = lo / L; k <= (hi - 1u) / L; ++k) sum += e[2u * k + ((q0 + k * L) / hop == j ? 0u : 1u)];
    return sum;
}

// ---- true peak -------------------------------------------------------------------------------------------------------------------
// w[m] = x[n - m], m = 0 .. 11: the largest magnitude among the four interpolated points at n
LD_FD double peak_at(const Plan& p, const double* w) {
    double best = fabs(w[0]);
    for (int ph = 0; ph < 3; ++ph) {
        double y = 0.0;
        for (uint32_t m = 0; m < kPhaseTaps; ++m) y += p.fir[ph][m] * w[m];
        best = fabs(y) > best ? fabs(y) : best;
    }
    return best;
}
// x[f - m] for a frame f of the set: from the set, or from the carried frames in front of it
LD_FD double window_frame(const float* src, uint32_t bs, uint32_t nCh, uint32_t c, const float* hist, uint32_t f, uint32_t m) {
    return m <= f ? clean(frame_at(src, bs, nCh, c, f - m)) : (double)hist[kHistory + f - m];
}
// the carried frames after a set of `valid` frames: slot j (oldest first)
LD_FD float history_next(const float* src, uint32_t bs, uint32_t nCh, uint32_t c, const float* old, uint32_t valid, uint32_t j) {
    return valid + j >= kHistory ? (float)clean(frame_at(src, bs, nCh, c, valid + j - kHistory)) : old[j + valid];
}
// the zero-padded tail behind the programme, from a COPY of the state: the peak a read reports
inline double peak_with_tail(const Plan& p, const ChannelState& st) {
    double best = bits_double(st.truePeakBits);
    for (uint32_t t = 1; t < kPhaseTaps; ++t) {
        double w[kPhaseTaps];
        for (uint32_t m = 0; m < kPhaseTaps; ++m) w[m] = m < t ? 0.0 : (double)st.hist[kHistory - 1u + t - m];
        const double v = peak_at(p, w);
        best = v > best ? v : best;
    }
    return best;
}

// ---- the plan (host) ---------------------------------------------------------------------------------------------------------------
inline void mat4_mul(const double* a, const double* b, double* out) {
    double r[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) { double s = 0.0; for (int k = 0; k < 4; ++k) s += a[4 * i + k] * b[4 * k + j]; r[4 * i + j] = s; }
    memcpy(out, r, sizeof r);
}
inline Biquad shelf_coeffs(double fs) {
    const double pi = 3.14159265358979323846, f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = tan(pi * f0 / fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416), a0 = 1.0 + K / Q + K * K;
    return Biquad{(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0};
}
inline Biquad highpass_coeffs(double fs) {
    const double pi = 3.14159265358979323846, f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = tan(pi * f0 / fs), a0 = 1.0 + K / Q + K * K;
    return Biquad{1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0};
}
inline void make_plan(double fs, Plan& p) {
    const double pi = 3.14159265358979323846;
    p.shelf = shelf_coeffs(fs); p.highpass = highpass_coeffs(fs);
    const double hop = floor(fs / 10.0 + 0.5);
    p.hop = hop < 1.0 ? 1u : (uint32_t)hop;
    p.L = p.hop < kSegment ? p.hop : kSegment;
    // column j of A^L: L frames of silence from the unit state e_j — the very steps the lanes take
    for (int j = 0; j < 4; ++j) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        s[j] = 1.0;
        for (uint32_t i = 0; i < p.L; ++i) (void)k_step(p, s, 0.0);
        for (int r = 0; r < 4; ++r) p.power[0][4 * r + j] = s[r];
    }
    for (uint32_t i = 1; i < kScanSteps; ++i) mat4_mul(p.power[i - 1], p.power[i - 1], p.power[i]);
    for (uint32_t ph = 1; ph < 4; ++ph) {
        double h[kPhaseTaps], sum = 0.0;
        for (uint32_t m = 0; m < kPhaseTaps; ++m) {
            const double j = (double)(ph + 4u * m), t = (j - 24.0) / 4.0;
            h[m] = sin(pi * t) / (pi * t) * 0.5 * (1.0 - cos(2.0 * pi * j / 48.0));      // (t is never 0 off phase 0)
            sum += h[m];
        }
        for (uint32_t m = 0; m < kPhaseTaps; ++m) p.fir[ph - 1u][m] = h[m] / sum;
    }
}

// ---- the scalar loop ---------------------------------------------------------------------------------------------------------------
// `n` frames of one channel at programme frame `t0`; a completed sub-block's mean square goes to emit(value)
template <class Emit>
inline void meter_host(const Plan& p, ChannelState& st, const float* x, size_t n, uint64_t t0, Emit emit) {
    uint32_t fill = (uint32_t)(t0 % p.hop);
    double peak = bits_double(st.truePeakBits);
    for (size_t f = 0; f < n; ++f) {
        const double xd = clean(x[f]);
        const float xf = (float)xd;
        uint32_t a; memcpy(&a, &xf, 4); a &= 0x7FFFFFFFu;
        st.samplePeakBits = a > st.samplePeakBits ? a : st.samplePeakBits;
        double w[kPhaseTaps];
        w[0] = xd;
        for (uint32_t m = 1; m < kPhaseTaps; ++m) w[m] = (double)st.hist[kHistory - m];
        const double v = peak_at(p, w);
        peak = v > peak ? v : peak;
        memmove(st.hist, st.hist + 1, (kHistory - 1u) * sizeof(float));
        st.hist[kHistory - 1u] = xf;
        const double y = k_step(p, st.s, xd);
        st.partial += y * y;
        if (++fill == p.hop) { emit(st.partial / (double)p.hop); st.partial = 0.0; fill = 0u; }
    }
    st.truePeakBits = double_bits(peak);
}

// ---- gating (host) -----------------------------------------------------------------------------------------------------------------
struct Gated { double integrated, momentaryMax, shortTermMax; uint64_t blocks, gatedBlocks; };
inline double lufs_of(double power) { return power > 0.0 ? -0.691 + 10.0 * log10(power) : -INFINITY; }
// ms[channel][subBlocks] mean squares, weights[channel] (null: 1.0 each). 400 ms blocks = 4 sub-blocks, hop 1; short term = 30.
inline Gated gate(const double* ms, size_t channels, size_t subBlocks, const double* weights) {
    Gated g{-INFINITY, -INFINITY, -INFINITY, 0u, 0u};
    auto window = [&](size_t i, size_t len) {
        double power = 0.0;
        for (size_t c = 0; c < channels; ++c) {
            double z = 0.0;
            for (size_t k = 0; k < len; ++k) z += ms[c * subBlocks + i + k];
            power += (weights ? weights[c] : 1.0) * (z / (double)len);
        }
        return power;
    };
    for (size_t i = 0; i + 30u <= subBlocks; ++i) { const double l = lufs_of(window(i, 30)); g.shortTermMax = l > g.shortTermMax ? l : g.shortTermMax; }
    if (subBlocks < 4u) return g;
    g.blocks = subBlocks - 3u;
    double absSum = 0.0; uint64_t absN = 0;
    for (size_t i = 0; i + 4u <= subBlocks; ++i) {
        const double pw = window(i, 4), l = lufs_of(pw);
        g.momentaryMax = l > g.momentaryMax ? l : g.momentaryMax;
        if (l > -70.0) { absSum += pw; ++absN; }
    }
    if (!absN) return g;
    const double rel = lufs_of(absSum / (double)absN) - 10.0;
    double sum = 0.0; uint64_t cnt = 0;
    for (size_t i = 0; i + 4u <= subBlocks; ++i) {
        const double pw = window(i, 4), l = lufs_of(pw);
        if (l > -70.0 && l > rel) { sum += pw; ++cnt; }
    }
    g.gatedBlocks = cnt;
    if (cnt) g.integrated = lufs_of(sum / (double)cnt);
    return g;
}

} // namespace loudness

#endif // ELEMHIP_LOUDNESS_H
