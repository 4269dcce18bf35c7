// noise_shape.h — the arithmetic and the tile schedule of noise-shaped requantisation (noise_shape.hip, elemhip_noise_shape_set).
//
// An error-feedback quantiser in front of s16 / s24 / FLAC delivery: the requantisation error of the last K samples of a channel,
// filtered by c_1 .. c_K, is taken off the next sample before it is rounded, so the error's spectrum is that of plain dither times
// the noise transfer function 1 - sum c_k z^-k. The TPDF dither is pcm_pack's (the same two hashes, keyed on seed, channel and the
// ABSOLUTE frame), taken at 8 fraction bits.
//
// Everything behind the float's split is int32: the sample as xi + xf / 256 LSB, the dither in Q8, the coefficients in Q11, the errors
// in Q8 clamped to +-kErrMax (64 LSB; a clamp counts as a saturation). With sum |cq_k| <= kSumMax the feedback sum stays below 2^31 and
// every product fits a 24-bit multiply. Host twin and kernel agree to the bit without a word about FMA contraction: the two float
// products of the split (x * 2^(bits-1), frac * 256) are exact.
//
// The state of a channel (ChannelState: the K newest errors, newest first, and the saturation count) is carried from set to set and
// from call to call, so the codes of a programme do not depend on how it is cut.
//
// The kernel's schedule — one workgroup per kChannels channels, which walks the set's tiles of up to kTile frames of one block in
// order; phases A (all lanes: split and dither into LDS rows), B (a lane per channel: the recurrence along its row) and C (all lanes:
// the codes to HBM) — is plain index arithmetic below: tests/native/noise_shape_host.cpp runs it lane by lane against shape_host(),
// the scalar loop the engine itself uses where a render's floats are on the host (engine_host_blocks.cpp).
#ifndef ELEMHIP_NOISE_SHAPE_H
#define ELEMHIP_NOISE_SHAPE_H
#include <stdint.h>
#include <stddef.h>
#include "pcm_pack.h"

namespace noise_shape {

constexpr uint32_t kErrFrac = 8;                 // F: fraction bits of an error
constexpr uint32_t kCoefFrac = 11;               // Q: fraction bits of a coefficient
constexpr uint32_t kMaxTaps = 12;
constexpr int32_t  kErrMax = 1 << 14;            // E: 64 LSB
constexpr int32_t  kSumMax = 131071;             // sum |cq_k| at most: kSumMax * kErrMax + 2^10 < 2^31

PCM_CX bool taps_ok(uint32_t K) { return K >= 1u && K <= kMaxTaps; }
PCM_CX bool bits_ok(uint32_t bits) { return bits == 16u || bits == 24u; }

// cq_k = floor(c_k * 2048 + 0.5), in double; false (and cq untouched past the failing entry) for a set that is refused
inline bool quantise_coeffs(const float* c, uint32_t K, int32_t* cq) {
    if (!taps_ok(K) || !c) return false;
    int64_t sum = 0;
    for (uint32_t k = 0; k < K; ++k) {
        if (!pcm_pack::finite_bits(pcm_pack::float_bits(c[k]))) return false;
        const double v = __builtin_floor((double)c[k] * 2048.0 + 0.5);
        if (v > (double)kSumMax || v < -(double)kSumMax) return false;
        cq[k] = (int32_t)v;
        sum += cq[k] < 0 ? -(int64_t)cq[k] : (int64_t)cq[k];
    }
    return sum <= (int64_t)kSumMax;
}

struct ChannelState {                            // 64 bytes, zero at a programme's start
    int32_t  e[kMaxTaps];                        // e[0] newest
    uint64_t saturated;
    uint64_t reserved;
};
static_assert(sizeof(ChannelState) == 64, "one cache line half");

// ---- one sample ------------------------------------------------------------------------------------------------------------------
// what does not depend on the recurrence (phase A): x -> xi, and xf + dq with dq next to it
struct Split { int32_t xi, packed; };            // packed = dq << 16 | (xf + dq) & 0xFFFF: xf in 0 .. 256, dq in -255 .. 255
PCM_FD int32_t packed_sum(int32_t p) { return (int32_t)((uint32_t)p << 16) >> 16; }      // xf + dq
PCM_FD int32_t packed_dither(int32_t p) { return p >> 16; }                                // dq

PCM_FD int32_t dither_q8(uint32_t hiKey, uint32_t lo) {
    const uint32_t k = pcm_pack::hash32(lo ^ hiKey);
    const uint32_t r1 = pcm_pack::hash32(k), r2 = pcm_pack::hash32(k ^ 0x85EBCA6Bu);     // dither_lo's two hashes
    return (int32_t)(r1 >> 24) - (int32_t)(r2 >> 24);
}
PCM_FD Split split(float x, uint32_t bits, int32_t dq) {
    const float S = bits == 16u ? 32768.0f : 8388608.0f;
    if (!pcm_pack::finite_bits(pcm_pack::float_bits(x))) x = 0.0f;
    x = x < -2.0f ? -2.0f : (x > 2.0f ? 2.0f : x);
    const float w = x * S;                       // exact
    const float fl = __builtin_floorf(w);
    const int32_t xf = (int32_t)__builtin_floorf((w - fl) * 256.0f + 0.5f);      // (the product is exact: contracted or not, the same bits)
    return Split{(int32_t)fl, (int32_t)(((uint32_t)dq << 16) | ((uint32_t)(xf + dq) & 0xFFFFu))};
}

// the recurrence (phase B): acc = sum cq_k e[k-1] comes from the caller, who knows how it holds e
struct Step { int32_t code, err; uint32_t sat; };
PCM_FD Step step(Split s, int32_t acc, int32_t lo, int32_t hi) {
    const int32_t fb = (acc + (1 << (kCoefFrac - 1u))) >> kCoefFrac;
    const int32_t r = packed_sum(s.packed) - fb;
    int32_t y = s.xi + ((r + 128) >> kErrFrac);
    y = y < lo ? lo : (y > hi ? hi : y);
    int32_t d = y - s.xi;
    d = d < -128 ? -128 : (d > 128 ? 128 : d);
    int32_t en = d * 256 - r + packed_dither(s.packed);       // (d << 8) - (xf - fb)
    const uint32_t sat = en > kErrMax || en < -kErrMax ? 1u : 0u;
    en = en > kErrMax ? kErrMax : (en < -kErrMax ? -kErrMax : en);
    return Step{y, en, sat};
}
PCM_CX int32_t code_min(uint32_t bits) { return bits == 16u ? -32768 : -8388608; }
PCM_CX int32_t code_max(uint32_t bits) { return bits == 16u ? 32767 : 8388607; }

// ---- the scalar loop -------------------------------------------------------------------------------------------------------------
// planar[c] + frame -> codes[c] + frame (rows `stride` apart in both), frames [0, n) at absolute time t0; row c is channel
// channel0 + c of the dither's key. `state` ([channels], in-out) may be null: a programme of its own that is forgotten.
inline void shape_host(const int32_t* cq, uint32_t K, uint32_t bits, bool dith, uint32_t seed, uint32_t channel0, int64_t t0,
                       const float* planar, uint32_t channels, size_t stride, size_t n, ChannelState* state, int32_t* codes) {
    const int32_t lo = code_min(bits), hi = code_max(bits);
    for (uint32_t c = 0; c < channels; ++c) {
        ChannelState st{};
        if (state) st = state[c];
        const uint32_t k0 = pcm_pack::channel_key(seed, channel0 + c);
        const float* row = planar + (size_t)c * stride;
        int32_t* out = codes + (size_t)c * stride;
        for (size_t f = 0; f < n; ++f) {
            const uint64_t t = (uint64_t)(t0 + (int64_t)f);
            const int32_t dq = dith ? dither_q8(pcm_pack::hi_key(k0, (uint32_t)(t >> 32)), (uint32_t)(t & 0xFFFFFFFFu)) : 0;
            int32_t acc = 0;
            for (uint32_t k = 0; k < K; ++k) acc += cq[k] * st.e[k];
            const Step s = step(split(row[f], bits, dq), acc, lo, hi);
            for (uint32_t k = K - 1u; k > 0u; --k) st.e[k] = st.e[k - 1u];
            st.e[0] = s.err;
            st.saturated += s.sat;
            out[f] = s.code;
        }
        if (state) state[c] = st;
    }
}

// ---- tiles -----------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kChannels = 16;               // CH: channels (phase B's lanes) of a workgroup
constexpr uint32_t kTile = 256;                  // T: frames of a tile at most
constexpr uint32_t kMaxBlock = pcm_pack::kMaxBlock;

PCM_FD uint32_t group_count(uint32_t channels) { return (channels + kChannels - 1u) / kChannels; }
PCM_FD uint32_t group_channels(uint32_t channels, uint32_t group) { const uint32_t c0 = group * kChannels; return channels - c0 < kChannels ? channels - c0 : kChannels; }
PCM_FD uint32_t tiles_per_block(uint32_t bs) { return (bs + kTile - 1u) / kTile; }
// tiles of a set in the order a workgroup walks them: tile j = (block j / tiles_per_block, tile j % tiles_per_block)
PCM_FD uint32_t tile_count(uint32_t bs, uint32_t validFrames) { return ((validFrames + bs - 1u) / bs) * tiles_per_block(bs); }
PCM_FD uint32_t tile_first(uint32_t ti) { return ti * kTile; }
// frames of tile `ti` of block `b` that are shaped (0: the tile lies behind the set's valid frames)
PCM_FD uint32_t tile_valid(uint32_t bs, uint32_t b, uint32_t ti, uint32_t validFrames) {
    const uint32_t f0 = tile_first(ti);
    if (f0 >= bs) return 0u;
    const uint64_t abs0 = (uint64_t)b * bs + f0;
    if (abs0 >= validFrames) return 0u;
    uint32_t n = bs - f0 < kTile ? bs - f0 : kTile;
    if ((uint64_t)n > validFrames - abs0) n = (uint32_t)(validFrames - abs0);
    return n;
}
// where frame f0 + f of channel c of block b lies in the set's floats — and its code in the buffer of the same shape
PCM_FD size_t sample_index(uint32_t bs, uint32_t numChannels, uint32_t b, uint32_t c, uint32_t f) { return ((size_t)b * numChannels + c) * bs + f; }

// Phases A and C: wave w takes the rows w, w + kWaves, ..; its lanes the frames lane, lane + 64, .. of the row: 256 consecutive bytes
// of HBM per wave instruction, 64 consecutive pairs (A) or codes (C) of LDS.
PCM_FD uint32_t sweep_row(uint32_t wave, uint32_t i) { return wave + i * kWaves; }
PCM_FD uint32_t sweep_frame(uint32_t lane, uint32_t j) { return lane + j * 64u; }

// ---- LDS rows --------------------------------------------------------------------------------------------------------------------
// Phase B's lanes 0 .. kChannels - 1 walk their rows in step: at frame f lane g reads the pair (xi, packed) of row g with one 8-byte
// read and writes the code of row g with one 4-byte write. 8-byte reads see 64 banks of 4 bytes, and the 16 lanes lie in one half-wave
// (one conflict group): with pair rows 2 * kTile + 2 dwords apart, row g's pair f starts at bank (2 g + 2 f) mod 64 — the 16 lanes
// take 32 distinct banks. 4-byte writes see 32 banks: with code rows kTile + 1 dwords apart lane g writes bank (g + f) mod 32 —
// 16 distinct banks. Phases A and C run along a row: consecutive lanes, consecutive addresses. The codes have rows of their own (not
// the pairs' first word) so that no read of phase B's row has to wait for a write to it: they are issued ahead of the recurrence.
constexpr uint32_t kPairRowDwords = 2u * kTile + 2u;
constexpr uint32_t kCodeRowDwords = kTile + 1u;
static_assert(kPairRowDwords % 64u == 2u && kCodeRowDwords % 32u == 1u, "the bank argument above");
PCM_FD uint32_t pair_dword(uint32_t g, uint32_t f) { return g * kPairRowDwords + 2u * f; }
PCM_FD uint32_t code_dword(uint32_t g, uint32_t f) { return g * kCodeRowDwords + f; }
constexpr uint32_t kPairDwords = kChannels * kPairRowDwords;
constexpr uint32_t kCodeDwords = kChannels * kCodeRowDwords;

} // namespace noise_shape

#endif // ELEMHIP_NOISE_SHAPE_H
