// flac_encode.h — the arithmetic, the decision rules and the lane schedule of FLAC delivery (flac_encode.hip, Engine::processBlocksFlac).
//
// A render's delivered frames, quantised exactly as PCM delivery quantises them (pcm_pack::quantise, the same dither key), leave as
// RFC 9639 "subset" FLAC frames of a fixed block size: CONSTANT, VERBATIM and FIXED (order 0..4) subframes with partitioned Rice
// residuals, and for two-channel streams the cheapest of independent, left/side, side/right and mid/side. Every choice is made on
// EXACT bit counts before a bit is written; a block of equal samples is CONSTANT, otherwise the smallest count wins and ties go to
// the simpler kind and then the lower number
// (CONSTANT, VERBATIM, FIXED 0..4; lower partition order; lower Rice parameter, a parameter before the escape; independent, left/side,
// side/right, mid/side). With option "flac_lpc_order" = P > 0 two LPC orders (P and ceil(P / 2), flac_lpc.h) are priced on top, to the bit
// like the FIXED ones; they come last in the tie rule, by ascending order. Integer arithmetic only — but for the LPC coefficients'
// recursion and quantisation, which one lane does in double under the rules flac_lpc.h states (+ - x / and floor() in a written order,
// no contraction) and the twin repeats statement by statement: the kernel's bytes are encode_host()'s.
//
// The kernels (flac_encode.hip):
//   stage     thread <-> frame of a channel row: quantise, fold the statistics, codes to [channel][programme frame] behind the carried ones
//   encode    one workgroup of 256 lanes per (FLAC frame, subframe candidate): a lane owns a run of at most 16 consecutive samples
//             (lane_run) inside ONE smallest partition; per predictor order the lanes' sums of (u >> k) for every Rice parameter k are
//             merged pairwise up a 9-level tree (tree_level) whose levels 0..pmax ARE the partition orders; decide(); an exclusive scan
//             of the lanes' code lengths; the bits are ORed into a zero-initialised image (only terminators and low bits are written)
//   assemble  one workgroup per (stream, FLAC frame): stereo mode, header, the chosen subframes shift-copied to their bit offsets
//             (frame_byte), CRC-16 per lane chunk combined by crc16_advance, frames stored back to back at the scanned byte offsets
//
// Plain C++ for host and device alike: tests/native/flac_encode_host.cpp runs the lane functions lane by lane against encode_host().
#ifndef ELEMHIP_FLAC_ENCODE_H
#define ELEMHIP_FLAC_ENCODE_H
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <vector>

#include "pcm_pack.h"
#include "flac_lpc.h"

namespace flac_encode {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxFrame = 4096;
constexpr uint32_t kMaxChannels = 8;           // channels of one stream
constexpr uint32_t kMaxOrder = 4;
constexpr uint32_t kRows = kMaxOrder + 1u + kLpcSlots;      // rows of the pricing tables: FIXED 0 .. 4, then the priced LPC orders
PCM_CX uint32_t lpc_row(uint32_t slot) { return kMaxOrder + 1u + slot; }
constexpr uint32_t kLevels = 9;                // tree levels 0..8: level L has 2^L nodes of 256 >> L lanes each
constexpr uint32_t kMaxParams = 31;            // Rice parameters 0..30 (5-bit method); 0..14 with the 4-bit method
constexpr uint32_t kEscape = 0x80u;            // a partition's choice: the parameter, or kEscape | raw bits

PCM_CX bool frame_ok(uint32_t ff) { return ff == 256u || ff == 512u || ff == 1024u || ff == 2048u || ff == 4096u; }
PCM_CX bool bits_ok(uint32_t bits) { return bits == 16u || bits == 24u; }
PCM_CX uint32_t param_bits(uint32_t bits) { return bits == 16u ? 4u : 5u; }          // the residual coding method's parameter width
PCM_CX uint32_t param_count(uint32_t bits) { return bits == 16u ? 15u : 31u; }       // (the all-ones value is the escape)
// candidates of a stream's frame: the channels, and for two channels left, right, mid, side
PCM_CX uint32_t candidates(uint32_t G) { return G == 2u ? 4u : G; }
PCM_CX uint32_t candidate_bps(uint32_t G, uint32_t bits, uint32_t cand) { return bits + (G == 2u && cand == 3u ? 1u : 0u); }
PCM_FD int32_t candidate_sample(uint32_t G, uint32_t cand, int32_t a, int32_t b) {      // a, b: the two channels' codes (G == 2)
    if (G != 2u || cand == 0u) return a;
    return cand == 1u ? b : cand == 2u ? (a + b) >> 1 : a - b;
}
// 32-bit words a subframe's bits take at most (its VERBATIM form), one spare word behind them
PCM_CX uint32_t slot_words(uint32_t ff, uint32_t bits) { return (8u + (bits + 1u) * ff + 31u) / 32u + 1u; }

// ---- CRCs (init 0, unreflected, no final xor) --------------------------------------------------------------------------------------
PCM_FD uint8_t crc8_update(uint8_t crc, uint8_t b) {
    crc ^= b;
    for (int i = 0; i < 8; ++i) crc = (uint8_t)((crc & 0x80u) ? (crc << 1) ^ 0x07u : (crc << 1));
    return crc;
}
PCM_FD uint16_t crc16_update(uint16_t crc, uint8_t b) {
    crc ^= (uint16_t)(b << 8);
    for (int i = 0; i < 8; ++i) crc = (uint16_t)((crc & 0x8000u) ? (crc << 1) ^ 0x8005u : (crc << 1));
    return crc;
}
// a(x) b(x) mod x^16 + x^15 + x^2 + 1
PCM_FD uint16_t crc16_mul(uint16_t a, uint16_t b) {
    uint16_t r = 0;
    for (int i = 15; i >= 0; --i) {
        r = (uint16_t)((r & 0x8000u) ? (r << 1) ^ 0x8005u : (r << 1));
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}
// the combine table: x^(8 * 2^k) mod P, the factor that advances a CRC over 2^k bytes
constexpr uint32_t kCrcPowers = 24;
PCM_FD uint16_t crc16_power(uint32_t k) {
    uint16_t p = 0x0100u;                      // x^8
    for (uint32_t i = 0; i < k; ++i) p = crc16_mul(p, p);
    return p;
}
// the CRC of a chunk, advanced over `bytes` bytes that follow it: a CRC with init 0 is linear, so crc(A | B) = advance(crc(A), |B|) ^ crc(B)
PCM_FD uint16_t crc16_advance(uint16_t crc, uint32_t bytes) {
    uint16_t p = 0x0100u;
    for (uint32_t k = 0; k < kCrcPowers && (bytes >> k); ++k) {
        if ((bytes >> k) & 1u) crc = crc16_mul(crc, p);
        p = crc16_mul(p, p);
    }
    return crc;
}

// ---- frame header --------------------------------------------------------------------------------------------------------------------
PCM_FD uint32_t utf8_bytes(uint32_t v) { return v < 0x80u ? 1u : v < 0x800u ? 2u : v < 0x10000u ? 3u : v < 0x200000u ? 4u : v < 0x4000000u ? 5u : 6u; }
PCM_FD uint32_t utf8_put(uint32_t v, uint8_t* out) {          // v <= 2^31 - 1
    const uint32_t n = utf8_bytes(v);
    if (n == 1u) { out[0] = (uint8_t)v; return 1u; }
    for (uint32_t i = n - 1u; i > 0u; --i) { out[i] = (uint8_t)(0x80u | (v & 0x3Fu)); v >>= 6; }
    out[0] = (uint8_t)((0xFF00u >> n) | v);
    return n;
}
PCM_FD uint32_t block_size_code(uint32_t n, uint32_t ff) {      // a whole frame: the table's code; the short final frame: explicit
    if (n == ff) return ff == 256u ? 8u : ff == 512u ? 9u : ff == 1024u ? 10u : ff == 2048u ? 11u : 12u;
    return n <= 256u ? 6u : 7u;
}
PCM_FD uint32_t sample_rate_code(uint32_t rate) {
    switch (rate) {
        case 88200u: return 1u; case 176400u: return 2u; case 192000u: return 3u; case 8000u: return 4u; case 16000u: return 5u;
        case 22050u: return 6u; case 24000u: return 7u; case 32000u: return 8u; case 44100u: return 9u; case 48000u: return 10u;
        case 96000u: return 11u; default: break;
    }
    if (rate == 0u) return 0u;
    if (rate <= 65535u) return 13u;                                  // Hz, 16 bits
    if (rate % 10u == 0u && rate / 10u <= 65535u) return 14u;        // tens of Hz, 16 bits
    if (rate % 1000u == 0u && rate / 1000u <= 255u) return 12u;      // kHz, 8 bits
    return 0u;                                                       // "see STREAMINFO"
}
constexpr uint32_t kMaxHeader = 16;
constexpr uint32_t INDEPENDENT = 0, LEFT_SIDE = 1, SIDE_RIGHT = 2, MID_SIDE = 3;
PCM_FD uint32_t header_bytes(uint32_t n, uint32_t ff, uint32_t rate, uint32_t number) {
    const uint32_t bc = block_size_code(n, ff), rc = sample_rate_code(rate);
    return 4u + utf8_bytes(number) + (bc == 6u ? 1u : bc == 7u ? 2u : 0u) + (rc == 12u ? 1u : rc >= 13u ? 2u : 0u) + 1u;
}
PCM_FD uint32_t header_put(uint32_t n, uint32_t ff, uint32_t rate, uint32_t G, uint32_t bits, uint32_t mode, uint32_t number, uint8_t* out) {
    const uint32_t bc = block_size_code(n, ff), rc = sample_rate_code(rate);
    const uint32_t ca = mode == INDEPENDENT ? G - 1u : 7u + mode;
    uint32_t p = 0;
    out[p++] = 0xFFu; out[p++] = 0xF8u;
    out[p++] = (uint8_t)((bc << 4) | rc);
    out[p++] = (uint8_t)((ca << 4) | ((bits == 16u ? 4u : 6u) << 1));
    p += utf8_put(number, out + p);
    if (bc == 6u) out[p++] = (uint8_t)(n - 1u);
    else if (bc == 7u) { out[p++] = (uint8_t)((n - 1u) >> 8); out[p++] = (uint8_t)(n - 1u); }
    if (rc == 12u) out[p++] = (uint8_t)(rate / 1000u);
    else if (rc >= 13u) { const uint32_t v = rc == 13u ? rate : rate / 10u; out[p++] = (uint8_t)(v >> 8); out[p++] = (uint8_t)v; }
    uint8_t crc = 0;
    for (uint32_t i = 0; i < p; ++i) crc = crc8_update(crc, out[i]);
    out[p++] = crc;
    return p;
}
// bytes of a frame whose subframes take `subBits` bits in all
PCM_FD uint32_t frame_bytes(uint32_t headerBytes, uint64_t subBits) { return headerBytes + (uint32_t)((subBits + 7u) / 8u) + 2u; }
// what a call that delivers `frames` frames can return at most per stream, whatever the block size: the carried frames in front of
// them included (under 4096), every frame VERBATIM under the longest header
PCM_FD uint64_t stream_bound(uint64_t frames, uint32_t G, uint32_t bits) {
    const uint64_t nFrames = frames / 256u + 2u;
    return nFrames * (kMaxHeader + 2u + G) + ((frames + kMaxFrame) * G * bits + 7u) / 8u;
}
// one frame of n samples at most
PCM_FD uint32_t frame_bound(uint32_t n, uint32_t G, uint32_t bits) { return kMaxHeader + (G * (8u + bits * n) + 7u) / 8u + 2u; }

// ---- predictors ----------------------------------------------------------------------------------------------------------------------
// the FIXED predictor's residual at sample i >= order (25-bit side samples at order 4 reach 2^29: int32 holds them)
PCM_FD int32_t residual(const int32_t* s, uint32_t i, uint32_t order) {
    switch (order) {
        case 0: return s[i];
        case 1: return s[i] - s[i - 1];
        case 2: return s[i] - 2 * s[i - 1] + s[i - 2];
        case 3: return s[i] - 3 * s[i - 1] + 3 * s[i - 2] - s[i - 3];
        default: return s[i] - 4 * s[i - 1] + 6 * s[i - 2] - 4 * s[i - 3] + s[i - 4];
    }
}
PCM_FD uint32_t zigzag(int32_t r) { return ((uint32_t)r << 1) ^ (uint32_t)(r >> 31); }
PCM_FD uint32_t bit_length(uint32_t u) { return u ? 32u - (uint32_t)__builtin_clz(u) : 0u; }     // = the two's-complement width of a residual with zigzag u
PCM_FD uint32_t max_order(uint32_t n) { return n > kMaxOrder ? kMaxOrder : n - 1u; }             // an order needs a residual: order < n

// ---- shape of a frame: partitions and lane runs ------------------------------------------------------------------------------------------
// pmax: the largest partition order that keeps partitions whole and >= 16 samples, 8 at most. The 2^pmax smallest partitions are cut
// over 256 >> pmax lanes each, so a lane's run lies inside one of them and holds n / 256 samples, rounded up: 16 at most.
struct Shape { uint32_t n, pmax, lanesPer, run, part; };
PCM_FD Shape shape(uint32_t n) {
    Shape s{n, 0u, 0u, 0u, 0u};
    while (s.pmax < 8u && (n & ((2u << s.pmax) - 1u)) == 0u && (n >> (s.pmax + 1u)) >= 16u) ++s.pmax;
    s.lanesPer = kThreads >> s.pmax; s.part = n >> s.pmax; s.run = (s.part + s.lanesPer - 1u) / s.lanesPer;
    return s;
}
PCM_FD void lane_run(const Shape& s, uint32_t lane, uint32_t& begin, uint32_t& end) {
    const uint32_t p = lane / s.lanesPer, sub = lane % s.lanesPer, base = p * s.part;
    const uint32_t b = sub * s.run, e = b + s.run;
    begin = base + (b < s.part ? b : s.part); end = base + (e < s.part ? e : s.part);
}
// node j of level L lies at lane j * (256 >> L) of the lanes' arrays; its choice at param[(1 << L) - 1 + j]
PCM_FD uint32_t node_lane(uint32_t L, uint32_t j) { return j * (kThreads >> L); }
PCM_FD uint32_t node_slot(uint32_t L, uint32_t j) { return (1u << L) - 1u + j; }
constexpr uint32_t kNodeSlots = 512;

PCM_FD uint32_t sat_add(uint32_t a, uint32_t b) { const uint64_t s = (uint64_t)a + b; return s > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)s; }

// the cheapest coding of a partition of `cnt` residuals: sum(k) = sum of (u >> k) (saturated sums are above every escape), maxU their largest
// zigzag. Returns the bits, *code = k or kEscape | raw bits.
template <class Sum>
PCM_FD uint32_t choose_param(uint32_t bits, uint32_t cnt, uint32_t maxU, Sum sum, uint32_t* code) {
    const uint32_t pb = param_bits(bits), K = param_count(bits);
    uint64_t best = ~(uint64_t)0; uint32_t bk = 0;
    for (uint32_t k = 0; k < K; ++k) {
        const uint64_t c = (uint64_t)pb + (uint64_t)cnt * (1u + k) + sum(k);
        if (c < best) { best = c; bk = k; }
    }
    const uint32_t raw = bit_length(maxU);
    const uint64_t esc = (uint64_t)pb + 5u + (uint64_t)cnt * raw;
    if (raw < 32u && esc < best) { best = esc; bk = kEscape | raw; }      // (5 bits name the width: an LPC residual of 32 bits stays Rice-coded)
    *code = bk;
    return (uint32_t)best;
}

// ---- the encode kernel's shared memory, and its phases lane by lane ------------------------------------------------------------------------
// (the image takes the sums' place once the decisions are made; before the first leaf they hold the windowed samples, then the
// workspace of the lane that designs the LPC candidates, whose lags arrive through maxU)
struct Work {
    int32_t  codes[kMaxFrame];
    union {
        uint32_t sums[kMaxParams * kThreads];    // [k][lane]; later the image: slot_words() words at most
        LpcScratch lpcWork;
    };
    uint16_t cnt[kThreads];                      // (a lane's run, and a node's samples: 4096 at most)
    uint32_t maxU[kThreads];
    uint32_t total[kRows][kLevels];              // [row][partition order]: the residual's partitions in all
    uint32_t rootMax[kRows];
    uint8_t  param[kRows][kNodeSlots];
    LpcPlan  lpc;
};
struct FixedResidual { const int32_t* s; uint32_t order; PCM_FD int32_t operator()(uint32_t i) const { return residual(s, i, order); } };
PCM_FD LpcResidual lpc_residual(const int32_t* s, const LpcPlan& plan, uint32_t slot) { return LpcResidual{s, plan.coef[slot], plan.order[slot], plan.shift[slot]}; }
struct OrPlain { PCM_FD void operator()(uint32_t* p, uint32_t v) const { *p |= v; } };
struct AddPlain { PCM_FD void operator()(uint32_t* p, uint32_t v) const { *p += v; } };

// phase 1 (per row): the lane's run -> its leaf of the tree; `order` warm-up samples have no residual, res(i) is sample i's
template <class Res>
PCM_FD void leaf_with(Work& w, const Shape& s, uint32_t bits, uint32_t order, uint32_t lane, Res res) {
    uint32_t b, e;
    lane_run(s, lane, b, e);
    if (b < order) b = order < e ? order : e;
    const uint32_t K = param_count(bits);
    uint32_t u[16], m = 0;
    const uint32_t c = e - b;
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) { u[j] = b + j < e ? zigzag(res(b + j)) : 0u; m = u[j] > m ? u[j] : m; }
    for (uint32_t k = 0; k < K; ++k) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) sum = sat_add(sum, u[j] >> k);
        w.sums[k * kThreads + lane] = sum;
    }
    w.cnt[lane] = (uint16_t)c; w.maxU[lane] = m;
}
PCM_FD void leaf(Work& w, const Shape& s, uint32_t bits, uint32_t order, uint32_t lane) { leaf_with(w, s, bits, order, lane, FixedResidual{w.codes, order}); }
PCM_FD void leaf_lpc(Work& w, const Shape& s, uint32_t bits, uint32_t slot, uint32_t lane) {
    leaf_with(w, s, bits, w.lpc.order[slot], lane, lpc_residual(w.codes, w.lpc, slot));
}
// phase 2 (per row — a FIXED order, or lpc_row(slot) —, L = 8 .. 0, a barrier between levels): lane j < 2^L merges node j's halves and, where the level is a partition
// order, prices the partition
template <class Add>
PCM_FD void tree_level(Work& w, const Shape& s, uint32_t bits, uint32_t order, uint32_t L, uint32_t lane, Add add) {
    if (lane >= (1u << L)) return;
    const uint32_t at = node_lane(L, lane), K = param_count(bits);
    if (L < 8u) {
        const uint32_t half = at + (kThreads >> (L + 1u));
        for (uint32_t k = 0; k < K; ++k) w.sums[k * kThreads + at] = sat_add(w.sums[k * kThreads + at], w.sums[k * kThreads + half]);
        w.cnt[at] = (uint16_t)(w.cnt[at] + w.cnt[half]);
        w.maxU[at] = w.maxU[at] > w.maxU[half] ? w.maxU[at] : w.maxU[half];
    }
    if (L == 0u) w.rootMax[order] = w.maxU[0];
    if (L > s.pmax) return;
    uint32_t code;
    const uint32_t* sums = w.sums;
    const uint32_t cost = choose_param(bits, w.cnt[at], w.maxU[at], [&](uint32_t k) { return (uint64_t)sums[k * kThreads + at]; }, &code);
    w.param[order][node_slot(L, lane)] = (uint8_t)code;
    add(&w.total[order][L], cost);
}

// ---- the decision ------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t CONSTANT = 0, VERBATIM = 1, FIXED = 2, LPC = 3;
struct Decision { uint32_t kind, order, porder, bits, slot = 0u; };      // slot: which priced LPC order (kind == LPC)
PCM_FD uint32_t decision_row(const Decision& d) { return d.kind == LPC ? lpc_row(d.slot) : d.order; }
// total[row][p]: the partitions' bits at partition order p; rootMax[1] == 0: every sample equals its predecessor. `lpc`: the priced LPC
// orders whose rows are filled (null: none); one that was dropped, or whose residual left int32 (rootMax == kLpcOverflow), is no candidate.
PCM_FD Decision decide(const Shape& s, uint32_t bps, const uint32_t (*total)[kLevels], const uint32_t* rootMax, const LpcPlan* lpc = nullptr) {
    const bool constant = s.n == 1u || rootMax[1] == 0u;
    // a constant block is CONSTANT. (Only for digital silence is there a shorter form, by one bit: FIXED 0 with a zero-width escape
    // partition. A silent frame is header + G (8 + bps) bits + CRC all the same: every reader knows that form.)
    if (constant) return Decision{CONSTANT, 0u, 0u, 8u + bps};
    Decision d{VERBATIM, 0u, 0u, 8u + bps * s.n};
    for (uint32_t o = 0; o <= max_order(s.n); ++o) {
        uint32_t rb = total[o][0], bp = 0;
        for (uint32_t p = 1; p <= s.pmax; ++p) if (total[o][p] < rb) { rb = total[o][p]; bp = p; }
        const uint64_t all = 8ull + (uint64_t)bps * o + 6u + rb;
        if (all < d.bits) d = Decision{FIXED, o, bp, (uint32_t)all};
    }
    for (uint32_t i = 0; lpc && i < lpc->count; ++i) {
        const uint32_t row = lpc_row(i);
        if (lpc->drop[i] != LPC_OK || rootMax[row] == kLpcOverflow) continue;
        uint32_t rb = total[row][0], bp = 0;
        for (uint32_t p = 1; p <= s.pmax; ++p) if (total[row][p] < rb) { rb = total[row][p]; bp = p; }
        const uint64_t all = (uint64_t)lpc_base(bps, lpc->order[i], lpc->precision) + rb;
        if (all < d.bits) d = Decision{LPC, lpc->order[i], bp, (uint32_t)all, i};
    }
    return d;
}
// independent, left/side, side/right, mid/side from the four candidates' bits
PCM_FD uint32_t choose_stereo(uint32_t l, uint32_t r, uint32_t m, uint32_t sd) {
    uint64_t best = (uint64_t)l + r; uint32_t mode = INDEPENDENT;
    if ((uint64_t)l + sd < best) { best = (uint64_t)l + sd; mode = LEFT_SIDE; }
    if ((uint64_t)sd + r < best) { best = (uint64_t)sd + r; mode = SIDE_RIGHT; }
    if ((uint64_t)m + sd < best) { best = (uint64_t)m + sd; mode = MID_SIDE; }
    return mode;
}
// the candidate that is subframe `ch` (0, 1) of a two-channel frame
PCM_FD uint32_t stereo_candidate(uint32_t mode, uint32_t ch) {
    return mode == INDEPENDENT ? ch : mode == LEFT_SIDE ? (ch ? 3u : 0u) : mode == SIDE_RIGHT ? (ch ? 1u : 3u) : (ch ? 3u : 2u);
}

// ---- bits ----------------------------------------------------------------------------------------------------------------------------------
// bit p of a stream is bit 31 - (p & 31) of word p >> 5 (the words leave byte-swapped). `nb` <= 32 bits of v at position pos.
template <class Or>
PCM_FD void put_bits(uint32_t* image, uint32_t pos, uint32_t nb, uint32_t v, Or orw) {
    if (nb == 0u) return;
    if (nb < 32u) v &= (1u << nb) - 1u;
    const uint32_t w = pos >> 5, sh = pos & 31u;
    if (sh + nb <= 32u) { if (v) orw(image + w, v << (32u - sh - nb)); return; }
    const uint32_t lo = sh + nb - 32u;
    if (v >> lo) orw(image + w, v >> lo);
    if (v << (32u - lo)) orw(image + w + 1u, v << (32u - lo));
}
PCM_FD uint32_t sample_len(uint32_t code, uint32_t u) { return (code & kEscape) ? (code & 31u) : 1u + code + (u >> code); }
// phase 3: the bits of the lane's run under the decision (a lane that opens a partition carries its parameter)
template <class Res>
PCM_FD uint32_t lane_bits_with(const Work& w, const Shape& s, uint32_t bits, const Decision& d, uint32_t lane, Res res) {
    uint32_t b, e;
    lane_run(s, lane, b, e);
    if (b < d.order) b = d.order < e ? d.order : e;
    const uint32_t span = kThreads >> d.porder, code = w.param[decision_row(d)][node_slot(d.porder, lane / span)];
    uint32_t len = lane % span == 0u ? param_bits(bits) + ((code & kEscape) ? 5u : 0u) : 0u;
    for (uint32_t i = b; i < e; ++i) len += sample_len(code, zigzag(res(i)));
    return len;
}
PCM_FD uint32_t lane_bits(const Work& w, const Shape& s, uint32_t bits, const Decision& d, uint32_t lane) {
    if (d.kind == FIXED) return lane_bits_with(w, s, bits, d, lane, FixedResidual{w.codes, d.order});
    if (d.kind == LPC) return lane_bits_with(w, s, bits, d, lane, lpc_residual(w.codes, w.lpc, d.slot));
    return 0u;
}
// what stands in front of the residual's partitions: subframe header, warm-up samples, coding method and partition order
PCM_FD uint32_t residual_base(uint32_t bps, uint32_t order) { return 8u + bps * order + 6u; }
PCM_FD uint32_t residual_base(uint32_t bps, const Decision& d, const LpcPlan& lpc) {
    return d.kind == LPC ? lpc_base(bps, d.order, lpc.precision) : residual_base(bps, d.order);
}
PCM_FD uint32_t subframe_byte(const Decision& d) {
    return d.kind == CONSTANT ? 0u : d.kind == VERBATIM ? 2u : d.kind == FIXED ? (8u | d.order) << 1 : (0x20u | (d.order - 1u)) << 1;
}
// the residual's partitions of a FIXED or LPC subframe, the lane's part
template <class Res, class Or>
PCM_FD void lane_emit_residual(const Work& w, uint32_t* image, const Shape& s, uint32_t bits, uint32_t bps, const Decision& d, uint32_t lane, uint32_t start, Res res, Or orw) {
    uint32_t b, e;
    lane_run(s, lane, b, e);
    if (b < d.order) b = d.order < e ? d.order : e;
    const uint32_t span = kThreads >> d.porder, code = w.param[decision_row(d)][node_slot(d.porder, lane / span)];
    uint32_t pos = residual_base(bps, d, w.lpc) + start;
    if (lane % span == 0u) {
        const uint32_t pb = param_bits(bits);
        if (code & kEscape) { put_bits(image, pos, pb, 0xFFFFFFFFu, orw); put_bits(image, pos + pb, 5u, code & 31u, orw); pos += pb + 5u; }
        else { put_bits(image, pos, pb, code, orw); pos += pb; }
    }
    for (uint32_t i = b; i < e; ++i) {
        const int32_t r = res(i);
        const uint32_t u = zigzag(r);
        if (code & kEscape) { put_bits(image, pos, code & 31u, (uint32_t)r, orw); pos += code & 31u; continue; }
        const uint32_t q = u >> code;                   // q zeros are already there
        put_bits(image, pos + q, 1u, 1u, orw);
        put_bits(image, pos + q + 1u, code, u, orw);
        pos += q + 1u + code;
    }
}
// phase 4: the lane's bits into the zeroed image; `start` = the exclusive scan of lane_bits (FIXED, LPC). Lane 0 writes what stands in front.
template <class Or>
PCM_FD void lane_emit(const Work& w, uint32_t* image, const Shape& s, uint32_t bits, uint32_t bps, const Decision& d, uint32_t lane, uint32_t start, Or orw) {
    if (lane == 0u) {
        put_bits(image, 0u, 8u, subframe_byte(d), orw);
        if (d.kind == CONSTANT) put_bits(image, 8u, bps, (uint32_t)w.codes[0], orw);
        if (d.kind == FIXED || d.kind == LPC) {
            uint32_t pos = 8u;
            for (uint32_t i = 0; i < d.order; ++i, pos += bps) put_bits(image, pos, bps, (uint32_t)w.codes[i], orw);
            if (d.kind == LPC) {
                const uint32_t q = w.lpc.precision;
                put_bits(image, pos, 4u, q - 1u, orw); put_bits(image, pos + 4u, 5u, w.lpc.shift[d.slot], orw); pos += 9u;
                for (uint32_t j = 0; j < d.order; ++j, pos += q) put_bits(image, pos, q, (uint32_t)(int32_t)w.lpc.coef[d.slot][j], orw);
            }
            put_bits(image, pos, 6u, ((bits == 16u ? 0u : 1u) << 4) | d.porder, orw);
        }
    }
    if (d.kind == CONSTANT) return;
    if (d.kind == VERBATIM) {
        uint32_t b, e;
        lane_run(s, lane, b, e);
        for (uint32_t i = b; i < e; ++i) put_bits(image, 8u + bps * i, bps, (uint32_t)w.codes[i], orw);
        return;
    }
    if (d.kind == FIXED) lane_emit_residual(w, image, s, bits, bps, d, lane, start, FixedResidual{w.codes, d.order}, orw);
    else lane_emit_residual(w, image, s, bits, bps, d, lane, start, lpc_residual(w.codes, w.lpc, d.slot), orw);
}

// ---- the assemble kernel: a frame's bytes from its header and its subframes' words ------------------------------------------------------------
struct FrameParts {
    uint8_t header[kMaxHeader];
    uint32_t headerBytes, count;                 // subframes
    const uint32_t* words[kMaxChannels];
    uint64_t offset[kMaxChannels + 1];           // bit offsets of the subframes behind the header; offset[count] = their bits in all
};
PCM_FD uint32_t word_bits(const uint32_t* words, uint64_t pos, uint32_t nb) {      // nb <= 8 bits at bit pos of a word stream
    const uint32_t w = (uint32_t)(pos >> 5), sh = (uint32_t)(pos & 31u);
    uint32_t v = words[w] << sh;
    if (sh + nb > 32u) v |= words[w + 1u] >> (32u - sh);
    return v >> (32u - nb);
}
// byte i of the frame in front of its CRC-16 (header, subframes bit-contiguous, zero bits up to the byte)
PCM_FD uint8_t frame_byte(const FrameParts& f, uint32_t i) {
    if (i < f.headerBytes) return f.header[i];
    uint64_t pos = (uint64_t)(i - f.headerBytes) * 8u;
    uint32_t need = 8u, v = 0u, q = 0u;
    while (q < f.count && f.offset[q + 1u] <= pos) ++q;
    while (need && q < f.count) {
        const uint64_t avail = f.offset[q + 1u] - pos;
        const uint32_t take = avail < need ? (uint32_t)avail : need;
        v = (v << take) | word_bits(f.words[q], pos - f.offset[q], take);
        need -= take; pos += take; ++q;
    }
    return (uint8_t)(v << need);
}
// lane chunks of the CRC: `total` bytes over 256 lanes
PCM_FD uint32_t crc_chunk(uint32_t total) { return (total + kThreads - 1u) / kThreads; }
PCM_FD uint16_t lane_crc(const FrameParts& f, uint32_t total, uint32_t lane) {
    const uint32_t c = crc_chunk(total), b = lane * c < total ? lane * c : total, e = b + c < total ? b + c : total;
    if (b == e) return 0u;
    uint16_t crc = 0;
    for (uint32_t i = b; i < e; ++i) crc = crc16_update(crc, frame_byte(f, i));
    return crc16_advance(crc, total - e);
}
// 16-byte pieces of the frame's stretch [at, at + len) of its stream's buffer, as pcm_pack's stage C cuts them
PCM_FD uint32_t piece_first(uint64_t at) { return (uint32_t)(at & 15u); }

// ---- the scalar twin (host) --------------------------------------------------------------------------------------------------------------------
struct BitWriter {
    uint8_t* out; size_t cap, bytes = 0; uint32_t acc = 0, fill = 0; bool overflow = false;
    BitWriter(uint8_t* o, size_t c) : out(o), cap(c) {}
    void put(uint32_t nb, uint32_t v) {
        for (uint32_t i = nb; i > 0u; --i) {
            acc = (acc << 1) | ((v >> (i - 1u)) & 1u);
            if (++fill == 8u) { if (bytes < cap) out[bytes] = (uint8_t)acc; else overflow = true; ++bytes; acc = 0; fill = 0; }
        }
    }
    void unary(uint32_t q) { for (; q >= 32u; q -= 32u) put(32u, 0u); put(q + 1u, 1u); }
    void align() { if (fill) put(8u - fill, 0u); }
};
struct SubPlan { Decision d; uint8_t param[1u << 8]; LpcPlan lpc; };
struct HostScratch {            // what the twin needs besides the stack
    std::vector<uint64_t> sums = std::vector<uint64_t>(256 * kMaxParams);
    std::vector<uint8_t> param = std::vector<uint8_t>(kRows * kNodeSlots);
    std::vector<int32_t> cand = std::vector<int32_t>(4 * kMaxFrame);
    SubPlan plans[kMaxChannels], four[4];
    std::vector<uint32_t> windowed = std::vector<uint32_t>(kMaxFrame);
};
// one row of the pricing tables the way the tree fills it: the smallest partitions' sums, merged pairwise per partition order
template <class Res>
inline void price_row(HostScratch& hs, const Shape& sh, uint32_t bits, uint32_t row, uint32_t warm, Res res, uint32_t (*total)[kLevels], uint32_t* rootMax) {
    const uint32_t K = param_count(bits), nb = 1u << sh.pmax;
    uint64_t* sums = hs.sums.data();
    uint32_t cnt[256], mx[256];
    uint8_t (*param)[kNodeSlots] = reinterpret_cast<uint8_t (*)[kNodeSlots]>(hs.param.data());
    for (uint32_t p = 0; p < nb; ++p) {
        uint32_t c = 0, m = 0;
        for (uint32_t k = 0; k < K; ++k) sums[p * kMaxParams + k] = 0;
        for (uint32_t i = p * sh.part; i < (p + 1u) * sh.part; ++i) {
            if (i < warm) continue;
            const uint32_t u = zigzag(res(i));
            for (uint32_t k = 0; k < K; ++k) sums[p * kMaxParams + k] += u >> k;
            m = u > m ? u : m; ++c;
        }
        cnt[p] = c; mx[p] = m;
    }
    for (uint32_t L = sh.pmax + 1u; L-- > 0u;) {
        const uint32_t nodes = 1u << L, stride = nb >> L;
        for (uint32_t j = 0; j < nodes; ++j) {
            const uint32_t at = j * stride;
            if (L < sh.pmax) {
                const uint32_t half = at + stride / 2u;
                for (uint32_t k = 0; k < K; ++k) sums[at * kMaxParams + k] += sums[half * kMaxParams + k];
                cnt[at] += cnt[half]; mx[at] = mx[at] > mx[half] ? mx[at] : mx[half];
            }
            uint32_t code;
            const uint64_t* rowSums = sums + at * kMaxParams;
            total[row][L] += choose_param(bits, cnt[at], mx[at], [&](uint32_t k) { return rowSums[k]; }, &code);
            param[row][node_slot(L, j)] = (uint8_t)code;
        }
    }
    rootMax[row] = mx[0];
}
// the decision for one subframe: the FIXED orders' rows, then (lpcOrder > 0) the LPC plan from the windowed samples' lags and its rows
inline void plan_subframe(HostScratch& hs, const int32_t* s, uint32_t n, uint32_t bits, uint32_t bps, SubPlan& plan, uint32_t lpcOrder = 0u) {
    const Shape sh = shape(n);
    uint8_t (*param)[kNodeSlots] = reinterpret_cast<uint8_t (*)[kNodeSlots]>(hs.param.data());
    uint32_t total[kRows][kLevels] = {}, rootMax[kRows] = {};
    for (uint32_t o = 0; o <= max_order(n); ++o) price_row(hs, sh, bits, o, o, FixedResidual{s, o}, total, rootMax);
    if (n == 1u) rootMax[1] = 0u;
    if (lpcOrder > 0u) {
        LpcScratch ws;
        int64_t lag[kLpcLags] = {};
        for (uint32_t i = 0; i < n; ++i) hs.windowed[i] = (uint32_t)lpc_windowed(s[i], i, n);
        lpc_lags(hs.windowed.data(), n, lpcOrder, 0u, 1u, lag);
        for (uint32_t k = 0; k < kLpcLags; ++k) ws.lag[k] = lag[k];
        lpc_design(ws, lpcOrder, n, bits, plan.lpc);
        for (uint32_t i = 0; i < plan.lpc.count; ++i)
            if (plan.lpc.drop[i] == LPC_OK) price_row(hs, sh, bits, lpc_row(i), plan.lpc.order[i], lpc_residual(s, plan.lpc, i), total, rootMax);
    }
    plan.d = decide(sh, bps, total, rootMax, lpcOrder > 0u ? &plan.lpc : nullptr);
    if (plan.d.kind == FIXED || plan.d.kind == LPC)
        for (uint32_t j = 0; j < (1u << plan.d.porder); ++j) plan.param[j] = param[decision_row(plan.d)][node_slot(plan.d.porder, j)];
}
inline void write_subframe(BitWriter& bw, const int32_t* s, uint32_t n, uint32_t bits, uint32_t bps, const SubPlan& plan) {
    const Decision& d = plan.d;
    bw.put(8u, subframe_byte(d));
    if (d.kind == CONSTANT) { bw.put(bps, (uint32_t)s[0]); return; }
    if (d.kind == VERBATIM) { for (uint32_t i = 0; i < n; ++i) bw.put(bps, (uint32_t)s[i]); return; }
    for (uint32_t i = 0; i < d.order; ++i) bw.put(bps, (uint32_t)s[i]);
    const LpcResidual lpc = d.kind == LPC ? lpc_residual(s, plan.lpc, d.slot) : LpcResidual{s, nullptr, 0u, 0u};
    if (d.kind == LPC) {
        bw.put(4u, plan.lpc.precision - 1u); bw.put(5u, plan.lpc.shift[d.slot]);
        for (uint32_t j = 0; j < d.order; ++j) bw.put(plan.lpc.precision, (uint32_t)(int32_t)plan.lpc.coef[d.slot][j]);
    }
    bw.put(2u, bits == 16u ? 0u : 1u); bw.put(4u, d.porder);
    const uint32_t pb = param_bits(bits), part = n >> d.porder;
    for (uint32_t j = 0; j < (1u << d.porder); ++j) {
        const uint32_t code = plan.param[j];
        if (code & kEscape) { bw.put(pb, 0xFFFFFFFFu >> (32u - pb)); bw.put(5u, code & 31u); } else bw.put(pb, code);
        for (uint32_t i = j * part; i < (j + 1u) * part; ++i) {
            if (i < d.order) continue;
            const int32_t r = d.kind == LPC ? lpc(i) : residual(s, i, d.order);
            if (code & kEscape) { bw.put(code & 31u, (uint32_t)r); continue; }
            const uint32_t u = zigzag(r);
            bw.unary(u >> code); bw.put(code, u);
        }
    }
}
// One stream's frame: `chan[g]` points at the n codes of channel g. Returns the frame's bytes (0: `cap` is too small).
inline size_t encode_frame_host(const int32_t* const* chan, uint32_t G, uint32_t n, uint32_t ff, uint32_t bits, uint32_t rate, uint32_t number,
                                uint8_t* out, size_t cap, HostScratch& hs, uint32_t* modeOut = nullptr, uint32_t lpcOrder = 0u) {
    int32_t (*cand)[kMaxFrame] = reinterpret_cast<int32_t (*)[kMaxFrame]>(hs.cand.data());
    SubPlan* plans = hs.plans;
    const int32_t* sub[kMaxChannels];
    uint32_t bps[kMaxChannels], mode = INDEPENDENT;
    if (G == 2u) {
        SubPlan* four = hs.four;
        for (uint32_t q = 0; q < 4u; ++q) {
            for (uint32_t i = 0; i < n; ++i) cand[q][i] = candidate_sample(2u, q, chan[0][i], chan[1][i]);
            plan_subframe(hs, cand[q], n, bits, candidate_bps(2u, bits, q), four[q], lpcOrder);
        }
        mode = choose_stereo(four[0].d.bits, four[1].d.bits, four[2].d.bits, four[3].d.bits);
        for (uint32_t c = 0; c < 2u; ++c) {
            const uint32_t q = stereo_candidate(mode, c);
            sub[c] = cand[q]; bps[c] = candidate_bps(2u, bits, q); plans[c] = four[q];
        }
    } else {
        for (uint32_t c = 0; c < G; ++c) { sub[c] = chan[c]; bps[c] = bits; plan_subframe(hs, chan[c], n, bits, bits, plans[c], lpcOrder); }
    }
    if (modeOut) *modeOut = mode;
    uint8_t header[kMaxHeader];
    const uint32_t hb = header_put(n, ff, rate, G, bits, mode, number, header);
    if (cap < hb) return 0;
    memcpy(out, header, hb);
    BitWriter bw(out + hb, cap - hb);
    for (uint32_t c = 0; c < G; ++c) write_subframe(bw, sub[c], n, bits, bps[c], plans[c]);
    bw.align();
    const size_t body = hb + bw.bytes;
    if (bw.overflow || body + 2u > cap) return 0;
    uint16_t crc = 0;
    for (size_t i = 0; i < body; ++i) crc = crc16_update(crc, out[i]);
    out[body] = (uint8_t)(crc >> 8); out[body + 1u] = (uint8_t)crc;
    return body + 2u;
}
// Planar codes -> one stream's frames, back to back: `planar[g]` holds `frames` codes of channel g; whole frames of `ff`, then (with
// `flush`) the remainder as one short frame. frameBytes (may be null) receives each frame's length. Returns the bytes written, or
// (size_t)-1 where `cap` is too small; *framesOut = frames written.
inline size_t encode_host(const int32_t* const* planar, uint32_t G, size_t frames, uint32_t ff, uint32_t bits, uint32_t rate, uint32_t firstNumber,
                          bool flush, uint8_t* out, size_t cap, uint32_t* frameBytes, size_t* framesOut, uint32_t lpcOrder = 0u) {
    size_t at = 0, done = 0, count = 0;
    HostScratch hs;
    const int32_t* chan[kMaxChannels];
    while (done < frames) {
        const size_t left = frames - done;
        if (left < ff && !flush) break;
        const uint32_t n = left < ff ? (uint32_t)left : ff;
        for (uint32_t g = 0; g < G; ++g) chan[g] = planar[g] + done;
        const size_t len = encode_frame_host(chan, G, n, ff, bits, rate, firstNumber + (uint32_t)count, out + at, cap - at, hs, nullptr, lpcOrder);
        if (len == 0) return (size_t)-1;
        if (frameBytes) frameBytes[count] = (uint32_t)len;
        at += len; done += n; ++count;
    }
    if (framesOut) *framesOut = count;
    return at;
}

} // namespace flac_encode

#endif // ELEMHIP_FLAC_ENCODE_H
