// The FLAC kernels' lane schedule on the CPU: flac_encode.h's per-lane functions run lane by lane the way flac_encode.hip runs them
// (barriers become loop boundaries, the block-wide scan and the XOR reduction plain loops, atomic ORs plain ORs), and every frame is
// compared byte for byte with encode_frame_host(), the scalar twin. Prints one JSON line.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "flac_encode.h"

namespace fe = flac_encode;

struct Counters { long constant = 0, verbatim = 0, fixed[5] = {0, 0, 0, 0, 0}, escapes = 0, porderMax = 0, modes[4] = {0, 0, 0, 0}, wide = 0, narrow = 0, longUnary = 0; };
static Counters g;

// the encode kernel for one candidate: returns its bits, the words in `out`
static uint32_t emulate_subframe(fe::Work& w, const int32_t* codes, uint32_t n, uint32_t bits, uint32_t bps, std::vector<uint32_t>& out) {
    std::memcpy(w.codes, codes, n * sizeof(int32_t));
    std::memset(w.total, 0, sizeof(w.total));
    std::memset(w.rootMax, 0, sizeof(w.rootMax));
    const fe::Shape sh = fe::shape(n);
    for (uint32_t order = 0; order <= fe::max_order(n); ++order) {
        for (uint32_t lane = 0; lane < fe::kThreads; ++lane) fe::leaf(w, sh, bits, order, lane);
        for (uint32_t L = 9u; L-- > 0u;)
            for (uint32_t lane = 0; lane < fe::kThreads; ++lane) fe::tree_level(w, sh, bits, order, L, lane, fe::AddPlain{});
    }
    const fe::Decision d = fe::decide(sh, bps, w.total, w.rootMax);
    uint32_t len[fe::kThreads], start[fe::kThreads], run = 0;
    for (uint32_t lane = 0; lane < fe::kThreads; ++lane) { len[lane] = fe::lane_bits(w, sh, bits, d, lane); start[lane] = run; run += len[lane]; }
    if (d.kind == fe::FIXED && fe::residual_base(bps, d.order) + run != d.bits) return 0u;      // the counted bits are the written bits
    if (d.kind == fe::CONSTANT) ++g.constant; else if (d.kind == fe::VERBATIM) ++g.verbatim; else {
        ++g.fixed[d.order];
        if ((long)d.porder > g.porderMax) g.porderMax = d.porder;
        for (uint32_t j = 0; j < (1u << d.porder); ++j) if (w.param[d.order][fe::node_slot(d.porder, j)] & fe::kEscape) ++g.escapes;
        for (uint32_t lane = 0; lane < fe::kThreads; ++lane) if (len[lane] > 16u * 64u) ++g.longUnary;
    }
    uint32_t* image = w.sums;
    const uint32_t words = (d.bits + 31u) / 32u + 1u;
    if (words > fe::slot_words(n > 256u ? 4096u : 256u, bits) || words > fe::kMaxParams * fe::kThreads) return 0u;
    for (uint32_t i = 0; i < words; ++i) image[i] = 0u;
    for (uint32_t lane = 0; lane < fe::kThreads; ++lane) fe::lane_emit(w, image, sh, bits, bps, d, lane, start[lane], fe::OrPlain{});
    out.assign(image, image + words);
    return d.bits;
}

// the assemble kernel for one frame, stored at byte `at` of a stream buffer the way the kernel's pieces store it
static bool emulate_frame(fe::Work& w, const int32_t* const* chan, uint32_t G, uint32_t n, uint32_t ff, uint32_t bits, uint32_t rate, uint32_t number,
                          uint32_t at, std::vector<uint8_t>& frame, uint32_t* modeOut) {
    const uint32_t cands = fe::candidates(G);
    std::vector<std::vector<uint32_t>> words(cands);
    std::vector<uint32_t> sb(cands);
    std::vector<int32_t> cand(n);
    for (uint32_t q = 0; q < cands; ++q) {
        for (uint32_t i = 0; i < n; ++i) cand[i] = fe::candidate_sample(G, q, chan[G == 2u ? 0u : q][i], G == 2u ? chan[1][i] : 0);
        sb[q] = emulate_subframe(w, cand.data(), n, bits, fe::candidate_bps(G, bits, q), words[q]);
        if (sb[q] == 0u) return false;
    }
    const uint32_t mode = G == 2u ? fe::choose_stereo(sb[0], sb[1], sb[2], sb[3]) : fe::INDEPENDENT;
    *modeOut = mode;
    fe::FrameParts parts;
    parts.headerBytes = fe::header_put(n, ff, rate, G, bits, mode, number, parts.header);
    if (parts.headerBytes != fe::header_bytes(n, ff, rate, number) || parts.headerBytes > fe::kMaxHeader) return false;
    parts.count = G;
    uint64_t off = 0;
    for (uint32_t c = 0; c < G; ++c) {
        const uint32_t q = G == 2u ? fe::stereo_candidate(mode, c) : c;
        parts.words[c] = words[q].data(); parts.offset[c] = off; off += sb[q];
    }
    parts.offset[G] = off;
    const uint32_t body = parts.headerBytes + (uint32_t)((off + 7u) / 8u), len = body + 2u;
    if (len != fe::frame_bytes(parts.headerBytes, off) || len > fe::frame_bound(n, G, bits)) return false;
    uint16_t crc = 0;
    for (uint32_t lane = 0; lane < fe::kThreads; ++lane) crc ^= fe::lane_crc(parts, body, lane);
    auto byteAt = [&](uint32_t i) -> uint8_t { return i < body ? fe::frame_byte(parts, i) : i == body ? (uint8_t)(crc >> 8) : (uint8_t)crc; };
    // pieces: every byte of [at, at + len) written exactly once, nothing outside
    const uint32_t head = fe::piece_first(at), pieces = pcm_pack::piece_count(head, len);
    std::vector<uint8_t> buf(head + len + 32u, 0xEE);
    std::vector<uint8_t> hits(buf.size(), 0);
    for (uint32_t p = 0; p < pieces; ++p) {
        const uint32_t lo = 16u * p > head ? 16u * p : head, hi = 16u * p + 16u < head + len ? 16u * p + 16u : head + len;
        if (pcm_pack::piece_whole(p, head, len)) { ++g.wide; for (uint32_t o = 16u * p; o < 16u * p + 16u; ++o) { buf[o] = byteAt(o - head); ++hits[o]; } continue; }
        ++g.narrow;
        for (uint32_t o = lo; o < hi; ++o) { buf[o] = byteAt(o - head); ++hits[o]; }
    }
    for (size_t o = 0; o < buf.size(); ++o) if (hits[o] != ((o >= head && o < head + len) ? 1 : 0)) return false;
    frame.assign(buf.begin() + head, buf.begin() + head + len);
    return true;
}

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

// kinds of channel content: 0 silence, 1 DC at the most negative code, 2 ramp, 3 sine, 4 white full scale, 5 alternating full scale,
// 6 one outlier in silence, 7 a copy of the previous channel (L = R), 8 its negative, 9 its half (side/right pays)
static void fill(std::vector<int32_t>& x, const std::vector<int32_t>* prev, uint32_t kind, uint32_t n, uint32_t bits, uint32_t seed) {
    const int32_t lim = 1 << (bits - 1u);
    x.assign(n, 0);
    uint32_t s = seed * 2654435761u + 17u;
    for (uint32_t i = 0; i < n; ++i) {
        switch (kind) {
            case 1: x[i] = -lim; break;
            case 2: x[i] = (int32_t)i - (int32_t)(n / 2u); break;
            case 3: x[i] = (int32_t)std::lrint(0.5 * (lim - 1) * std::sin(6.283185307179586 * 440.0 * i / 44100.0)); break;
            case 4: x[i] = (int32_t)(lcg(s) % (uint32_t)(2 * lim)) - lim; break;
            case 5: x[i] = (i & 1u) ? lim - 1 : -lim; break;
            case 6: x[i] = i == n / 3u ? lim - 1 : 0; break;
            case 7: x[i] = prev ? (*prev)[i] : 0; break;
            case 8: { const int32_t v = prev ? -(*prev)[i] : 0; x[i] = v >= lim ? lim - 1 : v; break; }
            case 9: x[i] = prev ? (*prev)[i] >> 1 : 0; break;
            default: break;
        }
    }
}

int main() {
    long failures = 0, cases = 0;
    auto w = std::make_unique<fe::Work>();
    // ---- CRCs and their combination ----
    const char* check = "123456789";
    uint8_t c8 = 0; uint16_t c16 = 0;
    for (int i = 0; i < 9; ++i) { c8 = fe::crc8_update(c8, (uint8_t)check[i]); c16 = fe::crc16_update(c16, (uint8_t)check[i]); }
    for (uint32_t k = 0; k + 1u < fe::kCrcPowers; ++k) if (fe::crc16_power(k + 1u) != fe::crc16_mul(fe::crc16_power(k), fe::crc16_power(k))) ++failures;
    {
        uint32_t s = 99u;
        std::vector<uint8_t> msg(70000);
        for (auto& b : msg) b = (uint8_t)lcg(s);
        for (uint32_t total : {1u, 2u, 255u, 256u, 257u, 4099u, 65536u, 70000u}) {
            uint16_t whole = 0;
            for (uint32_t i = 0; i < total; ++i) whole = fe::crc16_update(whole, msg[i]);
            for (uint32_t cut : {0u, 1u, total / 3u, total - 1u, total}) {
                uint16_t a = 0, b = 0;
                for (uint32_t i = 0; i < cut; ++i) a = fe::crc16_update(a, msg[i]);
                for (uint32_t i = cut; i < total; ++i) b = fe::crc16_update(b, msg[i]);
                if ((uint16_t)(fe::crc16_advance(a, total - cut) ^ b) != whole) ++failures;
            }
        }
    }
    // ---- the frame-number coding ----
    const uint32_t numbers[7] = {0u, 127u, 128u, 2047u, 2048u, 65536u, 0x7FFFFFFFu};
    const uint32_t numberBytes[7] = {1u, 1u, 2u, 2u, 3u, 4u, 6u};
    for (int i = 0; i < 7; ++i) if (fe::utf8_bytes(numbers[i]) != numberBytes[i]) ++failures;
    // ---- frames ----
    const uint32_t shorts[5] = {0u /* = ff */, 1u, 15u, 16u, 255u};
    const uint32_t rates[4] = {44100u, 48000u, 12345u, 352800u};
    fe::HostScratch hs;
    uint32_t caseNo = 0;
    auto one = [&](uint32_t ff, uint32_t G, uint32_t bits, uint32_t n, uint32_t number, uint32_t rate, uint32_t kind0) {
        std::vector<std::vector<int32_t>> x(G);
        const int32_t* chan[fe::kMaxChannels];
        for (uint32_t c = 0; c < G; ++c) {
            const uint32_t kind = G == 2u && c == 1u && (kind0 % 4u) != 0u ? 6u + (kind0 % 4u) : (kind0 + c) % 7u;
            fill(x[c], c ? &x[c - 1u] : nullptr, kind, n, bits, caseNo * 8u + c);
            chan[c] = x[c].data();
        }
        std::vector<uint8_t> got, want(fe::frame_bound(n, G, bits));
        uint32_t mode = 0, hostMode = 0;
        const bool ok = emulate_frame(*w, chan, G, n, ff, bits, rate, number, (caseNo * 7u + 3u) % 64u, got, &mode);
        const size_t len = fe::encode_frame_host(chan, G, n, ff, bits, rate, number, want.data(), want.size(), hs, &hostMode);
        ++cases; ++caseNo;
        if (!ok || len == 0 || len != got.size() || std::memcmp(got.data(), want.data(), len) != 0 || mode != hostMode) {
            ++failures;
            std::fprintf(stderr, "mismatch ff %u G %u bits %u n %u number %u kind %u: ok %d len %zu / %zu\n", ff, G, bits, n, number, kind0, (int)ok, got.size(), len);
        }
        if (G == 2u) ++g.modes[mode];
    };
    for (uint32_t ff : {256u, 4096u})
        for (uint32_t G : {1u, 2u, 3u, 8u})
            for (uint32_t bits : {16u, 24u})
                for (uint32_t si = 0; si < 5u; ++si) {
                    const uint32_t n = shorts[si] ? shorts[si] : ff;
                    // whole frames of 4096 take the content kinds in turn, everything else all of them
                    const uint32_t kinds = n == 4096u ? 2u : 7u;
                    for (uint32_t k = 0; k < kinds; ++k) one(ff, G, bits, n, numbers[(caseNo + k) % 7u], rates[caseNo % 4u], n == 4096u ? caseNo + k : k);
                }
    for (int i = 0; i < 7; ++i) for (uint32_t n : {256u, 15u}) one(256u, 2u, 16u, n, numbers[i], 44100u, 3u);
    // an odd frame is one partition: the outlier's unary run crosses hundreds of words
    for (uint32_t bits : {16u, 24u}) one(4096u, 1u, bits, 4095u, 5u, 44100u, 6u);
    const bool ok = failures == 0;
    std::printf("{\"ok\": %s, \"failures\": %ld, \"cases\": %ld, \"crc8\": %u, \"crc16\": %u, \"constant\": %ld, \"verbatim\": %ld, "
                "\"fixed\": [%ld, %ld, %ld, %ld, %ld], \"escapes\": %ld, \"porder_max\": %ld, \"modes\": [%ld, %ld, %ld, %ld], "
                "\"wide_stores\": %ld, \"narrow_stores\": %ld, \"long_unary_lanes\": %ld}\n",
                ok ? "true" : "false", failures, cases, (unsigned)c8, (unsigned)c16, g.constant, g.verbatim, g.fixed[0], g.fixed[1], g.fixed[2], g.fixed[3],
                g.fixed[4], g.escapes, g.porderMax, g.modes[0], g.modes[1], g.modes[2], g.modes[3], g.wide, g.narrow, g.longUnary);
    return ok ? 0 : 1;
}
