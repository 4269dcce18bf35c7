// The LPC path of the FLAC encode kernel on the CPU: the per-lane functions of flac_lpc.h and flac_encode.h run lane by lane the way
// elemhip_flac_encode<true> runs them (windowed samples, strided lags reduced over the lanes, one lane's design, leaf / tree per priced
// order, the extended decision, the scan, the bits), and every frame is compared byte for byte with encode_frame_host(..., lpcOrder),
// the scalar twin. Counts what occurred; prints one JSON line.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "flac_encode.h"

namespace fe = flac_encode;

struct Counters {
    long constant = 0, verbatim = 0, fixed = 0, lpcSlot[2] = {0, 0}, lpcOrderSeen[13] = {}, drop[4] = {0, 0, 0, 0}, overflow = 0, fixedBeatsLpc = 0;
    long lpcEscapes = 0, designDrop[4] = {0, 0, 0, 0}, modes[4] = {0, 0, 0, 0}, longest = 0, subframes = 0, forcedOverflow = 0;
};
static Counters g;

// the encode kernel with an LPC order for one candidate: returns its bits, the words in `out`
static uint32_t emulate_subframe(fe::Work& w, const int32_t* codes, uint32_t n, uint32_t ff, uint32_t bits, uint32_t bps, uint32_t P, std::vector<uint32_t>& out) {
    std::memcpy(w.codes, codes, n * sizeof(int32_t));
    std::memset(w.total, 0, sizeof(w.total));
    std::memset(w.rootMax, 0, sizeof(w.rootMax));
    const fe::Shape sh = fe::shape(n);
    for (uint32_t order = 0; order <= fe::max_order(n); ++order) {
        for (uint32_t lane = 0; lane < fe::kThreads; ++lane) fe::leaf(w, sh, bits, order, lane);
        for (uint32_t L = 9u; L-- > 0u;)
            for (uint32_t lane = 0; lane < fe::kThreads; ++lane) fe::tree_level(w, sh, bits, order, L, lane, fe::AddPlain{});
    }
    // lpc_prepare: the windowed samples, every lane's strided partial lags, their sum in an order of its own (from the last lane down)
    for (uint32_t lane = 0; lane < fe::kThreads; ++lane)
        for (uint32_t i = lane; i < n; i += fe::kThreads) w.sums[i] = (uint32_t)fe::lpc_windowed(w.codes[i], i, n);
    int64_t lag[fe::kLpcLags] = {};
    for (uint32_t lane = fe::kThreads; lane-- > 0u;) {
        int64_t acc[fe::kLpcLags] = {};
        fe::lpc_lags(w.sums, n, P, lane, fe::kThreads, acc);
        for (uint32_t k = 0; k < fe::kLpcLags; ++k) lag[k] += acc[k];
    }
    for (uint32_t k = 0; k < fe::kLpcLags; ++k) w.lpcWork.lag[k] = lag[k];
    fe::lpc_design(w.lpcWork, P, n, bits, w.lpc);
    for (uint32_t slot = 0; slot < w.lpc.count; ++slot) {
        if (w.lpc.drop[slot] != fe::LPC_OK) continue;
        for (uint32_t lane = 0; lane < fe::kThreads; ++lane) fe::leaf_lpc(w, sh, bits, slot, lane);
        for (uint32_t L = 9u; L-- > 0u;)
            for (uint32_t lane = 0; lane < fe::kThreads; ++lane) fe::tree_level(w, sh, bits, fe::lpc_row(slot), L, lane, fe::AddPlain{});
    }
    const fe::Decision d = fe::decide(sh, bps, w.total, w.rootMax, &w.lpc);
    uint32_t len[fe::kThreads], start[fe::kThreads], run = 0;
    for (uint32_t lane = 0; lane < fe::kThreads; ++lane) { len[lane] = fe::lane_bits(w, sh, bits, d, lane); start[lane] = run; run += len[lane]; }
    if ((d.kind == fe::FIXED || d.kind == fe::LPC) && fe::residual_base(bps, d, w.lpc) + run != d.bits) return 0u;      // the counted bits are the written bits
    if (d.bits > 8u + bps * n) return 0u;                                 // never longer than the VERBATIM form: the slots and the bounds stand
    // what occurred
    ++g.subframes;
    bool lpcValid = false;
    for (uint32_t slot = 0; slot < w.lpc.count; ++slot) {
        if (w.lpc.order[slot] >= n || w.lpc.order[slot] == 0u || w.lpc.order[slot] > P) return 0u;
        if (w.lpc.drop[slot] != fe::LPC_OK) { ++g.drop[w.lpc.drop[slot]]; continue; }
        if (w.rootMax[fe::lpc_row(slot)] == fe::kLpcOverflow) { ++g.overflow; continue; }
        lpcValid = true;
    }
    if (d.kind == fe::CONSTANT) ++g.constant; else if (d.kind == fe::VERBATIM) ++g.verbatim; else if (d.kind == fe::FIXED) { ++g.fixed; if (lpcValid) ++g.fixedBeatsLpc; } else {
        ++g.lpcSlot[w.lpc.count == 2u ? d.slot : 1u]; ++g.lpcOrderSeen[d.order];
        if (w.lpc.count == 2u && d.slot == 0u && d.order != (P + 1u) / 2u) return 0u;
        for (uint32_t j = 0; j < (1u << d.porder); ++j) if (w.param[fe::decision_row(d)][fe::node_slot(d.porder, j)] & fe::kEscape) ++g.lpcEscapes;
    }
    uint32_t* image = w.sums;
    const uint32_t words = (d.bits + 31u) / 32u + 1u;
    if (words > fe::slot_words(ff, bits) || words > fe::kMaxParams * fe::kThreads) return 0u;
    for (uint32_t i = 0; i < words; ++i) image[i] = 0u;
    for (uint32_t lane = 0; lane < fe::kThreads; ++lane) fe::lane_emit(w, image, sh, bits, bps, d, lane, start[lane], fe::OrPlain{});
    out.assign(image, image + words);
    return d.bits;
}

// the assemble kernel for one frame (its stores are flac_encode_host.cpp's matter)
static bool emulate_frame(fe::Work& w, const int32_t* const* chan, uint32_t G, uint32_t n, uint32_t ff, uint32_t bits, uint32_t rate, uint32_t number, uint32_t P,
                          std::vector<uint8_t>& frame, uint32_t* modeOut) {
    const uint32_t cands = fe::candidates(G);
    std::vector<std::vector<uint32_t>> words(cands);
    std::vector<uint32_t> sb(cands);
    std::vector<int32_t> cand(n);
    for (uint32_t q = 0; q < cands; ++q) {
        for (uint32_t i = 0; i < n; ++i) cand[i] = fe::candidate_sample(G, q, chan[G == 2u ? 0u : q][i], G == 2u ? chan[1][i] : 0);
        sb[q] = emulate_subframe(w, cand.data(), n, ff, bits, fe::candidate_bps(G, bits, q), P, words[q]);
        if (sb[q] == 0u) return false;
    }
    const uint32_t mode = G == 2u ? fe::choose_stereo(sb[0], sb[1], sb[2], sb[3]) : fe::INDEPENDENT;
    *modeOut = mode;
    fe::FrameParts parts;
    parts.headerBytes = fe::header_put(n, ff, rate, G, bits, mode, number, parts.header);
    parts.count = G;
    uint64_t off = 0;
    for (uint32_t c = 0; c < G; ++c) {
        const uint32_t q = G == 2u ? fe::stereo_candidate(mode, c) : c;
        parts.words[c] = words[q].data(); parts.offset[c] = off; off += sb[q];
    }
    parts.offset[G] = off;
    const uint32_t body = parts.headerBytes + (uint32_t)((off + 7u) / 8u), len = body + 2u;
    if (len != fe::frame_bytes(parts.headerBytes, off) || len > fe::frame_bound(n, G, bits)) return false;
    if ((long)len > g.longest) g.longest = len;
    uint16_t crc = 0;
    for (uint32_t lane = 0; lane < fe::kThreads; ++lane) crc ^= fe::lane_crc(parts, body, lane);
    frame.resize(len);
    for (uint32_t i = 0; i < body; ++i) frame[i] = fe::frame_byte(parts, i);
    frame[body] = (uint8_t)(crc >> 8); frame[body + 1u] = (uint8_t)crc;
    return true;
}

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

// kinds of channel content: 0 silence, 1 DC at the most negative code, 2 ramp, 3 sine 440 Hz, 4 white full scale, 5 alternating full
// scale, 6 one outlier in silence, 7 bright (5 kHz + 9 kHz + noise 60 dB below), 8 codes 0 and 1 in turn (every windowed sample is 0),
// 9 a slow full-scale sine (coefficients near the binomial ones), 10 the slow sine with alternating full scale over its last 24 samples,
// 11 bright with one full-scale outlier (an escape partition), 12 the mirror of the previous channel (-1 - x: the side needs all its bits)
constexpr uint32_t kKinds = 12;
static void fill(std::vector<int32_t>& x, const std::vector<int32_t>* prev, uint32_t kind, uint32_t n, uint32_t bits, uint32_t seed) {
    const int32_t lim = 1 << (bits - 1u);
    const double pi2 = 6.283185307179586;
    x.assign(n, 0);
    uint32_t s = seed * 2654435761u + 17u;
    for (uint32_t i = 0; i < n; ++i) {
        const double bright = 0.3 * std::sin(pi2 * 5000.0 * i / 44100.0) + 0.2 * std::sin(pi2 * 9000.0 * i / 44100.0) + 0.001 * (((double)(lcg(s) & 0xFFFFu) / 32768.0) - 1.0);
        const double slow = 0.999 * std::sin(pi2 * 60.0 * (i + 40.0) / 44100.0);
        switch (kind) {
            case 1: x[i] = -lim; break;
            case 2: x[i] = (int32_t)i - (int32_t)(n / 2u); break;
            case 3: x[i] = (int32_t)std::lrint(0.5 * (lim - 1) * std::sin(pi2 * 440.0 * i / 44100.0)); break;
            case 4: x[i] = (int32_t)(lcg(s) % (uint32_t)(2 * lim)) - lim; break;
            case 5: x[i] = (i & 1u) ? lim - 1 : -lim; break;
            case 6: x[i] = i == n / 3u ? lim - 1 : 0; break;
            case 7: x[i] = (int32_t)std::lrint((lim - 1) * bright); break;
            case 8: x[i] = (int32_t)(i & 1u); break;
            case 9: x[i] = (int32_t)std::lrint((lim - 1) * slow); break;
            case 10: x[i] = i + 24u >= n ? ((i & 1u) ? lim - 1 : -lim) : (int32_t)std::lrint((lim - 1) * slow); break;
            case 11: x[i] = i == n / 2u + 5u ? lim - 1 : (int32_t)std::lrint((lim - 1) * bright); break;
            case 12: x[i] = prev ? -1 - (*prev)[i] : 0; break;
            default: break;
        }
    }
}

int main() {
    long failures = 0, cases = 0;
    auto w = std::make_unique<fe::Work>();
    fe::HostScratch hs;
    uint32_t caseNo = 0;
    // ---- the rules on their own ----
    static_assert(fe::lpc_orders(12u, 4096u).count == 2u && fe::lpc_orders(12u, 4096u).order[0] == 6u && fe::lpc_orders(12u, 4096u).order[1] == 12u, "P and ceil(P / 2)");
    static_assert(fe::lpc_orders(1u, 256u).count == 1u && fe::lpc_orders(1u, 256u).order[0] == 1u, "P = 1 is its own half");
    static_assert(fe::lpc_orders(8u, 8u).count == 1u && fe::lpc_orders(8u, 8u).order[0] == 4u && fe::lpc_orders(8u, 4u).count == 0u && fe::lpc_orders(0u, 256u).count == 0u, "order < n");
    static_assert(fe::lpc_precision(16u, 4096u) == 12u && fe::lpc_precision(24u, 4096u) == 14u && fe::lpc_precision(24u, 1u) == 9u, "precision");
    for (uint32_t n : {1u, 2u, 15u, 255u, 256u, 4096u})
        for (uint32_t i = 0; i < n; ++i) {      // the window's rational form, as the issue states it
            const int64_t d = (int64_t)(n + 1u) * (n + 1u), c = 2 * (int64_t)i - (int64_t)n + 1;
            if (fe::lpc_window(i, n) != (int32_t)((32767 * (d - c * c)) / d) || fe::lpc_window(i, n) < 0 || fe::lpc_window(i, n) > 32767) ++failures;
        }
    {   // the design on lags no windowed signal gives: each reason to drop an order, and the conversion of lags beyond 2^53
        fe::LpcScratch ws; fe::LpcPlan plan;
        auto design = [&](std::initializer_list<int64_t> lags, uint32_t P, uint32_t n, uint32_t bits) {
            std::memset(&ws, 0, sizeof(ws)); uint32_t k = 0; for (int64_t v : lags) ws.lag[k++] = v;
            fe::lpc_design(ws, P, n, bits, plan);
            for (uint32_t i = 0; i < plan.count; ++i) ++g.designDrop[plan.drop[i]];
        };
        design({0, 0, 0}, 2u, 256u, 16u); if (plan.drop[0] != fe::LPC_ZERO_LAG || plan.drop[1] != fe::LPC_ZERO_LAG) ++failures;
        design({4, 4, 4}, 2u, 256u, 16u); if (plan.drop[0] != fe::LPC_ERROR || plan.drop[1] != fe::LPC_ERROR) ++failures;       // reflection 1: the error is 0
        design({4, 2, 4}, 2u, 256u, 16u); if (plan.drop[0] != fe::LPC_OK || plan.drop[1] != fe::LPC_ERROR) ++failures;          // order 1 stands, order 2 does not
        design({(int64_t)1 << 60, (int64_t)1 << 59}, 1u, 100u, 16u);                                                                // 0.5 -> 32 / 2^6
        if (plan.drop[0] != fe::LPC_OK || plan.coef[0][0] != 32 || plan.shift[0] != 6u) ++failures;
        design({1 << 20, -(1 << 19)}, 1u, 4096u, 24u); if (plan.drop[0] != fe::LPC_OK || plan.coef[0][0] != -4096 || plan.shift[0] != 13u) ++failures;
        const double big[2] = {-300.0, 1.5}; int16_t q[3]; uint32_t sh = 0;
        if (fe::lpc_quantise(big, 2u, 7u, q, &sh) != fe::LPC_SHIFT) ++failures; else ++g.designDrop[fe::LPC_SHIFT];                                                    // 300 needs 9 bits in front of the point
        const double half[3] = {0.5, -0.25, 0.126};                                                                              // e = 0: shift q - 1
        if (fe::lpc_quantise(half, 3u, 7u, q, &sh) != fe::LPC_OK || sh != 6u || q[0] != 32 || q[1] != -16 || q[2] != 8) ++failures;
        const double tiny[1] = {1e-9};
        if (fe::lpc_quantise(tiny, 1u, 12u, q, &sh) != fe::LPC_OK || sh != 15u || q[0] != 0) ++failures;
    }
    {   // the residual that leaves int32, on the side of the +-full-scale alternating 24-bit pair (+-(2^24 - 1)) under a plan put here by
        // hand: coefficient -8192 with shift 13 predicts the side exactly and wins; with shift 0 the residual has 38 bits, the marker
        // reaches the root through the lanes' tree and through the twin's rows alike, and the decision passes the candidate over
        const uint32_t n = 256u, bits = 24u, bps = 25u;
        std::vector<int32_t> side(n);
        for (uint32_t i = 0; i < n; ++i) side[i] = (i & 1u) ? (1 << 24) - 1 : -((1 << 24) - 1);
        const fe::Shape sh = fe::shape(n);
        for (uint32_t shift : {13u, 0u}) {
            std::memcpy(w->codes, side.data(), n * sizeof(int32_t));
            std::memset(w->total, 0, sizeof(w->total)); std::memset(w->rootMax, 0, sizeof(w->rootMax));
            uint32_t total[fe::kRows][fe::kLevels] = {}, rootMax[fe::kRows] = {};
            for (uint32_t order = 0; order <= fe::kMaxOrder; ++order) {
                for (uint32_t lane = 0; lane < fe::kThreads; ++lane) fe::leaf(*w, sh, bits, order, lane);
                for (uint32_t L = 9u; L-- > 0u;) for (uint32_t lane = 0; lane < fe::kThreads; ++lane) fe::tree_level(*w, sh, bits, order, L, lane, fe::AddPlain{});
                fe::price_row(hs, sh, bits, order, order, fe::FixedResidual{side.data(), order}, total, rootMax);
            }
            w->lpc = fe::LpcPlan{1u, 14u, {1u, 0u}, {shift, 0u}, {fe::LPC_OK, fe::LPC_OK}, {{-8192}, {0}}};
            for (uint32_t lane = 0; lane < fe::kThreads; ++lane) fe::leaf_lpc(*w, sh, bits, 0u, lane);
            for (uint32_t L = 9u; L-- > 0u;) for (uint32_t lane = 0; lane < fe::kThreads; ++lane) fe::tree_level(*w, sh, bits, fe::lpc_row(0u), L, lane, fe::AddPlain{});
            fe::price_row(hs, sh, bits, fe::lpc_row(0u), 1u, fe::lpc_residual(side.data(), w->lpc, 0u), total, rootMax);
            const fe::Decision lanes = fe::decide(sh, bps, w->total, w->rootMax, &w->lpc), twin = fe::decide(sh, bps, total, rootMax, &w->lpc);
            if (std::memcmp(total, w->total, sizeof(total)) != 0 || std::memcmp(rootMax, w->rootMax, sizeof(rootMax)) != 0) ++failures;
            if (lanes.kind != twin.kind || lanes.bits != twin.bits) ++failures;
            if (shift == 13u && (lanes.kind != fe::LPC || rootMax[fe::lpc_row(0u)] != 0u)) ++failures;
            if (shift == 0u) { if (lanes.kind == fe::LPC || rootMax[fe::lpc_row(0u)] != fe::kLpcOverflow) ++failures; else ++g.forcedOverflow; }
        }
    }
    // ---- frames ----
    auto one = [&](uint32_t ff, uint32_t G, uint32_t bits, uint32_t n, uint32_t P, uint32_t kind0, bool mirror) {
        std::vector<std::vector<int32_t>> x(G);
        const int32_t* chan[fe::kMaxChannels];
        for (uint32_t c = 0; c < G; ++c) {
            const uint32_t kind = mirror && c == 1u ? 12u : (kind0 + 5u * c) % kKinds;
            fill(x[c], c ? &x[c - 1u] : nullptr, kind, n, bits, caseNo * 8u + c);
            chan[c] = x[c].data();
        }
        std::vector<uint8_t> got, want(fe::frame_bound(n, G, bits));
        uint32_t mode = 0, hostMode = 0;
        const bool ok = emulate_frame(*w, chan, G, n, ff, bits, 44100u, caseNo, P, got, &mode);
        const size_t len = fe::encode_frame_host(chan, G, n, ff, bits, 44100u, caseNo, want.data(), want.size(), hs, &hostMode, P);
        ++cases; ++caseNo;
        if (!ok || len == 0 || len != got.size() || std::memcmp(got.data(), want.data(), len) != 0 || mode != hostMode) {
            ++failures;
            std::fprintf(stderr, "mismatch ff %u G %u bits %u n %u P %u kind %u: ok %d len %zu / %zu\n", ff, G, bits, n, P, kind0, (int)ok, got.size(), len);
        }
        if (G == 2u) ++g.modes[mode];
    };
    for (uint32_t ff : {256u, 4096u})
        for (uint32_t G : {1u, 2u, 3u, 8u})
            for (uint32_t bits : {16u, 24u})
                for (uint32_t P : {1u, 8u, 12u}) {
                    const uint32_t ns[7] = {ff, 1u, 2u, P, P + 1u, 15u, 255u};
                    for (uint32_t n : ns) {
                        // whole frames of 4096 take three content kinds in turn, everything else all of them (G channels at a time)
                        const uint32_t kinds = n == 4096u ? 3u : kKinds;
                        for (uint32_t k = 0; k < kinds; k += n == 4096u ? 1u : (G > 2u ? 3u : 1u)) one(ff, G, bits, n, P, n == 4096u ? caseNo + k : k, false);
                    }
                }
    // the +-full-scale alternating pair and its mirror: mid is -1 throughout, the side +-(2^bits - 1); and the slow sine that ends in it
    for (uint32_t bits : {16u, 24u})
        for (uint32_t P : {1u, 8u, 12u})
            for (uint32_t n : {256u, 4096u, 255u}) { one(n == 255u ? 256u : n, 2u, bits, n, P, 5u, true); one(n == 255u ? 256u : n, 2u, bits, n, P, 10u, true); }
    // equal samples stay CONSTANT whatever the order
    {
        const long before = g.constant, subs = g.subframes;
        for (uint32_t P : {1u, 8u, 12u}) one(256u, 1u, 16u, 256u, P, 1u, false);
        if (g.constant - before != 3 || g.subframes - subs != 3) ++failures;
    }
    const bool ok = failures == 0;
    std::printf("{\"ok\": %s, \"failures\": %ld, \"cases\": %ld, \"subframes\": %ld, \"constant\": %ld, \"verbatim\": %ld, \"fixed\": %ld, \"lpc_half_order\": %ld, "
                "\"lpc_full_order\": %ld, \"lpc_orders\": [%ld, %ld, %ld, %ld, %ld, %ld], \"drop_zero_lag\": %ld, \"drop_error\": %ld, \"drop_shift\": %ld, "
                "\"drop_overflow\": %ld, \"design_drops\": [%ld, %ld, %ld, %ld], \"forced_overflow\": %ld, \"fixed_beats_lpc\": %ld, \"lpc_escapes\": %ld, \"modes\": [%ld, %ld, %ld, %ld], "
                "\"longest_frame\": %ld}\n",
                ok ? "true" : "false", failures, cases, g.subframes, g.constant, g.verbatim, g.fixed, g.lpcSlot[0], g.lpcSlot[1], g.lpcOrderSeen[1], g.lpcOrderSeen[4],
                g.lpcOrderSeen[6], g.lpcOrderSeen[8], g.lpcOrderSeen[12], g.lpcOrderSeen[2] + g.lpcOrderSeen[3] + g.lpcOrderSeen[5] + g.lpcOrderSeen[7], g.drop[fe::LPC_ZERO_LAG],
                g.drop[fe::LPC_ERROR], g.drop[fe::LPC_SHIFT], g.overflow, g.designDrop[0], g.designDrop[1], g.designDrop[2], g.designDrop[3], g.forcedOverflow, g.fixedBeatsLpc, g.lpcEscapes,
                g.modes[0], g.modes[1], g.modes[2], g.modes[3], g.longest);
    return ok ? 0 : 1;
}
