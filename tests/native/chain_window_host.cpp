// tests/native/chain_window_host.cpp — the store windows of the quad-skewed recurrence loop (elementary_amd/csrc/chain_skew.h,
// island_ops.inc chain_loop_q) emulated on the HOST, 64 lanes in lock step, with the header's own index arithmetic: a lane keeps its
// piece of W consecutive groups and the group that closes the window issues the W stores under one EXEC switch. A one-pole,
// z = x + p z, rendered span by span exactly as the loop is written out, for every window size that fits the span's depth; W = 1 is
// the unwindowed schedule and the reference for the others:
//   every frame of every member's block is stored exactly once, with the bytes (and at the byte offset) the unwindowed schedule stores;
//   no store of a window is issued before the steps of the window's last group have run;
//   no window holds groups of two spans, its immediates stay below 4096 and its stores share the span's scalar offset;
//   the last window of a block closes with the block's last group: nothing is left open for the state hand-over;
//   the window the kernel takes (chain_skew::window) fits every depth the loops are instantiated with.
//   c++ -std=c++17 -O2 -ffp-contract=off -I elementary_amd/csrc tests/native/chain_window_host.cpp -o chain_window_host
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "chain_skew.h"

namespace cs = chain_skew;

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::fprintf(stderr, "FAILED %s: ", #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } } while (0)

struct Stats { long stores = 0, switches = 0, windows = 0; };
struct Piece { float v[cs::kQuad]; };

// One block of n frames, `count` members, spans of `depth` groups, windows of w groups. out[m]: the member's block buffer as BYTES
// (4n), writes[m][frame]: how often a frame was stored.
static void run_block(uint32_t n, uint32_t count, uint32_t depth, uint32_t w, const std::vector<std::vector<float>>& x, const std::vector<float>& p,
                      std::vector<float>& z, std::vector<std::vector<unsigned char>>& out, std::vector<std::vector<int>>& writes, Stats& st) {
    const uint32_t groups = n / cs::kGroup, spans = groups / depth;
    const unsigned long long smask = cs::store_mask(count);
    std::vector<std::vector<Piece>> held(w, std::vector<Piece>(64));     // held[i][lane]: the piece of the window's i-th group
    std::vector<int64_t> heldGroup(w, -1);                                // ... and which group of the block it belongs to
    uint32_t open = 0;                                                    // groups in the open window
    uint32_t stepped = 0;                                                 // groups whose 16 steps every lane has run
    for (uint32_t s = 0; s < spans; ++s) {
        const uint32_t soff = s * depth * cs::kGroup * 4u;                // the span's scalar byte offset
        for (uint32_t d = 0; d < depth; ++d) {
            const uint32_t g = s * depth + d;
            for (uint32_t lane = 0; lane < 64u; ++lane) {
                const uint32_t m = cs::lane_member(lane, count), k = cs::lane_skew(lane, count);
                float y[cs::kGroup] = {};
                for (uint32_t j = 0; j < cs::kGroup; ++j) {
                    const float xv = x[m][cs::load_offset(g, j / cs::kQuad, k, n) / 4u + j % cs::kQuad];
                    if (g > 0u || cs::head_active(k, j)) { z[lane] = xv + p[m] * z[lane]; y[j] = z[lane]; }
                }
                for (uint32_t i = 0; i < cs::kQuad; ++i) held[d % w][lane].v[i] = y[cs::kGroup - cs::kQuad + i];
            }
            heldGroup[d % w] = g;
            ++open; ++stepped;
            if (!cs::window_closes(d, w)) continue;
            // the closing group's one statement: EXEC saved, narrowed, w stores, EXEC restored
            const uint32_t d0 = cs::window_first(d, w);
            CHECK(open == w, "n %u depth %u w %u span %u group %u: the window holds %u groups", n, depth, w, s, d, open);
            CHECK(d0 <= d && d - d0 + 1u == w && d < depth, "n %u depth %u w %u: window [%u, %u] leaves the span", n, depth, w, d0, d);
            st.switches++; st.windows++;
            for (uint32_t i = 0; i < w; ++i) {
                const uint32_t gi = s * depth + d0 + i, imm = (d0 + i) * cs::kGroup * 4u;
                CHECK(heldGroup[i] == (int64_t)gi, "n %u depth %u w %u: slot %u holds group %lld, not %u", n, depth, w, i, (long long)heldGroup[i], gi);
                CHECK(gi < stepped, "n %u depth %u w %u: group %u stored before its steps", n, depth, w, gi);
                CHECK(s * depth + d < stepped, "n %u depth %u w %u: window stored before its last group's steps", n, depth, w);
                CHECK(gi / depth == s, "n %u depth %u w %u: group %u of span %u stored with span %u's offset", n, depth, w, gi, gi / depth, s);
                CHECK(imm + cs::store_bias(0u) < 4096u, "n %u depth %u w %u: immediate %u", n, depth, w, imm);
                st.stores++;
                for (uint32_t lane = 0; lane < 64u; ++lane) {
                    if (!((smask >> lane) & 1ull)) continue;
                    const uint32_t m = cs::lane_member(lane, count), k = cs::lane_skew(lane, count);
                    const uint32_t at = soff + imm + cs::store_bias(k);          // scalar offset + immediate + the lane's VGPR bias
                    CHECK(at == 4u * cs::stored_frame(gi, k) && at + 16u <= 4u * n, "n %u w %u lane %u group %u: byte offset %u", n, w, lane, gi, at);
                    if (at + 16u > 4u * n) continue;
                    std::memcpy(&out[m][at], held[i][lane].v, 16);
                    for (uint32_t f = 0; f < cs::kQuad; ++f) writes[m][at / 4u + f]++;
                }
                heldGroup[i] = -1;
            }
            open = 0;
        }
        CHECK(open == 0u, "n %u depth %u w %u: span %u ends with %u groups held", n, depth, w, s, open);
    }
    CHECK(open == 0u && stepped == groups, "n %u depth %u w %u: the block ends with %u groups held", n, depth, w, open);
    for (uint32_t lane = 0; lane < 64u; ++lane) z[lane] = z[cs::state_lane(lane)];      // the state hand-over, behind every store
}

static void one_case(uint32_t n, uint32_t count, uint32_t depth, std::mt19937& rng, Stats& st, int& cases) {
    std::uniform_real_distribution<float> ux(-1.0f, 1.0f), up(-0.98f, 0.98f);
    std::vector<float> p(count), zs0(count);
    for (uint32_t m = 0; m < count; ++m) { p[m] = up(rng); zs0[m] = ux(rng); }
    std::vector<std::vector<std::vector<float>>> x(2, std::vector<std::vector<float>>(count, std::vector<float>(n)));
    for (auto& xb : x) for (auto& xm : xb) for (float& v : xm) v = ux(rng);
    std::vector<std::vector<std::vector<unsigned char>>> plain;           // what W = 1 stored, per block
    for (uint32_t w : {1u, 2u, 4u, 8u}) {
        if (!cs::window_fits(w, depth)) continue;
        ++cases;
        std::vector<float> z(64), zs = zs0;
        for (uint32_t lane = 0; lane < 64u; ++lane) z[lane] = zs[cs::lane_member(lane, count)];
        for (int block = 0; block < 2; ++block) {                          // two blocks: the state carries over
            std::vector<std::vector<unsigned char>> out(count, std::vector<unsigned char>(4u * n, 0xA5));
            std::vector<std::vector<int>> writes(count, std::vector<int>(n, 0));
            Stats before = st;
            run_block(n, count, depth, w, x[block], p, z, out, writes, st);
            CHECK(st.stores - before.stores == (long)(n / cs::kGroup) && (st.switches - before.switches) * (long)w == (long)(n / cs::kGroup),
                  "n %u depth %u w %u: %ld stores under %ld switches", n, depth, w, st.stores - before.stores, st.switches - before.switches);
            for (uint32_t m = 0; m < count; ++m)
                for (uint32_t t = 0; t < n; ++t) {
                    zs[m] = x[block][m][t] + p[m] * zs[m];
                    float got; std::memcpy(&got, &out[m][4u * t], 4);
                    CHECK(writes[m][t] == 1, "n %u count %u depth %u w %u member %u frame %u stored %d times", n, count, depth, w, m, t, writes[m][t]);
                    CHECK(bits(got) == bits(zs[m]), "n %u count %u depth %u w %u member %u frame %u: %08x vs %08x", n, count, depth, w, m, t, bits(got), bits(zs[m]));
                }
            if (w == 1u) plain.push_back(out);
            else CHECK(out == plain[(size_t)block], "n %u count %u depth %u w %u block %d: not the bytes of the unwindowed schedule", n, count, depth, w, block);
            for (uint32_t lane = 0; lane < 64u; ++lane)
                CHECK(bits(z[lane]) == bits(zs[cs::lane_member(lane, count)]), "n %u count %u depth %u w %u block %d lane %u: final state", n, count, depth, w, block, lane);
        }
    }
}

int main() {
    std::mt19937 rng(20260309u);
    Stats st;
    int cases = 0;
    const uint32_t ns[] = {64u, 128u, 192u, 512u}, counts[] = {1u, 3u, 16u};
    for (uint32_t n : ns)
        for (uint32_t c : counts)
            for (uint32_t depth : {2u, 4u, 8u})                            // the depths chain_loop_m instantiates: spans of 32, 64 and 128 frames
                if (n % (depth * cs::kGroup) == 0u) one_case(n, c, depth, rng, st, cases);
    // the windows the kernel takes: never wider than the span, always a divisor of it
    for (uint32_t depth : {2u, 4u, 8u})
        for (bool streamed : {false, true}) {
            const uint32_t w = cs::window(streamed, depth);
            CHECK(cs::window_fits(w, depth) && (w == 1u || w == 2u || w == 4u || w == 8u), "window(%d, %u) = %u", (int)streamed, depth, w);
        }
    CHECK(!cs::window_fits(0u, 4u) && !cs::window_fits(8u, 4u) && !cs::window_fits(3u, 8u) && cs::window_fits(8u, 8u), "window_fits");
    CHECK(cs::window_closes(3u, 4u) && !cs::window_closes(2u, 4u) && cs::window_closes(7u, 4u) && cs::window_first(7u, 4u) == 4u && cs::window_first(0u, 1u) == 0u, "window arithmetic");
    std::printf("{\"ok\": %s, \"cases\": %d, \"stores\": %ld, \"switches\": %ld, \"failures\": %d}\n",
                failures ? "false" : "true", cases, st.stores, st.switches, failures);
    return failures ? 1 : 0;
}
