// tests/native/chain_carry_host.cpp — the quad-skewed recurrence loop WITHOUT its tail (elementary_amd/csrc/chain_skew.h, island_ops.inc
// chain_loop_q) emulated on the HOST, 64 lanes in lock step, with the header's own index arithmetic. Behind the last group of a
// block no lane loads or steps any more: every lane takes the carried registers of chain_skew::state_lane(lane), the lane of
// skew 0 of its quad. Two carried registers, as the kernels have them: a one-pole's float state, z = x + p z, and an integer
// that counts the frames a lane has stepped (maxhold's counter is such a register). Checked against the plain serial loop, for
// every count 1 .. 16 and n in {64, 128, 192, 512}, three blocks in a row (the state a block ends with starts the next one):
//   every frame of every member's block is written exactly once, with the serial loop's bits;
//   no load leaves the operand's block buffer, [0, 4n - 16] bytes, in any lane, and none is issued behind the last group;
//   before the broadcast a lane of skew k is 4k frames short of the final state (what the broadcast is for);
//   after it every lane holds the serial loop's final state, both registers;
//   a mirror lane (lane >= 4 * count) holds after the broadcast the bits it held before.
//   c++ -std=c++17 -O2 -ffp-contract=off -I elementary_amd/csrc tests/native/chain_carry_host.cpp -o chain_carry_host
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

struct Stats { long loads = 0, clampedLoads = 0, stores = 0, shortLanes = 0, mirrorLanes = 0; };
struct State { float z; uint32_t at; };     // the registers a step carries

// one block of n frames for a task of `count` members; x[m], p[m]: operands; s[lane]: state in, state out
static void run_block(uint32_t n, uint32_t count, const std::vector<std::vector<float>>& x, const std::vector<float>& p,
                      std::vector<State>& s, const std::vector<State>& serial, std::vector<std::vector<float>>& out,
                      std::vector<std::vector<int>>& writes, Stats& st) {
    const uint32_t groups = n / cs::kGroup;
    const unsigned long long smask = cs::store_mask(count);
    auto load = [&](uint32_t lane, uint32_t g, uint32_t j) -> float {     // operand of step j of group g, as the lane loads it
        const uint32_t m = cs::lane_member(lane, count), k = cs::lane_skew(lane, count), q = j / cs::kQuad;
        const uint32_t off = cs::load_offset(g, q, k, n);
        st.loads++;
        CHECK(g < groups, "a load behind the last group: n %u lane %u group %u", n, lane, g);
        CHECK(off <= 4u * n - 16u && off % 16u == 0u, "n %u count %u lane %u g %u q %u: offset %u", n, count, lane, g, q, off);
        const int64_t plain = (int64_t)(64u * g + 16u * q) - 16 * (int64_t)k;
        if (plain != (int64_t)off) { st.clampedLoads++; CHECK(g == 0u && plain < 0, "only the head clamps: group %u lane %u", g, lane); }
        if (g >= 1u) {     // steady: the kernel forms VGPR bias + immediate bias, no clamp
            const int64_t steady = (int64_t)cs::load_bias(k) + (int64_t)(64u * g + 16u * q) + cs::kLoadImmBias;
            CHECK(steady == (int64_t)off && plain == (int64_t)off, "steady group %u lane %u: %lld vs %u", g, lane, (long long)steady, off);
        }
        if (off > 4u * n - 16u) return 0.0f;
        return x[m][off / 4u + j % cs::kQuad];
    };
    for (uint32_t g = 0; g < groups; ++g) {
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            const uint32_t m = cs::lane_member(lane, count), k = cs::lane_skew(lane, count);
            float y[cs::kGroup] = {};
            for (uint32_t j = 0; j < cs::kGroup; ++j) {
                const float xv = load(lane, g, j);
                if (g > 0u || cs::head_active(k, j)) { s[lane].z = xv + p[m] * s[lane].z; s[lane].at++; y[j] = s[lane].z; }
            }
            if ((smask >> lane) & 1ull) {
                const uint32_t f0 = cs::stored_frame(g, k);
                CHECK(cs::store_bias(k) + 64u * g == 4u * f0, "store offset of group %u skew %u", g, k);
                CHECK(f0 + 3u < n, "store past the block: frame %u", f0);
                st.stores++;
                for (uint32_t i = 0; i < cs::kQuad && f0 + i < n; ++i) { out[m][f0 + i] = y[cs::kGroup - cs::kQuad + i]; writes[m][f0 + i]++; }
            }
        }
    }
    // before the broadcast: skew 0 is done, skew k has 4k frames to go
    for (uint32_t lane = 0; lane < 64u; ++lane) {
        const uint32_t m = cs::lane_member(lane, count), k = cs::lane_skew(lane, count);
        CHECK(s[lane].at + cs::kQuad * k == serial[m].at, "n %u count %u lane %u: %u frames stepped, skew %u, serial %u", n, count, lane, s[lane].at, k, serial[m].at);
        if (k == 0u) CHECK(bits(s[lane].z) == bits(serial[m].z), "n %u count %u lane %u: skew 0 is not at the final state", n, count, lane);
        else st.shortLanes++;
    }
    // the broadcast: all 64 lanes at once, every register (a DPP quad permute reads the registers as they were before it)
    CHECK(cs::kStateQuadPerm == 0, "quad_perm:[0,0,0,0] reads lane 0 of the quad");
    const std::vector<State> before = s;
    for (uint32_t lane = 0; lane < 64u; ++lane) {
        const uint32_t src = cs::state_lane(lane);
        CHECK(src <= lane && lane - src < cs::kQuad && src % cs::kQuad == 0u, "state lane of %u: %u", lane, src);
        CHECK(cs::lane_member(src, count) == cs::lane_member(lane, count) && cs::lane_skew(src, count) == 0u, "lane %u takes its state from %u", lane, src);
        s[lane] = before[src];
    }
    for (uint32_t lane = 4u * count; lane < 64u; ++lane) {
        st.mirrorLanes++;
        CHECK(bits(s[lane].z) == bits(before[lane].z) && s[lane].at == before[lane].at, "n %u count %u mirror lane %u changed", n, count, lane);
    }
}

static void one_case(uint32_t n, uint32_t count, std::mt19937& rng, Stats& st) {
    std::uniform_real_distribution<float> ux(-1.0f, 1.0f), up(-0.98f, 0.98f);
    CHECK(cs::applies(count), "count %u", count);
    std::vector<float> p(count);
    std::vector<State> serial(count), s(64);
    for (uint32_t m = 0; m < count; ++m) { p[m] = up(rng); serial[m].z = ux(rng); serial[m].at = 0u; }
    for (uint32_t lane = 0; lane < 64u; ++lane) s[lane] = serial[cs::lane_member(lane, count)];
    for (int block = 0; block < 3; ++block) {
        std::vector<std::vector<float>> x(count, std::vector<float>(n)), out(count, std::vector<float>(n, -7.0f)), ref(count, std::vector<float>(n));
        std::vector<std::vector<int>> writes(count, std::vector<int>(n, 0));
        for (uint32_t m = 0; m < count; ++m) for (uint32_t t = 0; t < n; ++t) x[m][t] = ux(rng);
        for (uint32_t m = 0; m < count; ++m)
            for (uint32_t t = 0; t < n; ++t) { serial[m].z = x[m][t] + p[m] * serial[m].z; serial[m].at++; ref[m][t] = serial[m].z; }
        run_block(n, count, x, p, s, serial, out, writes, st);
        for (uint32_t m = 0; m < count; ++m)
            for (uint32_t t = 0; t < n; ++t) {
                CHECK(writes[m][t] == 1, "n %u count %u member %u frame %u written %d times", n, count, m, t, writes[m][t]);
                CHECK(bits(out[m][t]) == bits(ref[m][t]), "n %u count %u member %u frame %u: %08x vs %08x", n, count, m, t, bits(out[m][t]), bits(ref[m][t]));
            }
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            const State& want = serial[cs::lane_member(lane, count)];
            CHECK(bits(s[lane].z) == bits(want.z) && s[lane].at == want.at, "n %u count %u block %d lane %u: final state", n, count, block, lane);
        }
    }
}

int main() {
    std::mt19937 rng(20260801u);
    Stats st;
    int cases = 0;
    const uint32_t ns[] = {64u, 128u, 192u, 512u};
    for (uint32_t n : ns) for (uint32_t c = 1u; c <= cs::kMaxCount; ++c) { one_case(n, c, rng, st); ++cases; }
    for (uint32_t j = 0; j < cs::kTailSteps; ++j) CHECK(!cs::tail_active(0u, j), "skew 0 had no tail step %u", j);
    std::printf("{\"ok\": %s, \"cases\": %d, \"loads\": %ld, \"clamped_loads\": %ld, \"stores\": %ld, \"short_lanes\": %ld, \"mirror_lanes\": %ld, \"failures\": %d}\n",
                failures ? "false" : "true", cases, st.loads, st.clampedLoads, st.stores, st.shortLanes, st.mirrorLanes, failures);
    return failures ? 1 : 0;
}
