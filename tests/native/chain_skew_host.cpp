// tests/native/chain_skew_host.cpp — the quad-skewed recurrence loop of the specialised kernels (elementary_amd/csrc/chain_skew.h,
// island_ops.inc chain_loop_q) emulated on the HOST, 64 lanes in lock step, with the header's own index arithmetic: which frames a
// lane steps, loads and stores, and where. Checked against the plain serial loop of a one-pole, z = x + p z:
//   every frame of every member's block is written exactly once, with the serial loop's bits;
//   every lane of a member ends the block with the serial loop's final state (two blocks in a row: the state carries over);
//   no load leaves the operand's block buffer, [0, 4n - 16] bytes, in any lane, mirror lanes included;
//   the steady groups' unclamped address (VGPR bias + immediate bias) is the clamped one;
//   a task of 17 members is refused.
//   c++ -std=c++17 -O2 -ffp-contract=off -I elementary_amd/csrc tests/native/chain_skew_host.cpp -o chain_skew_host
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

struct Stats { long loads = 0, clampedLoads = 0, stores = 0; };

// one block of n frames for a task of `count` members; x[m], p[m]: operands; z[lane]: state in, state out
static void run_block(uint32_t n, uint32_t count, const std::vector<std::vector<float>>& x, const std::vector<float>& p,
                      std::vector<float>& z, std::vector<std::vector<float>>& out, std::vector<std::vector<int>>& writes, Stats& st) {
    const uint32_t groups = n / cs::kGroup;
    const unsigned long long smask = cs::store_mask(count);
    auto load = [&](uint32_t lane, uint32_t g, uint32_t j) -> float {     // operand of step j of group g, as the lane loads it
        const uint32_t m = cs::lane_member(lane, count), k = cs::lane_skew(lane, count), q = j / cs::kQuad;
        const uint32_t off = cs::load_offset(g, q, k, n);
        st.loads++;
        CHECK(off <= 4u * n - 16u && off % 16u == 0u, "n %u count %u lane %u g %u q %u: offset %u", n, count, lane, g, q, off);
        const int64_t plain = (int64_t)(64u * g + 16u * q) - 16 * (int64_t)k;
        if (plain != (int64_t)off) st.clampedLoads++;
        if (g >= 1u && g < groups) {     // steady: the kernel forms VGPR bias + immediate bias, no clamp
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
                if (g > 0u || cs::head_active(k, j)) { z[lane] = xv + p[m] * z[lane]; y[j] = z[lane]; }
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
    for (uint32_t lane = 0; lane < 64u; ++lane) {     // tail
        const uint32_t m = cs::lane_member(lane, count), k = cs::lane_skew(lane, count);
        for (uint32_t j = 0; j < cs::kTailSteps; ++j) {
            const float xv = load(lane, groups, j);
            if (cs::tail_active(k, j)) z[lane] = xv + p[m] * z[lane];
        }
    }
}

static void one_case(uint32_t n, uint32_t count, std::mt19937& rng, Stats& st) {
    std::uniform_real_distribution<float> ux(-1.0f, 1.0f), up(-0.98f, 0.98f);
    CHECK(cs::applies(count), "count %u", count);
    std::vector<float> p(count), zs(count), z(64);
    for (uint32_t m = 0; m < count; ++m) { p[m] = up(rng); zs[m] = ux(rng); }
    for (uint32_t lane = 0; lane < 64u; ++lane) z[lane] = zs[cs::lane_member(lane, count)];
    // lanes: 4 per member, skews 0 .. 3; the rest mirror the last member unskewed and do not store
    for (uint32_t lane = 0; lane < 64u; ++lane) {
        const uint32_t m = cs::lane_member(lane, count), k = cs::lane_skew(lane, count);
        CHECK(m < count && k < 4u, "lane %u", lane);
        if (lane < 4u * count) CHECK(m == lane / 4u && k == lane % 4u, "lane %u -> (%u, %u)", lane, m, k);
        else CHECK(m == count - 1u && k == 0u && !((cs::store_mask(count) >> lane) & 1ull), "mirror lane %u", lane);
    }
    for (int block = 0; block < 2; ++block) {
        std::vector<std::vector<float>> x(count, std::vector<float>(n)), out(count, std::vector<float>(n, -7.0f)), ref(count, std::vector<float>(n));
        std::vector<std::vector<int>> writes(count, std::vector<int>(n, 0));
        for (uint32_t m = 0; m < count; ++m) for (uint32_t t = 0; t < n; ++t) x[m][t] = ux(rng);
        for (uint32_t m = 0; m < count; ++m) for (uint32_t t = 0; t < n; ++t) { zs[m] = x[m][t] + p[m] * zs[m]; ref[m][t] = zs[m]; }
        run_block(n, count, x, p, z, out, writes, st);
        for (uint32_t m = 0; m < count; ++m)
            for (uint32_t t = 0; t < n; ++t) {
                CHECK(writes[m][t] == 1, "n %u count %u member %u frame %u written %d times", n, count, m, t, writes[m][t]);
                CHECK(bits(out[m][t]) == bits(ref[m][t]), "n %u count %u member %u frame %u: %08x vs %08x", n, count, m, t, bits(out[m][t]), bits(ref[m][t]));
            }
        for (uint32_t lane = 0; lane < 64u; ++lane)
            CHECK(bits(z[lane]) == bits(zs[cs::lane_member(lane, count)]), "n %u count %u block %d lane %u: final state", n, count, block, lane);
    }
}

int main() {
    std::mt19937 rng(20260118u);
    Stats st;
    int cases = 0;
    const uint32_t ns[] = {64u, 128u, 192u, 512u}, counts[] = {1u, 3u, 16u};
    for (uint32_t n : ns) for (uint32_t c : counts) { one_case(n, c, rng, st); ++cases; }
    CHECK(!cs::applies(17u) && !cs::applies(0u) && !cs::applies(64u), "a task of 17 members must be refused");
    CHECK(cs::applies(16u) && cs::store_mask(16u) == ~0ull && cs::store_mask(1u) == 0xFull, "store masks");
    std::printf("{\"ok\": %s, \"cases\": %d, \"loads\": %ld, \"clamped_loads\": %ld, \"stores\": %ld, \"failures\": %d}\n",
                failures ? "false" : "true", cases, st.loads, st.clampedLoads, st.stores, failures);
    return failures ? 1 : 0;
}
