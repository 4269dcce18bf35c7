// limiter_host.cpp — elementary_amd/csrc/limiter.h on the CPU (tests/test_limiter_host.py builds and runs it; no GPU, no HIP):
//   (no mode)  the plans and their refusals; the scalar loop limiter_host() over a test programme, in one call and cut into calls; the
//              kernels' schedule (limiter.hip) emulated workgroup by workgroup and lane by lane — every loop over `lane` below is what
//              the lanes of one workgroup do between two barriers — over block sizes, look-aheads and links, against the scalar loop
//              bit for bit. Writes x / y files for the numpy comparison and prints one JSON line.
//   apply      limiter_host() over <dir>/apply_in.f32 [channels][frames] -> apply_out.f32 and apply_stats.json, cut into calls of
//              `call` frames: what the GPU tests compare the host-block path with.
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

#include "limiter.h"

namespace lm = limiter;

static std::vector<float> programme(uint32_t nCh, size_t n, uint32_t seed) {
    std::vector<float> x((size_t)nCh * n);
    uint32_t r = seed * 2654435761u + 12345u;
    for (uint32_t c = 0; c < nCh; ++c)
        for (size_t f = 0; f < n; ++f) {
            r = r * 1664525u + 1013904223u;
            const double noise = ((double)(r >> 8) / 8388608.0 - 1.0);
            const double loud = ((f / ((n < 300u ? 40u : 300u) + 90u * c)) % 3u == 1u) ? 3.0 : 0.3;      // (loud stretches in the shortest programmes too)
            double v = c % 2u == 0u ? 0.4 * sin(1.5707963267948966 * (double)f + 0.7853981633974483 + c) * (loud > 1.0 ? 3.5 : 1.0) : loud * noise;
            if (f == 777u + 13u * c) v = 3.0;
            x[(size_t)c * n + f] = (float)v;
        }
    if (n > 1500 && nCh > 1) { uint32_t nan = 0x7FC00000u, inf = 0x7F800000u; memcpy(&x[n + 1200], &nan, 4); memcpy(&x[n + 1400], &inf, 4); }
    return x;
}

struct Run { std::vector<float> y; std::vector<unsigned char> state; std::vector<lm::GroupStats> stats; };

static Run scalar(const loudness::Plan& lp, const lm::Plan& p, uint32_t nCh, const std::vector<float>& x, size_t n, size_t call) {
    Run r;
    r.y.assign((size_t)nCh * n, 0.0f);
    r.state.resize(lm::state_bytes(p, nCh));
    lm::state_reset(p, nCh, r.state.data());
    r.stats.assign(lm::group_count(p, nCh), lm::GroupStats{0u, 0u});
    for (size_t f0 = 0; f0 < n; f0 += call) {
        const size_t m = call < n - f0 ? call : n - f0;
        lm::limiter_host(lp, p, nCh, r.state.data(), r.stats.data(), x.data() + f0, n, m, f0, r.y.data() + f0, n);
    }
    return r;
}

// ---- the kernels of limiter.hip, lane loops for lanes --------------------------------------------------------------------------------
struct Args {
    const float* src; float* dst; const unsigned char* stateIn; unsigned char* stateOut; lm::GroupStats* stats; double* frames; double* tiles;
    uint64_t n0; uint32_t bs, nCh, valid, outBlocks, frameCap, tileCap; lm::Plan p; loudness::Plan lp;
};
static uint64_t gOutside = 0;      // stores the kernels would have made outside their buffers

static void emu_detect(const Args& a, uint32_t tile, uint32_t g) {
    const lm::Plan& p = a.p;
    const uint32_t E = lm::ext_frames(p), width = lm::group_width(p, a.nCh), groups = lm::group_count(p, a.nCh), H = lm::hist_frames(p), fFirst = tile * lm::kTile;
    std::vector<double> m0(E), m1(E);
    std::vector<float> row(lm::row_frames(p));
    double* from = m0.data();
    double* to = m1.data();
    const float* hist = reinterpret_cast<const float*>(a.stateIn + lm::state_off_hist(p, groups));
    for (uint32_t k = 0; k < width; ++k) {
        const uint32_t c = g * width + k;
        for (uint32_t lane = 0; lane < lm::kTile; ++lane) lm::tile_stage(p, a.src, a.bs, a.nCh, c, a.valid, hist + (size_t)c * H, fFirst, lane, row.data());
        for (uint32_t lane = 0; lane < lm::kTile; ++lane) lm::tile_detect(a.lp, p, row.data(), k == 0u, lane, from);
    }
    for (uint32_t lane = 0; lane < lm::kTile; ++lane) lm::tile_reduce(p, lane, from);
    const uint32_t P = lm::hold_pow2(p);
    for (uint32_t w = 1u; w < P; w *= 2u) {
        for (uint32_t lane = 0; lane < lm::kTile; ++lane) lm::tile_double(p, from, to, w, lane);
        double* t = from; from = to; to = t;
    }
    double waves[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (uint32_t lane = 0; lane < lm::kTile; ++lane) {
        const double dm = lm::tile_hold(p, from, P, lane);
        const uint32_t f = fFirst + lane;
        if (f < a.valid) {
            if (f >= a.frameCap) { ++gOutside; continue; }
            a.frames[(size_t)g * a.frameCap + f] = dm;
            waves[lane >> 6] = lm::dmax(waves[lane >> 6], dm + lm::ramp(p, a.n0 + f));
        }
    }
    if (tile >= a.tileCap) { ++gOutside; return; }
    a.tiles[(size_t)g * a.tileCap + tile] = lm::dmax(lm::dmax(waves[0], waves[1]), lm::dmax(waves[2], waves[3]));
}

static void emu_scan(const Args& a, uint32_t g) {
    const uint32_t numTiles = lm::tile_count(a.valid);
    double carry = reinterpret_cast<const double*>(a.stateIn)[g];
    double* at = a.tiles + (size_t)g * a.tileCap;
    for (uint32_t t0 = 0; t0 < numTiles; t0 += 64u) {
        double v[64], up[64];
        for (uint32_t lane = 0; lane < 64u; ++lane) v[lane] = t0 + lane < numTiles ? at[t0 + lane] : -INFINITY;
        for (uint32_t o = 1u; o < 64u; o <<= 1) {
            for (uint32_t lane = 0; lane < 64u; ++lane) up[lane] = lane >= o ? v[lane - o] : v[lane];
            for (uint32_t lane = 0; lane < 64u; ++lane) if (lane >= o) v[lane] = lm::dmax(v[lane], up[lane]);
        }
        for (uint32_t lane = 0; lane < 64u; ++lane)
            if (t0 + lane < numTiles) at[t0 + lane] = lane == 0u ? carry : lm::dmax(carry, v[lane - 1u]);
        carry = lm::dmax(carry, v[63]);
    }
    reinterpret_cast<double*>(a.stateOut)[g] = carry;
}

static void emu_release(const Args& a, uint32_t tile, uint32_t g) {
    const lm::Plan& p = a.p;
    double sc[2][lm::kTile], dm[lm::kTile], ns[lm::kTile];
    for (uint32_t lane = 0; lane < lm::kTile; ++lane) {
        const uint32_t f = tile * lm::kTile + lane;
        const bool live = f < a.valid;
        dm[lane] = live ? a.frames[(size_t)g * a.frameCap + f] : 0.0;
        ns[lane] = lm::ramp(p, a.n0 + f);
        sc[0][lane] = live ? dm[lane] + ns[lane] : -INFINITY;
    }
    double* from = sc[0];
    double* to = sc[1];
    for (uint32_t w = 1u; w < lm::kTile; w *= 2u) {
        for (uint32_t lane = 0; lane < lm::kTile; ++lane) lm::scan_step(from, to, w, lane);
        double* t = from; from = to; to = t;
    }
    for (uint32_t lane = 0; lane < lm::kTile; ++lane) {
        const uint32_t f = tile * lm::kTile + lane;
        if (f >= a.valid) continue;
        const double d = lm::release(dm[lane], lm::dmax(a.tiles[(size_t)g * a.tileCap + tile], from[lane]), ns[lane]);
        a.frames[(size_t)g * a.frameCap + f] = d;
        if (d > 0.0 && loudness::double_bits(d) > a.stats[g].maxBits) a.stats[g].maxBits = loudness::double_bits(d);       // atomicMax
    }
}

static void emu_apply(const Args& a, uint32_t tile, uint32_t g, std::vector<uint8_t>& written, size_t dstFloats) {
    const lm::Plan& p = a.p;
    const uint32_t width = lm::group_width(p, a.nCh), groups = lm::group_count(p, a.nCh), H = lm::hist_frames(p), fFirst = tile * lm::kTile, bs = a.bs;
    const double* dHist = reinterpret_cast<const double*>(a.stateIn + lm::state_off_d(p, groups)) + (size_t)g * p.D;
    const float* hist = reinterpret_cast<const float*>(a.stateIn + lm::state_off_hist(p, groups));
    std::vector<double> win(lm::kTile + p.D);
    for (uint32_t lane = 0; lane < lm::kTile; ++lane) lm::tile_window(p, a.frames + (size_t)g * a.frameCap, a.valid, dHist, fFirst, lane, win.data());
    for (uint32_t lane = 0; lane < lm::kTile; ++lane) {
        const uint32_t f = fFirst + lane;
        const bool live = f < a.valid, inside = (uint64_t)f < (uint64_t)a.outBlocks * bs;
        const double gn = live ? lm::tile_gain(p, win.data(), lane) : 1.0;
        if (inside)
            for (uint32_t k = 0; k < width; ++k) {
                const uint32_t c = g * width + k;
                const size_t at = ((size_t)(f / bs) * a.nCh + c) * bs + f % bs;
                if (at >= dstFloats) { ++gOutside; continue; }
                a.dst[at] = live ? lm::apply(p, gn, lm::input_at(a.src, bs, a.nCh, c, a.valid, hist + (size_t)c * H, H, (int64_t)f - (int64_t)lm::latency(p))) : 0.0f;
                ++written[at];
            }
        if (live && gn < 1.0) ++a.stats[g].limited;
    }
}

static void emu_history(const Args& a) {
    const lm::Plan& p = a.p;
    const uint32_t groups = lm::group_count(p, a.nCh), H = lm::hist_frames(p);
    for (uint32_t c = 0; c < a.nCh; ++c)
        for (uint32_t j = 0; j < H; ++j) {
            const float* old = reinterpret_cast<const float*>(a.stateIn + lm::state_off_hist(p, groups)) + (size_t)c * H;
            reinterpret_cast<float*>(a.stateOut + lm::state_off_hist(p, groups))[(size_t)c * H + j] = lm::history_next(a.src, a.bs, a.nCh, c, old, a.valid, H, j);
        }
    for (uint32_t g = 0; g < groups; ++g)
        for (uint32_t j = 0; j < p.D; ++j) {
            const double* old = reinterpret_cast<const double*>(a.stateIn + lm::state_off_d(p, groups)) + (size_t)g * p.D;
            reinterpret_cast<double*>(a.stateOut + lm::state_off_d(p, groups))[(size_t)g * p.D + j] = lm::d_history_next(a.frames + (size_t)g * a.frameCap, old, a.valid, p.D, j);
        }
}

struct LaneResult { uint64_t differing, writtenTwice, unwritten, tailNotZero, outside, stateDiffers, statsDiffer; };

// the programme in launch sets of setBlocks blocks of bs frames (the last block cut), emulated, against the scalar loop
static LaneResult lanes(const loudness::Plan& lp, const lm::Plan& p, uint32_t nCh, uint32_t bs, uint32_t setBlocks, size_t n, const std::vector<float>& x, const Run& want) {
    LaneResult r{0, 0, 0, 0, 0, 0, 0};
    const uint32_t groups = lm::group_count(p, nCh);
    const size_t setFrames = (size_t)setBlocks * bs, halfFloats = (size_t)setBlocks * nCh * bs;
    std::vector<unsigned char> state[2];
    for (auto& s : state) { s.resize(lm::state_bytes(p, nCh)); lm::state_reset(p, nCh, s.data()); }
    std::vector<lm::GroupStats> stats(groups, lm::GroupStats{0u, 0u});
    std::vector<double> frames((size_t)groups * setFrames), tiles((size_t)groups * lm::tile_count((uint32_t)setFrames));
    std::vector<float> src(halfFloats), dst(halfFloats);
    int cur = 0;
    gOutside = 0;
    for (size_t f0 = 0; f0 < n; f0 += setFrames) {
        const uint32_t valid = (uint32_t)(setFrames < n - f0 ? setFrames : n - f0), nb = (valid + bs - 1u) / bs;
        for (size_t b = 0; b < nb; ++b)
            for (uint32_t c = 0; c < nCh; ++c)
                for (uint32_t o = 0; o < bs; ++o) {
                    const size_t f = b * bs + o;
                    src[(b * nCh + c) * bs + o] = f < valid ? x[(size_t)c * n + f0 + f] : -99.0f;      // (what lies behind the set's last frame must not matter)
                }
        std::fill(dst.begin(), dst.end(), 77.0f);
        Args a{src.data(), dst.data(), state[cur].data(), state[cur ^ 1].data(), stats.data(), frames.data(), tiles.data(), (uint64_t)f0, bs, nCh, valid, nb,
               (uint32_t)setFrames, (uint32_t)lm::tile_count((uint32_t)setFrames), p, lp};
        const uint32_t numTiles = lm::tile_count(valid), outTiles = (uint32_t)(((uint64_t)nb * bs + lm::kTile - 1u) / lm::kTile);
        for (uint32_t g = 0; g < groups; ++g) for (uint32_t t = 0; t < numTiles; ++t) emu_detect(a, t, g);
        for (uint32_t g = 0; g < groups; ++g) emu_scan(a, g);
        for (uint32_t g = 0; g < groups; ++g) for (uint32_t t = 0; t < numTiles; ++t) emu_release(a, t, g);
        std::vector<uint8_t> written(halfFloats, 0);
        for (uint32_t g = 0; g < groups; ++g) for (uint32_t t = 0; t < outTiles; ++t) emu_apply(a, t, g, written, (size_t)nb * nCh * bs);
        emu_history(a);
        cur ^= 1;
        for (size_t b = 0; b < nb; ++b)
            for (uint32_t c = 0; c < nCh; ++c)
                for (uint32_t o = 0; o < bs; ++o) {
                    const size_t at = (b * nCh + c) * bs + o, f = b * bs + o;
                    if (written[at] > 1) ++r.writtenTwice;
                    if (written[at] == 0) ++r.unwritten;
                    if (f < valid) { if (memcmp(&dst[at], &want.y[(size_t)c * n + f0 + f], 4) != 0) ++r.differing; }
                    else if (dst[at] != 0.0f) ++r.tailNotZero;
                }
    }
    r.outside = gOutside;
    r.stateDiffers = memcmp(state[cur].data(), want.state.data(), want.state.size()) != 0;
    for (uint32_t g = 0; g < groups; ++g) r.statsDiffer += stats[g].maxBits != want.stats[g].maxBits || stats[g].limited != want.stats[g].limited;
    return r;
}

static bool same_run(const Run& a, const Run& b) {
    return a.y.size() == b.y.size() && memcmp(a.y.data(), b.y.data(), a.y.size() * 4) == 0 && a.state == b.state &&
           memcmp(a.stats.data(), b.stats.data(), a.stats.size() * sizeof(lm::GroupStats)) == 0;
}

static void write_floats(const std::string& path, const float* v, size_t n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(v, 4, n, f) != n) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: limiter_host <dir> [apply rate ceiling gain lookahead_ms release_ms link channels call]\n"); return 2; }
    const std::string dir = argv[1];
    if (argc >= 3 && std::string(argv[2]) == "apply") {
        if (argc < 11) return 2;
        const double rate = atof(argv[3]);
        lm::Plan p{};
        if (!lm::make_plan(rate, atof(argv[4]), atof(argv[5]), atof(argv[6]), atof(argv[7]), atof(argv[8]), p)) { fprintf(stderr, "no plan\n"); return 3; }
        const uint32_t nCh = (uint32_t)atoi(argv[9]);
        const size_t call = (size_t)atoll(argv[10]);
        if (!lm::channels_ok(p, nCh) || call == 0) return 3;
        loudness::Plan lp; loudness::make_plan(rate, lp);
        FILE* f = fopen((dir + "/apply_in.f32").c_str(), "rb");
        if (!f) return 2;
        fseek(f, 0, SEEK_END); const size_t total = (size_t)ftell(f) / 4; fseek(f, 0, SEEK_SET);
        std::vector<float> x(total);
        if (fread(x.data(), 4, total, f) != total) return 2;
        fclose(f);
        const size_t n = total / nCh;
        const Run r = scalar(lp, p, nCh, x, n, call);
        write_floats(dir + "/apply_out.f32", r.y.data(), r.y.size());
        FILE* o = fopen((dir + "/apply_stats.json").c_str(), "w");
        fprintf(o, "{\"max_reduction\": [");
        for (size_t g = 0; g < r.stats.size(); ++g) fprintf(o, "%s%.17g", g ? ", " : "", loudness::bits_double(r.stats[g].maxBits));
        fprintf(o, "], \"limited_frames\": [");
        for (size_t g = 0; g < r.stats.size(); ++g) fprintf(o, "%s%llu", g ? ", " : "", r.stats[g].limited);
        fprintf(o, "]}\n");
        fclose(o);
        return 0;
    }
    const double rate = 12000.0;
    loudness::Plan lp; loudness::make_plan(rate, lp);
    printf("{\"plans\": [");
    {
        // D = round(ms rate / 1000): 1 .. 1024 pass, everything else is refused; so are the other parameters outside their ranges
        struct Case { double rate, ceil, gain, look, rel, link; } cases[] = {
            {48000, -1, 0, 1.5, 500, 0}, {44100, -1, 0, 1.5, 500, 0}, {12000, -1, 0, 0.0834, 50, 0}, {12000, -1, 0, 1024.0 / 12.0, 50, 2}, {48000, -40, 60, 21.33, 0.02, 3},
            {12000, -1, 0, 0.04, 50, 0}, {12000, -1, 0, 1024.6 / 12.0, 50, 0}, {48000, -1, 0, 0, 500, 0}, {48000, -1, 0, -1, 500, 0}, {48000, 0.1, 0, 1.5, 500, 0},
            {48000, -40.5, 0, 1.5, 500, 0}, {48000, -1, 60.5, 1.5, 500, 0}, {48000, -1, -61, 1.5, 500, 0}, {48000, -1, 0, 1.5, 0.005, 0}, {48000, -1, 0, 1.5, 500, -1},
            {48000, -1, 0, 1.5, 500, 1.5}, {48000, -1, 0, NAN, 500, 0}, {0, -1, 0, 1.5, 500, 0}};
        bool first = true;
        for (const Case& c : cases) {
            lm::Plan p{}; p.D = 4242u;
            const bool ok = lm::make_plan(c.rate, c.ceil, c.gain, c.look, c.rel, c.link, p);
            char look[64];
            if (c.look == c.look) snprintf(look, sizeof look, "%.17g", c.look); else snprintf(look, sizeof look, "null");
            printf("%s{\"rate\": %.17g, \"lookahead_ms\": %s, \"ok\": %s, \"D\": %u, \"R\": %u, \"latency\": %u, \"hist\": %u, \"untouched\": %s}", first ? "" : ", ", c.rate,
                   look, ok ? "true" : "false", ok ? p.D : 0u, ok ? p.R : 0u, ok ? lm::latency(p) : 0u, ok ? lm::hist_frames(p) : 0u, ok || p.D == 4242u ? "true" : "false");
            first = false;
        }
    }
    printf("], \"scalar\": [");
    {
        bool first = true;
        const size_t n = 3000;
        const uint32_t nCh = 6;
        const std::vector<float> x = programme(nCh, n, 1u);
        write_floats(dir + "/x.f32", x.data(), x.size());
        const uint32_t Ds[] = {1, 18, 66, 300}, links[] = {0, 1, 2, 3};
        for (uint32_t D : Ds)
            for (uint32_t link : links) {
                lm::Plan p{};
                if (!lm::make_plan(rate, -1.0, 2.0, D * 1000.0 / rate, 50.0, link, p) || p.D != D) { fprintf(stderr, "plan D %u\n", D); return 1; }
                const Run one = scalar(lp, p, nCh, x, n, n);
                write_floats(dir + "/y_" + std::to_string(D) + "_" + std::to_string(link) + ".f32", one.y.data(), one.y.size());
                printf("%s{\"D\": %u, \"link\": %u, \"frames\": %zu, \"channels\": %u, \"max_reduction\": [", first ? "" : ", ", D, link, n, nCh);
                for (size_t g = 0; g < one.stats.size(); ++g) printf("%s%.17g", g ? ", " : "", loudness::bits_double(one.stats[g].maxBits));
                printf("], \"limited_frames\": [");
                for (size_t g = 0; g < one.stats.size(); ++g) printf("%s%llu", g ? ", " : "", one.stats[g].limited);
                printf("], \"cuts\": [");
                const size_t calls[] = {1, 37, 511, 1453};
                for (size_t k = 0; k < 4; ++k) printf("%s{\"call_frames\": %zu, \"same_bits\": %s}", k ? ", " : "", calls[k], same_run(one, scalar(lp, p, nCh, x, n, calls[k])) ? "true" : "false");
                printf("]}");
                first = false;
            }
    }
    printf("], \"lanes\": [");
    {
        bool first = true;
        const uint32_t nCh = 6, sizes[] = {16, 128, 350, 512}, Ds[] = {1, 18, 66, 300}, links[] = {0, 1, 2, 3};
        for (uint32_t bs : sizes)
            for (uint32_t D : Ds)
                for (uint32_t link : links) {
                    lm::Plan p{};
                    if (!lm::make_plan(rate, -1.0, 2.0, D * 1000.0 / rate, 50.0, link, p) || p.D != D) return 1;
                    // sets of 8 blocks, three sets and a cut last block; and sets of ONE block: at block size 16 and 128 shorter than the latency
                    for (uint32_t setBlocks : {8u, 1u}) {
                        if (setBlocks == 1u && !(bs <= 128u && (link == 0u || link == 2u))) continue;
                        const size_t n = setBlocks == 8u ? (size_t)20 * bs + 37 : (size_t)9 * bs + 5;
                        const std::vector<float> x = programme(nCh, n, bs + D);
                        const Run want = scalar(lp, p, nCh, x, n, n);
                        const LaneResult r = lanes(lp, p, nCh, bs, setBlocks, n, x, want);
                        uint64_t limited = 0;
                        for (const lm::GroupStats& s : want.stats) limited += s.limited;
                        printf("%s{\"bs\": %u, \"D\": %u, \"link\": %u, \"set_blocks\": %u, \"frames\": %zu, \"limited\": %llu, \"differing\": %llu, \"written_twice\": %llu, "
                               "\"unwritten\": %llu, \"tail_not_zero\": %llu, \"outside\": %llu, \"state_differs\": %llu, \"stats_differ\": %llu}", first ? "" : ", ", bs, D, link,
                               setBlocks, n, (unsigned long long)limited, (unsigned long long)r.differing, (unsigned long long)r.writtenTwice, (unsigned long long)r.unwritten,
                               (unsigned long long)r.tailNotZero, (unsigned long long)r.outside, (unsigned long long)r.stateDiffers, (unsigned long long)r.statsDiffer);
                        first = false;
                    }
                }
    }
    printf("]}\n");
    return 0;
}
