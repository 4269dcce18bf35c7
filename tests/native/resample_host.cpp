// The delivery-rate converter without a GPU: elementary_amd/csrc/resample.h compiled for the host.
//   plans      L, M, T, Do, H of the ratios the tests name, and which rates have no plan
//   tables     the prototype each plan's table holds, de-interleaved from the kernel's [k][r] order into time order
//              (<workdir>/proto_<fin>_<fout>.f32): the test measures the filter from it
//   scalar     resample_host() over 3000 frames of sine plus noise per ratio, in one call (<workdir>/x_..., y_...) and cut into calls
//              of 1, 37, 511 and 1453 frames: bits and counts
//   lanes      the kernel's schedule (resample.hip) emulated workgroup by workgroup and lane by lane with the header's functions over
//              launch sets with two history copies: every LDS slot read was staged and lies inside the row, every frame of the
//              converted half is written exactly once, and the programme equals the scalar loop bit for bit
// Prints one JSON line. Usage: resample_host <workdir>
//   resample_host <workdir> apply <fin> <fout> <channels>   resample_host() over <workdir>/apply_in.f32 ([channels][frames], one
//              programme from time 0) into <workdir>/apply_out.f32: what the engine must deliver for those floats, bit for bit
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "resample.h"

namespace rs = resample;

static std::vector<float> signal(size_t n, uint32_t seed, double freq) {
    std::vector<float> x(n);
    uint32_t s = seed;
    for (size_t i = 0; i < n; ++i) {
        s = s * 1664525u + 1013904223u;
        x[i] = (float)(0.6 * sin(6.283185307179586 * freq * (double)i) + 0.3 * ((double)(s >> 8) / 8388608.0 - 1.0));
    }
    return x;
}

static void dump(const std::string& path, const float* p, size_t n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(p, sizeof(float), n, f) != n) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
    fclose(f);
}

struct Tables { rs::Plan p; std::vector<float> table; std::vector<int32_t> rowBase; };
static bool tables(double fin, double fout, Tables& t) {
    if (!rs::make_plan(fin, fout, t.p)) return false;
    t.table.assign((size_t)t.p.T * t.p.L, 0.0f); t.rowBase.assign(t.p.L, 0);
    rs::make_tables(t.p, t.table.data(), t.rowBase.data());
    return true;
}

// ---- the kernel's schedule ---------------------------------------------------------------------------------------------------------
struct LaneCheck { uint64_t ldsOut = 0, ldsUnstaged = 0, spanOver = 0, writtenTwice = 0, unwritten = 0, outOfHalf = 0, tailNotZero = 0; };

// one launch: elemhip_resample<C> over grid (tiles, groups) and the history step; dst is [outBlocks][nCh][bs]
template <int C>
static void emulate_launch(const Tables& t, const float* src, uint32_t bs, uint32_t nCh, uint32_t validIn, const float* histIn, float* histOut,
                           uint64_t t0, uint64_t n0, uint32_t validOut, uint32_t outBlocks, std::vector<float>& dst, LaneCheck& chk) {
    const rs::Plan& p = t.p;
    const uint32_t rowFloats = rs::row_floats(p), tiles = (uint32_t)rs::ceil_div((uint64_t)outBlocks * bs, rs::kTile), groups = (nCh + C - 1) / C;
    std::vector<int> writes(dst.size(), 0);
    std::vector<float> rows((size_t)C * rowFloats);
    std::vector<char> staged((size_t)C * rowFloats);
    for (uint32_t by = 0; by < groups; ++by)
        for (uint32_t bx = 0; bx < tiles; ++bx) {
            const uint32_t fFirst = bx * rs::kTile, c0 = by * C;
            std::fill(staged.begin(), staged.end(), 0);
            rs::Tile tile{0, 0u};
            if (fFirst < validOut) {
                tile = rs::tile_of(p, t.rowBase.data(), n0, fFirst, validOut);
                if (tile.span > rs::span_max(p)) chk.spanOver++;
                const int64_t rel0 = tile.jlo - (int64_t)t0;
                for (uint32_t lane = 0; lane < rs::kTile; ++lane)
                    for (int ch = 0; ch < C; ++ch) {
                        const uint32_t c = c0 + ch;
                        const float* hist = histIn + (size_t)(c < nCh ? c : 0u) * p.H;
                        for (uint32_t i = lane; i < tile.span; i += rs::kTile) {
                            const size_t at = (size_t)ch * rowFloats + rs::skew(i);
                            if (rs::skew(i) >= rowFloats) { chk.ldsOut++; continue; }
                            rows[at] = c < nCh ? rs::input_at(src, bs, nCh, c, validIn, hist, p.H, rel0 + (int64_t)i) : 0.0f;
                            staged[at] = 1;
                        }
                    }
            }
            for (uint32_t lane = 0; lane < rs::kTile; ++lane) {
                const uint32_t f = fFirst + lane;
                if ((uint64_t)f >= (uint64_t)outBlocks * bs) continue;
                float acc[C];
                for (int ch = 0; ch < C; ++ch) acc[ch] = 0.0f;
                if (f < validOut) {
                    const uint64_t n = n0 + f;
                    const uint32_t base = rs::lane_base(p, t.rowBase.data(), tile, n);
                    rs::tap_sum<C>(t.table.data() + (uint32_t)(n % p.L), p.L, p.T, [&](int ch, uint32_t k) {
                        const uint32_t slot = rs::skew(base + k);
                        if (slot >= rowFloats) { chk.ldsOut++; return 0.0f; }
                        if (!staged[(size_t)ch * rowFloats + slot]) chk.ldsUnstaged++;
                        return rows[(size_t)ch * rowFloats + slot];
                    }, acc);
                }
                for (int ch = 0; ch < C; ++ch) {
                    if (c0 + ch >= nCh) continue;
                    const size_t at = ((size_t)(f / bs) * nCh + c0 + ch) * bs + f % bs;
                    if (at >= dst.size()) { chk.outOfHalf++; continue; }
                    dst[at] = acc[ch];
                    writes[at]++;
                }
            }
        }
    for (uint32_t b = 0; b < outBlocks; ++b)
        for (uint32_t c = 0; c < nCh; ++c)
            for (uint32_t i = 0; i < bs; ++i) {
                const size_t at = ((size_t)b * nCh + c) * bs + i;
                if (writes[at] == 0) chk.unwritten++;
                if (writes[at] > 1) chk.writtenTwice++;
                if ((uint64_t)b * bs + i >= validOut && dst[at] != 0.0f) chk.tailNotZero++;
            }
    for (uint32_t c = 0; c < nCh; ++c)
        for (uint32_t j = 0; j < p.H; ++j) histOut[(size_t)c * p.H + j] = rs::history_next(src, bs, nCh, c, histIn + (size_t)c * p.H, validIn, p.H, j);
}

// a programme of `frames` frames of nCh channels rendered in launch sets of setBlocks blocks of bs frames (the last block cut),
// against resample_host() over each channel in one call
static std::string lanes(const Tables& t, uint32_t bs, uint32_t nCh, uint32_t setBlocks, size_t frames, bool single) {
    const rs::Plan& p = t.p;
    std::vector<std::vector<float>> x(nCh);
    for (uint32_t c = 0; c < nCh; ++c) x[c] = signal(frames, 77u + c, 0.01 + 0.003 * c);
    std::vector<std::vector<float>> want(nCh), got(nCh);
    for (uint32_t c = 0; c < nCh; ++c) {
        std::vector<float> hist(p.H, 0.0f);
        want[c].resize((size_t)rs::outputs_before(p, frames));
        rs::resample_host(p, t.table.data(), t.rowBase.data(), hist.data(), x[c].data(), frames, 0, want[c].data());
    }
    const size_t numBlocks = (frames + bs - 1) / bs;
    const size_t capFrames = (size_t)rs::ceil_div((uint64_t)setBlocks * bs * p.L, p.M) + 1, capBlocks = (capFrames + bs - 1) / bs;
    std::vector<float> hist[2] = {std::vector<float>((size_t)nCh * p.H, 0.0f), std::vector<float>((size_t)nCh * p.H, 0.0f)};
    int cur = 0;
    uint64_t tIn = 0, tOut = 0;
    LaneCheck chk;
    uint64_t overCap = 0;
    for (size_t b0 = 0; b0 < numBlocks; b0 += setBlocks) {
        const size_t nb = std::min<size_t>(setBlocks, numBlocks - b0);
        std::vector<float> src(nb * nCh * bs, 0.0f);
        for (size_t b = 0; b < nb; ++b)
            for (uint32_t c = 0; c < nCh; ++c)
                for (uint32_t i = 0; i < bs; ++i) { const size_t f = (b0 + b) * bs + i; src[(b * nCh + c) * bs + i] = f < frames ? x[c][f] : 123.0f; }      // (padding the kernel must not read)
        const uint32_t validIn = (uint32_t)std::min<size_t>(nb * bs, frames - b0 * bs);
        const uint32_t validOut = (uint32_t)(rs::outputs_before(p, tIn + validIn) - tOut), outBlocks = (validOut + bs - 1) / bs;
        if (outBlocks > capBlocks) { overCap++; break; }
        std::vector<float> dst((size_t)capBlocks * nCh * bs, -7.0f);
        if (single) emulate_launch<1>(t, src.data(), bs, nCh, validIn, hist[cur].data(), hist[cur ^ 1].data(), tIn, tOut, validOut, outBlocks, dst, chk);
        else emulate_launch<(int)rs::kGroup>(t, src.data(), bs, nCh, validIn, hist[cur].data(), hist[cur ^ 1].data(), tIn, tOut, validOut, outBlocks, dst, chk);
        cur ^= 1;
        for (uint32_t c = 0; c < nCh; ++c)
            for (uint32_t f = 0; f < validOut; ++f) got[c].push_back(dst[((size_t)(f / bs) * nCh + c) * bs + f % bs]);
        tIn += validIn; tOut += validOut;
    }
    uint64_t differing = 0;
    for (uint32_t c = 0; c < nCh; ++c) {
        if (got[c].size() != want[c].size()) { differing += 1u << 20; continue; }
        for (size_t i = 0; i < got[c].size(); ++i) differing += memcmp(&got[c][i], &want[c][i], 4) != 0;
    }
    char buf[512];
    snprintf(buf, sizeof buf, "{\"L\":%u,\"M\":%u,\"bs\":%u,\"channels\":%u,\"set_blocks\":%u,\"frames\":%zu,\"group\":%d,\"outputs\":%llu,\"differing\":%llu,"
             "\"lds_out\":%llu,\"lds_unstaged\":%llu,\"span_over\":%llu,\"written_twice\":%llu,\"unwritten\":%llu,\"out_of_half\":%llu,\"tail_not_zero\":%llu,\"over_cap\":%llu}",
             p.L, p.M, bs, nCh, setBlocks, frames, single ? 1 : (int)rs::kGroup, (unsigned long long)tOut, (unsigned long long)differing, (unsigned long long)chk.ldsOut,
             (unsigned long long)chk.ldsUnstaged, (unsigned long long)chk.spanOver, (unsigned long long)chk.writtenTwice, (unsigned long long)chk.unwritten,
             (unsigned long long)chk.outOfHalf, (unsigned long long)chk.tailNotZero, (unsigned long long)overCap);
    return buf;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: resample_host <workdir>\n"); return 2; }
    const std::string dir = argv[1];
    if (argc == 6 && std::string(argv[2]) == "apply") {
        Tables t;
        const size_t nCh = (size_t)atoi(argv[5]);
        if (!tables(atof(argv[3]), atof(argv[4]), t) || nCh == 0) { fprintf(stderr, "no plan\n"); return 1; }
        FILE* f = fopen((dir + "/apply_in.f32").c_str(), "rb");
        if (!f) { fprintf(stderr, "no input\n"); return 2; }
        fseek(f, 0, SEEK_END);
        const size_t floats = (size_t)ftell(f) / sizeof(float), n = floats / nCh;
        fseek(f, 0, SEEK_SET);
        std::vector<float> x(floats);
        if (fread(x.data(), sizeof(float), floats, f) != floats) { fprintf(stderr, "short read\n"); return 2; }
        fclose(f);
        const size_t m = (size_t)rs::outputs_before(t.p, n);
        std::vector<float> y(nCh * m);
        for (size_t c = 0; c < nCh; ++c) {
            std::vector<float> hist(t.p.H, 0.0f);
            rs::resample_host(t.p, t.table.data(), t.rowBase.data(), hist.data(), x.data() + c * n, n, 0, y.data() + c * m);
        }
        dump(dir + "/apply_out.f32", y.data(), y.size());
        printf("{\"frames\":%zu,\"outputs\":%zu}\n", n, m);
        return 0;
    }
    const double ratios[5][2] = {{48000, 44100}, {44100, 48000}, {176400, 44100}, {8000, 12000}, {12000, 8000}};
    std::string out = "{\"plans\":[";
    char buf[512];
    for (int i = 0; i < 5; ++i) {
        Tables t;
        if (!tables(ratios[i][0], ratios[i][1], t)) { fprintf(stderr, "no plan for %g -> %g\n", ratios[i][0], ratios[i][1]); return 1; }
        // time order: the prototype at t = (m - Wc L) / L, m = (T - 1 - k) L + p for row r of phase p
        std::vector<float> proto((size_t)t.p.T * t.p.L, 0.0f);
        for (uint32_t r = 0; r < t.p.L; ++r)
            for (uint32_t k = 0; k < t.p.T; ++k) proto[(size_t)(t.p.T - 1u - k) * t.p.L + rs::row_phase(t.p, r)] = t.table[(size_t)k * t.p.L + r];
        snprintf(buf, sizeof buf, "proto_%d_%d.f32", (int)ratios[i][0], (int)ratios[i][1]);
        dump(dir + "/" + buf, proto.data(), proto.size());
        snprintf(buf, sizeof buf, "%s{\"fin\":%d,\"fout\":%d,\"L\":%u,\"M\":%u,\"T\":%u,\"Do\":%u,\"Wc\":%u,\"H\":%u}", i ? "," : "", (int)ratios[i][0], (int)ratios[i][1],
                 t.p.L, t.p.M, t.p.T, t.p.Do, t.p.Wc, t.p.H);
        out += buf;
    }
    out += "],\"refused\":[";
    const double bad[5][2] = {{44100, 44101}, {8000, 192000}, {44100.5, 48000}, {48000, 0}, {1000000, 44100}};
    for (int i = 0; i < 5; ++i) {
        rs::Plan p{};
        snprintf(buf, sizeof buf, "%s{\"fin\":%.10g,\"fout\":%.10g,\"refused\":%s}", i ? "," : "", bad[i][0], bad[i][1], rs::make_plan(bad[i][0], bad[i][1], p) ? "false" : "true");
        out += buf;
    }
    out += "],\"scalar\":[";
    for (int i = 0; i < 5; ++i) {
        Tables t;
        tables(ratios[i][0], ratios[i][1], t);
        const size_t n = 3000;
        const std::vector<float> x = signal(n, 5u + (uint32_t)i, 997.0 / ratios[i][0]);
        std::vector<float> hist(t.p.H, 0.0f), y((size_t)rs::outputs_before(t.p, n));
        const size_t made = rs::resample_host(t.p, t.table.data(), t.rowBase.data(), hist.data(), x.data(), n, 0, y.data());
        snprintf(buf, sizeof buf, "x_%d_%d.f32", (int)ratios[i][0], (int)ratios[i][1]);
        dump(dir + "/" + buf, x.data(), x.size());
        snprintf(buf, sizeof buf, "y_%d_%d.f32", (int)ratios[i][0], (int)ratios[i][1]);
        dump(dir + "/" + buf, y.data(), y.size());
        snprintf(buf, sizeof buf, "%s{\"fin\":%d,\"fout\":%d,\"frames\":%zu,\"outputs\":%zu,\"cuts\":[", i ? "," : "", (int)ratios[i][0], (int)ratios[i][1], n, made);
        out += buf;
        const size_t cuts[4] = {1, 37, 511, 1453};
        for (int c = 0; c < 4; ++c) {
            std::vector<float> h2(t.p.H, 0.0f), y2, part(y.size() + 8);
            uint64_t tIn = 0, countsWrong = 0;
            while (tIn < n) {
                const size_t m = std::min(cuts[c], n - (size_t)tIn);
                const size_t k = rs::resample_host(t.p, t.table.data(), t.rowBase.data(), h2.data(), x.data() + tIn, m, tIn, part.data());
                y2.insert(y2.end(), part.begin(), part.begin() + k);
                tIn += m;
                countsWrong += y2.size() != (size_t)((tIn * t.p.L + t.p.M - 1) / t.p.M);
            }
            const bool same = y2.size() == y.size() && memcmp(y2.data(), y.data(), y.size() * sizeof(float)) == 0 && memcmp(h2.data(), hist.data(), hist.size() * sizeof(float)) == 0;
            snprintf(buf, sizeof buf, "%s{\"call_frames\":%zu,\"same_bits\":%s,\"counts_wrong\":%llu}", c ? "," : "", cuts[c], same ? "true" : "false", (unsigned long long)countsWrong);
            out += buf;
        }
        out += "]}";
    }
    out += "],\"lanes\":[";
    bool first = true;
    for (int i = 0; i < 5; ++i) {
        Tables t;
        tables(ratios[i][0], ratios[i][1], t);
        const uint32_t sizes[3] = {128, 512, 350};
        for (uint32_t bs : sizes) {
            // 20 blocks + 37 frames in sets of 8: three sets, a cut last block, history across set boundaries; 3 channels and 5 (a
            // group of four and a group of one)
            out += (first ? "" : ",") + lanes(t, bs, bs == 512 ? 5u : 3u, 8u, 20u * bs + 37u, false);
            first = false;
        }
        // sets shorter than T (and, at 4:1 with 256 taps, than the carried frames): one block of 128 a set, then sets of 19 frames' worth
        out += "," + lanes(t, 128u, 2u, 1u, 9u * 128u + 19u, false);
        out += "," + lanes(t, 16u, 3u, 1u, 40u * 16u + 5u, true);
    }
    out += "]}";
    printf("%s\n", out.c_str());
    return 0;
}
