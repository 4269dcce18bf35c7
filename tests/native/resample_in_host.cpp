// The input-rate converter without a GPU: elementary_amd/csrc/resample.h (the input side) and pcm_unpack.h compiled for the host.
//   plans      L, M, T, Do, H of the ratios the tests name (fin = the input's rate, fout = the engine's), and which rates have no plan
//   need       inputs_before(n) against the smallest t with ceil(t L / M) >= n, by brute force for n <= 5000
//   scalar     resample_in_host() over 3000 engine frames of sine plus noise per ratio, in one call (<workdir>/in_x_..., in_y_...: the
//              consumed inputs and the outputs) and cut into calls of 1, 37, 511 and 1453 engine frames: bits, carried frames, counts
//   lanes      the kernels' schedule (resample_in.hip) emulated workgroup by workgroup and lane by lane with the headers' functions over
//              launch sets with two history copies, the set's stretch staged as the engine stages it (streams a 16-byte multiple
//              apart, garbage behind each): every byte read lies inside its stream's staging stride, every LDS slot and image byte
//              lies in range and was staged, no tap reaches in front of the carried frames, every frame of the set's input half is
//              written exactly once, zeros behind the last valid frame, and the programme equals the scalar loop bit for bit
// Prints one JSON line. Usage: resample_in_host <workdir>
//   resample_in_host <workdir> apply <fin> <fout> <channels> <engineFrames>   resample_in_host() over <workdir>/apply_in.f32
//              ([channels][frames] decoded input, one programme from time 0) into <workdir>/apply_out.f32 ([channels][engineFrames]):
//              what the engine's render must be fed for those inputs, bit for bit
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "resample.h"
#include "pcm_unpack.h"

namespace rs = resample;
namespace pp = pcm_pack;
namespace pu = pcm_unpack;

static void dump(const std::string& path, const float* p, size_t n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(p, sizeof(float), n, f) != n) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
    fclose(f);
}

struct Tables { rs::Plan p; std::vector<float> table; std::vector<int32_t> rowBase; };
static bool tables(double fin, double fout, Tables& t) {
    if (!rs::make_plan_in(fin, fout, t.p)) return false;
    t.table.assign((size_t)t.p.T * t.p.L, 0.0f); t.rowBase.assign(t.p.L, 0);
    rs::make_tables(t.p, t.table.data(), t.rowBase.data());
    return true;
}

// sample codes of a programme: sine plus noise, as the format holds them (f32: the float's bits)
static uint32_t code_of(uint32_t fmt, double v) {
    if (fmt == pp::S16) return (uint32_t)(int32_t)lrint(v * 32767.0) & 0xFFFFu;
    if (fmt == pp::S24) return (uint32_t)(int32_t)lrint(v * 8388607.0) & 0xFFFFFFu;
    return pp::float_bits((float)v);
}
static std::vector<uint32_t> codes(uint32_t fmt, size_t n, uint32_t seed, double freq) {
    std::vector<uint32_t> x(n);
    uint32_t s = seed;
    for (size_t i = 0; i < n; ++i) {
        s = s * 1664525u + 1013904223u;
        x[i] = code_of(fmt, 0.6 * sin(6.283185307179586 * freq * (double)i) + 0.3 * ((double)(s >> 8) / 8388608.0 - 1.0));
    }
    return x;
}

// ---- the kernels' schedule ---------------------------------------------------------------------------------------------------------
struct LaneCheck { uint64_t ldsOut = 0, ldsUnstaged = 0, spanOver = 0, writtenTwice = 0, unwritten = 0, outOfHalf = 0, tailNotZero = 0, srcOut = 0, histFront = 0; };

struct Launch {
    const unsigned char* src; size_t srcBytes; uint64_t streamStride;
    uint32_t fmt, G, numStreams, bs, nCh, validIn, validOut, numBlocks;
    uint64_t t0, n0;
    const float* histIn; float* histOut;
};

// a read of `bytes` at offset `off` of stream s: inside the stream's stride (and the buffer)?
static bool src_ok(const Launch& a, uint32_t s, uint64_t off, uint32_t bytes) {
    return off + bytes <= a.streamStride && (uint64_t)s * a.streamStride + off + bytes <= a.srcBytes;
}
static float sample_at(const Launch& a, uint32_t s, uint64_t frame, uint32_t g, LaneCheck& chk) {
    const uint64_t off = (frame * a.G + g) * pp::sample_bytes(a.fmt);
    if (frame >= a.validIn || !src_ok(a, s, off, pp::sample_bytes(a.fmt))) { chk.srcOut++; return 0.0f; }
    return pu::decode(a.fmt, pu::load_raw(a.fmt, a.src + (size_t)s * a.streamStride + off));
}

// one launch: elemhip_resample_in<FMT, C> over grid (tiles, streams x groups) and the history step; dst is [numBlocks][nCh][bs]
template <int C>
static void emulate_launch(const Tables& t, const Launch& a, std::vector<float>& dst, LaneCheck& chk) {
    const rs::Plan& p = t.p;
    const uint32_t G = a.G, B = pp::sample_bytes(a.fmt), groups = (G + C - 1) / C, bs = a.bs, nCh = a.nCh;
    const uint32_t rowFloats = rs::row_floats(p), tiles = (uint32_t)rs::ceil_div((uint64_t)a.numBlocks * bs, rs::kTile);
    const uint32_t imageOff = rs::in_image_offset(p, C), ldsBytes = rs::in_lds_bytes(p, C);
    if ((size_t)C * rowFloats * 4u > imageOff || ldsBytes > 65536u) chk.ldsOut++;
    std::vector<int> writes(dst.size(), 0);
    std::vector<float> rows((size_t)C * rowFloats);
    std::vector<char> staged((size_t)C * rowFloats);
    std::vector<unsigned char> image(ldsBytes - imageOff);
    std::vector<char> imageStaged(image.size());
    for (uint32_t by = 0; by < a.numStreams * groups; ++by)
        for (uint32_t bx = 0; bx < tiles; ++bx) {
            const uint32_t fFirst = bx * rs::kTile, s = by / groups, g0 = (by % groups) * C;
            std::fill(staged.begin(), staged.end(), 0);
            std::fill(imageStaged.begin(), imageStaged.end(), 0);
            rs::Tile tile{0, 0u};
            if (fFirst < a.validOut) {
                tile = rs::tile_of(p, t.rowBase.data(), a.n0, fFirst, a.validOut);
                if (tile.span > rs::span_max(p)) chk.spanOver++;
                const int64_t rel0 = tile.jlo - (int64_t)a.t0;
                const rs::StreamPart part = rs::stream_part(rel0, tile.span, a.validIn);
                if (part.hi < tile.span) chk.srcOut++;            // (a slot behind the stretch: a tap would reach past what the call was given)
                for (uint32_t lane = 0; lane < rs::kTile; ++lane)
                    for (int ch = 0; ch < C; ++ch) {
                        const bool live = g0 + ch < G;
                        const float* hist = a.histIn + ((size_t)s * G + (live ? g0 + ch : 0u)) * p.H;
                        for (uint32_t i = lane; i < tile.span; i += rs::kTile) {
                            if (live && i >= part.lo && i < part.hi) continue;
                            if (rs::skew(i) >= rowFloats) { chk.ldsOut++; continue; }
                            const int64_t rel = rel0 + (int64_t)i;
                            if (live && i < part.lo && rel + (int64_t)p.H < 0 && (int64_t)a.t0 + rel >= 0) chk.histFront++;
                            rows[(size_t)ch * rowFloats + rs::skew(i)] = live && i < part.lo ? rs::carried_at(hist, p.H, rel) : 0.0f;
                            staged[(size_t)ch * rowFloats + rs::skew(i)] = 1;
                        }
                    }
                if (part.hi > part.lo) {
                    const uint64_t frame0 = (uint64_t)(rel0 + (int64_t)part.lo);
                    if (G <= (uint32_t)C) {
                        const uint64_t c0 = frame0 * G * B;
                        const uint32_t head = pp::image_head(c0), total = (part.hi - part.lo) * G, pieces = pp::piece_count(head, total * B);
                        for (uint32_t lane = 0; lane < rs::kTile; ++lane)
                            for (uint32_t q = lane; q < pieces; q += rs::kTile) {
                                if (16u * q + 16u > image.size()) { chk.ldsOut++; continue; }
                                if (!src_ok(a, s, c0 - head + 16u * q, 16u)) { chk.srcOut++; continue; }
                                memcpy(image.data() + 16u * q, a.src + (size_t)s * a.streamStride + (size_t)(c0 - head) + 16u * q, 16);
                                memset(imageStaged.data() + 16u * q, 1, 16);
                            }
                        for (uint32_t lane = 0; lane < rs::kTile; ++lane)
                            for (uint32_t j = lane; j < total; j += rs::kTile) {
                                const uint32_t off = pp::image_offset(head, j, a.fmt), slot = rs::skew(part.lo + j / G);
                                if (off + B > image.size() || slot >= rowFloats) { chk.ldsOut++; continue; }
                                for (uint32_t k = 0; k < B; ++k) if (!imageStaged[off + k]) chk.ldsUnstaged++;
                                rows[(size_t)(j % G) * rowFloats + slot] = pu::decode(a.fmt, pu::load_raw(a.fmt, image.data() + off));
                                staged[(size_t)(j % G) * rowFloats + slot] = 1;
                            }
                    } else {
                        for (uint32_t lane = 0; lane < rs::kTile; ++lane)
                            for (int ch = 0; ch < C; ++ch)
                                if (g0 + ch < G)
                                    for (uint32_t i = part.lo + lane; i < part.hi; i += rs::kTile) {
                                        if (rs::skew(i) >= rowFloats) { chk.ldsOut++; continue; }
                                        rows[(size_t)ch * rowFloats + rs::skew(i)] = sample_at(a, s, frame0 + (i - part.lo), g0 + ch, chk);
                                        staged[(size_t)ch * rowFloats + rs::skew(i)] = 1;
                                    }
                    }
                }
            }
            for (uint32_t lane = 0; lane < rs::kTile; ++lane) {
                const uint32_t f = fFirst + lane;
                if ((uint64_t)f >= (uint64_t)a.numBlocks * bs) continue;
                float acc[C];
                for (int ch = 0; ch < C; ++ch) acc[ch] = 0.0f;
                if (f < a.validOut) {
                    const uint64_t n = a.n0 + f;
                    const uint32_t base = rs::lane_base(p, t.rowBase.data(), tile, n);
                    rs::tap_sum<C>(t.table.data() + (uint32_t)(n % p.L), p.L, p.T, [&](int ch, uint32_t k) {
                        const uint32_t slot = rs::skew(base + k);
                        if (slot >= rowFloats) { chk.ldsOut++; return 0.0f; }
                        if (!staged[(size_t)ch * rowFloats + slot]) chk.ldsUnstaged++;
                        return rows[(size_t)ch * rowFloats + slot];
                    }, acc);
                }
                for (int ch = 0; ch < C; ++ch) {
                    if (g0 + ch >= G) continue;
                    const size_t at = ((size_t)(f / bs) * nCh + (size_t)s * G + g0 + ch) * bs + f % bs;
                    if (at >= dst.size()) { chk.outOfHalf++; continue; }
                    dst[at] = acc[ch];
                    writes[at]++;
                }
            }
        }
    for (uint32_t b = 0; b < a.numBlocks; ++b)
        for (uint32_t c = 0; c < a.numStreams * G; ++c)
            for (uint32_t i = 0; i < bs; ++i) {
                const size_t at = ((size_t)b * nCh + c) * bs + i;
                if (writes[at] == 0) chk.unwritten++;
                if (writes[at] > 1) chk.writtenTwice++;
                if ((uint64_t)b * bs + i >= a.validOut && dst[at] != 0.0f) chk.tailNotZero++;
            }
    // the history step: grid (ceil(H / 256), channels)
    for (uint32_t c = 0; c < a.numStreams * G; ++c)
        for (uint32_t j = 0; j < p.H; ++j)
            a.histOut[(size_t)c * p.H + j] = rs::history_pull([&](uint32_t fr) { return sample_at(a, c / G, fr, c % G, chk); }, a.histIn + (size_t)c * p.H, a.validIn, p.H, j);
}

// a programme of `frames` engine frames fed by `nStreams` streams of G channels in format fmt, rendered in launch sets of setBlocks
// blocks of bs frames (the last block cut), against resample_in_host() over each decoded channel in one call
static std::string lanes(const Tables& t, uint32_t fmt, uint32_t G, uint32_t nStreams, uint32_t bs, uint32_t setBlocks, size_t frames) {
    const rs::Plan& p = t.p;
    const uint32_t nCh = nStreams * G, B = pp::sample_bytes(fmt);
    const size_t inFrames = (size_t)rs::inputs_before(p, frames);
    std::vector<std::vector<float>> x(nCh), want(nCh), got(nCh);
    std::vector<std::vector<unsigned char>> stream(nStreams, std::vector<unsigned char>(inFrames * G * B + 1));
    for (uint32_t c = 0; c < nCh; ++c) {
        const std::vector<uint32_t> cd = codes(fmt, inFrames, 77u + c, 0.01 + 0.0003 * c);
        x[c].resize(inFrames + 1);
        for (size_t f = 0; f < inFrames; ++f) {
            x[c][f] = pu::decode(fmt, cd[f]);
            unsigned char* d = stream[c / G].data() + (f * G + c % G) * B;
            for (uint32_t k = 0; k < B; ++k) d[k] = (unsigned char)(cd[f] >> (8u * k));
        }
        std::vector<float> hist(p.H, 0.0f);
        want[c].resize(frames);
        rs::resample_in_host(p, t.table.data(), t.rowBase.data(), hist.data(), x[c].data(), 0, frames, want[c].data());
    }
    const uint32_t C = G > 1u && rs::in_lds_bytes(p, rs::kGroup) <= 65536u ? rs::kGroup : 1u;      // (launch_resample_in's choice)
    const size_t numBlocks = (frames + bs - 1) / bs;
    const uint64_t maxIn = rs::ceil_div((uint64_t)setBlocks * bs * p.M, p.L) + 1u;
    std::vector<float> hist[2] = {std::vector<float>((size_t)nCh * p.H, 0.0f), std::vector<float>((size_t)nCh * p.H, 0.0f)};
    int cur = 0;
    uint64_t n = 0, inOff = 0, overCap = 0, shortSets = 0;
    LaneCheck chk;
    for (size_t b0 = 0; b0 < numBlocks; b0 += setBlocks) {
        const size_t nb = std::min<size_t>(setBlocks, numBlocks - b0);
        Launch a{};
        a.validOut = (uint32_t)std::min<size_t>(nb * bs, frames - b0 * bs);
        a.t0 = rs::inputs_before(p, n); a.n0 = n;
        a.validIn = (uint32_t)(rs::inputs_before(p, n + a.validOut) - a.t0);
        if (a.validIn > maxIn || a.t0 != inOff) overCap++;
        shortSets += a.validOut < p.T;
        a.streamStride = pp::stream_stride(a.validIn, G, fmt);
        std::vector<unsigned char> staging((size_t)nStreams * a.streamStride, 0xAB);      // (garbage the kernel must not decode)
        for (uint32_t s = 0; s < nStreams; ++s) memcpy(staging.data() + s * a.streamStride, stream[s].data() + inOff * G * B, (size_t)a.validIn * G * B);
        a.src = staging.data(); a.srcBytes = staging.size(); a.fmt = fmt; a.G = G; a.numStreams = nStreams; a.bs = bs; a.nCh = nCh; a.numBlocks = (uint32_t)nb;
        a.histIn = hist[cur].data(); a.histOut = hist[cur ^ 1].data();
        std::vector<float> dst(nb * nCh * bs, -7.0f);
        if (C == 1u) emulate_launch<1>(t, a, dst, chk); else emulate_launch<(int)rs::kGroup>(t, a, dst, chk);
        cur ^= 1;
        for (uint32_t c = 0; c < nCh; ++c)
            for (uint32_t f = 0; f < a.validOut; ++f) got[c].push_back(dst[((size_t)(f / bs) * nCh + c) * bs + f % bs]);
        n += a.validOut; inOff += a.validIn;
    }
    uint64_t differing = 0;
    for (uint32_t c = 0; c < nCh; ++c) {
        if (got[c].size() != want[c].size()) { differing += 1u << 20; continue; }
        for (size_t i = 0; i < got[c].size(); ++i) differing += memcmp(&got[c][i], &want[c][i], 4) != 0;
    }
    char buf[640];
    snprintf(buf, sizeof buf, "{\"L\":%u,\"M\":%u,\"fmt\":%u,\"G\":%u,\"streams\":%u,\"bs\":%u,\"set_blocks\":%u,\"frames\":%zu,\"group\":%u,\"consumed\":%llu,\"short_sets\":%llu,"
             "\"differing\":%llu,\"lds_out\":%llu,\"lds_unstaged\":%llu,\"span_over\":%llu,\"written_twice\":%llu,\"unwritten\":%llu,\"out_of_half\":%llu,"
             "\"tail_not_zero\":%llu,\"src_out\":%llu,\"hist_front\":%llu,\"over_cap\":%llu}",
             p.L, p.M, fmt, G, nStreams, bs, setBlocks, frames, C, (unsigned long long)inOff, (unsigned long long)shortSets, (unsigned long long)differing,
             (unsigned long long)chk.ldsOut, (unsigned long long)chk.ldsUnstaged, (unsigned long long)chk.spanOver, (unsigned long long)chk.writtenTwice,
             (unsigned long long)chk.unwritten, (unsigned long long)chk.outOfHalf, (unsigned long long)chk.tailNotZero, (unsigned long long)chk.srcOut,
             (unsigned long long)chk.histFront, (unsigned long long)overCap);
    return buf;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: resample_in_host <workdir>\n"); return 2; }
    const std::string dir = argv[1];
    if (argc == 7 && std::string(argv[2]) == "apply") {
        Tables t;
        const size_t nCh = (size_t)atoi(argv[5]), frames = (size_t)atoll(argv[6]);
        if (!tables(atof(argv[3]), atof(argv[4]), t) || nCh == 0) { fprintf(stderr, "no plan\n"); return 1; }
        FILE* f = fopen((dir + "/apply_in.f32").c_str(), "rb");
        if (!f) { fprintf(stderr, "no input\n"); return 2; }
        fseek(f, 0, SEEK_END);
        const size_t floats = (size_t)ftell(f) / sizeof(float), n = floats / nCh;
        fseek(f, 0, SEEK_SET);
        std::vector<float> x(floats + 1);
        if (fread(x.data(), sizeof(float), floats, f) != floats) { fprintf(stderr, "short read\n"); return 2; }
        fclose(f);
        if (n < rs::inputs_before(t.p, frames)) { fprintf(stderr, "%zu input frames, %zu engine frames need %llu\n", n, frames, (unsigned long long)rs::inputs_before(t.p, frames)); return 1; }
        std::vector<float> y(nCh * frames + 1);
        for (size_t c = 0; c < nCh; ++c) {
            std::vector<float> hist(t.p.H, 0.0f);
            rs::resample_in_host(t.p, t.table.data(), t.rowBase.data(), hist.data(), x.data() + c * n, 0, frames, y.data() + c * frames);
        }
        dump(dir + "/apply_out.f32", y.data(), nCh * frames);
        printf("{\"frames\":%zu,\"consumed\":%llu}\n", frames, (unsigned long long)rs::inputs_before(t.p, frames));
        return 0;
    }
    const double ratios[5][2] = {{44100, 176400}, {44100, 48000}, {48000, 44100}, {8000, 12000}, {12000, 8000}};
    std::string out = "{\"plans\":[";
    char buf[512];
    for (int i = 0; i < 5; ++i) {
        Tables t;
        if (!tables(ratios[i][0], ratios[i][1], t)) { fprintf(stderr, "no plan for %g -> %g\n", ratios[i][0], ratios[i][1]); return 1; }
        // need(n) by brute force: the smallest t with ceil(t L / M) >= n
        uint64_t needWrong = 0, tt = 0;
        for (uint64_t n = 0; n <= 5000; ++n) {
            while ((tt * t.p.L + t.p.M - 1) / t.p.M < n) ++tt;
            needWrong += rs::inputs_before(t.p, n) != tt;
        }
        snprintf(buf, sizeof buf, "%s{\"fin\":%d,\"fout\":%d,\"L\":%u,\"M\":%u,\"T\":%u,\"Do\":%u,\"Wc\":%u,\"H\":%u,\"need_wrong\":%llu}", i ? "," : "", (int)ratios[i][0],
                 (int)ratios[i][1], t.p.L, t.p.M, t.p.T, t.p.Do, t.p.Wc, t.p.H, (unsigned long long)needWrong);
        out += buf;
    }
    out += "],\"refused\":[";
    // not integral twice over, M > 8 L (fine for the output side: 9 -> 1 has a plan there), T > 1024
    const double bad[5][2] = {{44101, 44100}, {0.5, 44100}, {72000, 8000}, {136000, 8000}, {44100, 0}};
    for (int i = 0; i < 5; ++i) {
        rs::Plan p{};
        snprintf(buf, sizeof buf, "%s{\"fin\":%.10g,\"fout\":%.10g,\"refused\":%s,\"output_side\":%s}", i ? "," : "", bad[i][0], bad[i][1],
                 rs::make_plan_in(bad[i][0], bad[i][1], p) ? "false" : "true", rs::make_plan(bad[i][0], bad[i][1], p) ? "true" : "false");
        out += buf;
    }
    out += "],\"scalar\":[";
    for (int i = 0; i < 5; ++i) {
        Tables t;
        tables(ratios[i][0], ratios[i][1], t);
        const size_t n = 3000, ni = (size_t)rs::inputs_before(t.p, n);
        std::vector<float> x(ni + 1);
        { const std::vector<uint32_t> cd = codes(pp::F32, ni, 5u + (uint32_t)i, 997.0 / ratios[i][0]); for (size_t k = 0; k < ni; ++k) x[k] = pu::decode(pp::F32, cd[k]); }
        std::vector<float> hist(t.p.H, 0.0f), y(n);
        const size_t used = rs::resample_in_host(t.p, t.table.data(), t.rowBase.data(), hist.data(), x.data(), 0, n, y.data());
        snprintf(buf, sizeof buf, "in_x_%d_%d.f32", (int)ratios[i][0], (int)ratios[i][1]);
        dump(dir + "/" + buf, x.data(), ni);
        snprintf(buf, sizeof buf, "in_y_%d_%d.f32", (int)ratios[i][0], (int)ratios[i][1]);
        dump(dir + "/" + buf, y.data(), y.size());
        snprintf(buf, sizeof buf, "%s{\"fin\":%d,\"fout\":%d,\"frames\":%zu,\"consumed\":%zu,\"cuts\":[", i ? "," : "", (int)ratios[i][0], (int)ratios[i][1], n, used);
        out += buf;
        const size_t cuts[4] = {1, 37, 511, 1453};
        for (int c = 0; c < 4; ++c) {
            std::vector<float> h2(t.p.H, 0.0f), y2(n);
            uint64_t done = 0, tIn = 0, countsWrong = 0;
            while (done < n) {
                const size_t m = std::min(cuts[c], n - (size_t)done);
                tIn += rs::resample_in_host(t.p, t.table.data(), t.rowBase.data(), h2.data(), x.data() + tIn, done, m, y2.data() + done);
                done += m;
                countsWrong += tIn != rs::inputs_before(t.p, done);
            }
            const bool same = tIn == used && memcmp(y2.data(), y.data(), n * sizeof(float)) == 0 && memcmp(h2.data(), hist.data(), hist.size() * sizeof(float)) == 0;
            snprintf(buf, sizeof buf, "%s{\"call_frames\":%zu,\"same_bits\":%s,\"counts_wrong\":%llu}", c ? "," : "", cuts[c], same ? "true" : "false", (unsigned long long)countsWrong);
            out += buf;
        }
        out += "]}";
    }
    out += "],\"lanes\":[";
    bool first = true;
    const uint32_t fmts[3] = {pp::S16, pp::S24, pp::F32};
    for (int i = 0; i < 5; ++i) {
        Tables t;
        tables(ratios[i][0], ratios[i][1], t);
        // 20 blocks + 37 frames in sets of 8: three sets, a cut last block, carried frames across set boundaries. One-channel streams
        // (the one-channel kernel, the image), 3 (the image, a silent fourth row), 8 and 40 (wide: sample by sample, two and ten
        // groups); the formats rotate so that every format meets every width over the five ratios
        const uint32_t Gs[4] = {1, 3, 8, 40}, sizes[4] = {350, 128, 512, 128}, streams[4] = {3, 2, 1, 1};
        for (int g = 0; g < 4; ++g) {
            out += (first ? "" : ",") + lanes(t, fmts[(i + g) % 3], Gs[g], streams[g], sizes[g], 8u, 20u * sizes[g] + 37u);
            first = false;
        }
        // sets shorter than T: one block of 16 engine frames a set, through the one-channel kernel
        out += "," + lanes(t, fmts[i % 3], 1u, 2u, 16u, 1u, 40u * 16u + 5u);
    }
    {   // a plan whose four rows and image do not fit 64 KB: a three-channel stream through the one-channel kernel, sample by sample
        Tables t;
        if (!tables(64000, 8000, t)) { fprintf(stderr, "no plan for 64000 -> 8000\n"); return 1; }
        out += "," + lanes(t, pp::S24, 3u, 1u, 128u, 8u, 9u * 128u + 19u);
    }
    out += "]}";
    printf("%s\n", out.c_str());
    return 0;
}
