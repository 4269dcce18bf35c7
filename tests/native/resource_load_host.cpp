// resource_load_host.cpp — the resource loader's pieces, tiles and lanes on the CPU (elementary_amd/csrc/resource_load.h and the
// headers behind it, which resource_load.hip takes every index from). A source of G = 1, 2, 3, 8 channels, the three PCM formats and
// N = 1, 63, 257, 1000 frames is loaded at the engine's rate and at 48000 -> 44100 (147:160), 44100 -> 48000, 96000 -> 44100 (T = 140)
// and 22050 -> 44100, cut into pieces of 64 and 256 source frames (pieces end inside a tile and inside a tap window) and as one piece.
// Every piece is staged as the engine stages it — exactly the staged bytes, so a load beyond them is the sanitizer's to catch — and
// the emulated threads run the kernel's stages in the kernel's order into poisoned rows. Checked: every frame of every row written
// exactly once and nothing else touched, the bits those of load_host() over the whole file, every 16-byte load and store aligned and
// inside its buffer, every LDS access inside the launch's LDS, every LDS slot read after it was written; the copy kernel's transposed
// half-wave writes and quad reads free of bank conflicts, the tap reads of the converting kernel at most 2-way and free of conflicts
// when upsampling. The last line is JSON.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "resource_load.h"

namespace rl = resource_load;
namespace rs = resample;
namespace pp = pcm_pack;
namespace pu = pcm_unpack;

static uint32_t rng = 0x2468ACEu;
static uint32_t rnd() { rng = rng * 1664525u + 1013904223u; return rng >> 8; }

struct Totals { long cases = 0, failures = 0, pieces = 0, wideLoads = 0, wideStores = 0, narrowStores = 0, halfWaveWrites = 0, writeConflicts = 0,
                halfWaveReads = 0, readConflicts = 0, tapReads = 0, tapConflicts = 0, tapOver2 = 0, tapUpConflicts = 0, stageWrites = 0, stageMaxWay = 0; };

static const uint32_t kPoison = 0xA5A5A5A5u;

struct Case { uint32_t G, fmt, N, fin, fout, P; };
static void fail(Totals& t, const char* what, const Case& c) {
    if (t.failures < 20) std::fprintf(stderr, "FAIL %s: G %u fmt %u N %u %u -> %u piece %u\n", what, c.G, c.fmt, c.N, c.fin, c.fout, c.P);
    t.failures++;
}

struct Rows {
    std::vector<uint32_t*> all, row;
    std::vector<std::vector<uint8_t>> writes;
    size_t floats = 0;
    static constexpr size_t guard = 16;
    void make(uint32_t G, size_t n) {
        floats = n + 5;                                  // (some floats behind the last frame: nobody's)
        for (uint32_t g = 0; g < G; ++g) {
            uint32_t* p = static_cast<uint32_t*>(std::aligned_alloc(64, ((floats + 2 * guard) * 4 + 63) / 64 * 64));
            for (size_t i = 0; i < floats + 2 * guard; ++i) p[i] = kPoison;
            all.push_back(p); row.push_back(p + guard); writes.emplace_back(floats, 0);
        }
    }
    ~Rows() { for (uint32_t* p : all) std::free(p); }
};

// ---- the copy kernel, one piece ----
static bool copy_piece(Totals& T, const Case& c, const unsigned char* staged, size_t srcBytes, uint32_t head, uint32_t validIn, uint64_t out0, Rows& R) {
    const uint32_t G = c.G, fmt = c.fmt, B = pp::sample_bytes(fmt);
    std::vector<uint16_t> rowBase(G);
    const uint32_t rowDwords = pp::row_bases(G, rowBase.data()), ldsBytes = pp::lds_bytes(rowDwords, G);
    if (ldsBytes > 65536u) return false;
    bool bad = false;
    for (uint32_t ti = 0; ti < rl::copy_tiles(validIn, G); ++ti) {
        std::vector<unsigned char> lds(ldsBytes, 0xEE);
        std::vector<uint8_t> rowWritten(rowDwords, 0);
        uint32_t* rows = reinterpret_cast<uint32_t*>(lds.data());
        const uint32_t imageAt = pp::lds_image_offset(rowDwords);
        unsigned char* image = lds.data() + imageAt;
        const uint32_t n = rl::copy_tile_frames(validIn, G, ti), f0 = rl::copy_tile_first(ti, G);
        if (n == 0u) { bad = true; continue; }
        // ---- A ----
        const uint64_t c0 = rl::copy_stretch_begin(head, f0, G, fmt);
        const uint32_t h = pp::image_head(c0), total = n * G, len = total * B, pieces = pp::piece_count(h, len);
        const size_t inOff = (size_t)(c0 - h);
        for (uint32_t p = 0; p < pieces; ++p) {
            const size_t at = inOff + 16u * p;
            if ((at & 15u) || at + 16u > srcBytes || 16u * p + 16u > pp::image_bytes(G) || imageAt + 16u * p + 16u > ldsBytes) { bad = true; break; }
            std::memcpy(image + 16u * p, staged + at, 16);
            T.wideLoads++;
        }
        // ---- B ----
        for (uint32_t j0 = 0; j0 < total; j0 += 32u) {
            uint32_t seen = 0;
            for (uint32_t j = j0; j < total && j < j0 + 32u; ++j) {
                const uint32_t bank = (rowBase[j % G] + j / G) & 31u;
                if (seen & (1u << bank)) T.writeConflicts++;
                seen |= 1u << bank;
            }
            T.halfWaveWrites++;
        }
        for (uint32_t tid = 0; tid < pp::kThreads; ++tid) {
            uint32_t g = tid % G, f = tid / G;
            const uint32_t dg = pp::kThreads % G, df = pp::kThreads / G;
            for (uint32_t j = tid; j < total; j += pp::kThreads) {
                if (g != j % G || f != j / G) bad = true;
                const uint32_t o = pp::image_offset(h, j, fmt), at = rowBase[g] + f;
                if (o < h || o + B > h + len || at >= rowDwords || rowWritten[at]) { bad = true; break; }
                rowWritten[at] = 1;
                rows[at] = pu::decode_bits(fmt, pu::load_raw(fmt, image + o));
                g += dg; f += df;
                if (g >= G) { g -= G; ++f; }
            }
        }
        // ---- C ----
        const uint32_t chunks = rl::copy_row_chunks(n), items = G * chunks;
        for (uint32_t wave = 0; wave < pp::kWaves; ++wave)
            for (uint32_t item = wave; item < items; item += pp::kWaves) {
                const uint32_t g = item / chunks;
                const size_t rowAt = (size_t)out0 + f0;
                const uint32_t m = (uint32_t)(reinterpret_cast<uintptr_t>(R.row[g] + rowAt) >> 2) & 3u;
                if (pp::row_quads(n, m) > chunks * 64u) bad = true;
                for (uint32_t e = 0; e < 4u; ++e)
                    for (uint32_t hw = 0; hw < 2u; ++hw) {
                        uint32_t seen = 0; bool any = false;
                        for (uint32_t lane = 32u * hw; lane < 32u * hw + 32u; ++lane) {
                            const int32_t f = pp::quad_first((item % chunks) * 64u + lane, m) + (int32_t)pu::quad_slot(e, lane);
                            if (f < 0 || (uint32_t)f >= n) continue;
                            const uint32_t bank = (rowBase[g] + (uint32_t)f) & 31u;
                            if (seen & (1u << bank)) T.readConflicts++;
                            seen |= 1u << bank; any = true;
                        }
                        if (any) T.halfWaveReads++;
                    }
                for (uint32_t lane = 0; lane < 64u; ++lane) {
                    const int32_t first = pp::quad_first((item % chunks) * 64u + lane, m);
                    uint32_t t[4], v[4];
                    for (uint32_t e = 0; e < 4u; ++e) {
                        const int32_t f = first + (int32_t)pu::quad_slot(e, lane);
                        t[e] = 0u;
                        if (f >= 0 && (uint32_t)f < n) {
                            const uint32_t at = rowBase[g] + (uint32_t)f;
                            if (at >= rowDwords || !rowWritten[at]) { bad = true; continue; }
                            t[e] = rows[at];
                        }
                    }
                    for (uint32_t x = 0; x < 4u; ++x) v[x] = t[pu::quad_read_of(x, lane)];
                    const bool whole = pp::quad_whole(first, n);
                    if (whole) { if (reinterpret_cast<uintptr_t>(R.row[g] + rowAt + first) & 15u) bad = true; T.wideStores++; }
                    for (int32_t x = 0; x < 4; ++x) {
                        const int32_t f = first + x;
                        if (f < 0 || (uint32_t)f >= n) continue;
                        if (!whole) T.narrowStores++;
                        if (rowAt + (size_t)f >= R.floats) { bad = true; continue; }
                        R.row[g][rowAt + f] = v[x];
                        R.writes[g][rowAt + f]++;
                    }
                }
            }
    }
    return !bad;
}

// ---- the converting kernel, one piece ----
static bool convert_piece(Totals& T, const Case& c, const rs::Plan& p, const float* table, const int32_t* rowBase, const unsigned char* staged,
                          size_t srcBytes, uint32_t head, uint64_t in0, uint32_t validIn, uint64_t out0, uint32_t validOut, Rows& R) {
    const uint32_t G = c.G, fmt = c.fmt, B = pp::sample_bytes(fmt), C = rl::convert_channels(p, G);
    if (C == 0u) return false;
    const uint32_t ldsBytes = rs::in_lds_bytes(p, C), rowFloats = rs::row_floats(p), groups = (G + C - 1u) / C;
    const uint64_t n0 = rl::programme_output(p, out0);
    bool bad = false;
    for (uint32_t bx = 0; bx < (validOut + rs::kTile - 1u) / rs::kTile; ++bx)
        for (uint32_t by = 0; by < groups; ++by) {
            std::vector<unsigned char> lds(ldsBytes, 0xEE);
            std::vector<uint8_t> written((size_t)C * rowFloats, 0);
            float* rows = reinterpret_cast<float*>(lds.data());
            const uint32_t fFirst = bx * rs::kTile, g0 = by * C;
            const rs::Tile t = rs::tile_of(p, rowBase, n0, fFirst, validOut);
            const int64_t rel0 = t.jlo - (int64_t)in0;
            const rs::StreamPart part = rs::stream_part(rel0, t.span, validIn);
            if (t.span > rs::span_max(p)) { bad = true; continue; }
            auto put = [&](uint32_t ch, uint32_t slot, float x) {
                const size_t at = (size_t)ch * rowFloats + rs::skew(slot);
                if (ch >= C || rs::skew(slot) >= rowFloats || at * 4u + 4u > rs::in_image_offset(p, C) || written[at]) { bad = true; return; }
                written[at] = 1; rows[at] = x;
            };
            for (uint32_t ch = 0; ch < C; ++ch) {
                const bool live = g0 + ch < G;
                for (uint32_t i = 0; i < t.span; ++i) if (!live || i < part.lo || i >= part.hi) put(ch, i, 0.0f);
            }
            if (part.hi > part.lo) {
                const uint64_t frame0 = (uint64_t)(rel0 + (int64_t)part.lo);
                if (rel0 + (int64_t)part.lo < 0 || frame0 + (part.hi - part.lo) > validIn) { bad = true; continue; }
                if (G <= C) {
                    const uint32_t imageAt = rs::in_image_offset(p, C);
                    unsigned char* image = lds.data() + imageAt;
                    const uint64_t c0 = (uint64_t)head + frame0 * G * B;
                    const uint32_t h = pp::image_head(c0), total = (part.hi - part.lo) * G, pieces = pp::piece_count(h, total * B);
                    for (uint32_t q = 0; q < pieces; ++q) {
                        const size_t at = (size_t)(c0 - h) + 16u * q;
                        if ((at & 15u) || at + 16u > srcBytes || imageAt + 16u * q + 16u > ldsBytes) { bad = true; break; }
                        std::memcpy(image + 16u * q, staged + at, 16);
                        T.wideLoads++;
                    }
                    for (uint32_t j0 = 0; j0 < total; j0 += 32u) {      // a half-wave's staging write: distinct addresses per bank
                        uint32_t ways[32] = {0};
                        for (uint32_t j = j0; j < total && j < j0 + 32u; ++j) ways[((j % G) * rowFloats + rs::skew(part.lo + j / G)) & 31u]++;
                        for (uint32_t b = 0; b < 32u; ++b) if ((long)ways[b] > T.stageMaxWay) T.stageMaxWay = ways[b];
                        T.stageWrites++;
                    }
                    for (uint32_t j = 0; j < total; ++j) {
                        const uint32_t o = pp::image_offset(h, j, fmt);
                        if (o + B > h + total * B) { bad = true; break; }
                        put(j % G, part.lo + j / G, pu::decode(fmt, pu::load_raw(fmt, image + o)));
                    }
                } else {
                    for (uint32_t ch = 0; ch < C; ++ch)
                        if (g0 + ch < G)
                            for (uint32_t i = part.lo; i < part.hi; ++i) {
                                const size_t at = (size_t)head + ((frame0 + (i - part.lo)) * G + g0 + ch) * B;
                                if (at + B > srcBytes) { bad = true; continue; }
                                put(ch, i, pu::decode(fmt, pu::load_raw(fmt, staged + at)));
                            }
                }
            }
            // ---- C: the tap reads' banks, half-wave by half-wave, then the sums ----
            for (uint32_t hw = 0; hw * 32u < rs::kTile; ++hw)
                for (uint32_t k = 0; k < p.T; ++k) {
                    uint32_t addr[32][3], ways[32] = {0};
                    bool any = false;
                    for (uint32_t lane = 32u * hw; lane < 32u * hw + 32u; ++lane) {
                        const uint32_t f = fFirst + lane;
                        if (f >= validOut) continue;
                        const uint32_t a = rs::skew(rs::lane_base(p, rowBase, t, n0 + f) + k), b = a & 31u;
                        bool dup = false;
                        for (uint32_t w = 0; w < ways[b] && w < 3u; ++w) dup = dup || addr[b][w] == a;
                        if (!dup) { if (ways[b] < 3u) addr[b][ways[b]] = a; ways[b]++; }
                        any = true;
                    }
                    if (!any) continue;
                    uint32_t worst = 0;
                    for (uint32_t b = 0; b < 32u; ++b) worst = ways[b] > worst ? ways[b] : worst;
                    T.tapReads++;
                    if (worst > 1u) { T.tapConflicts++; if (p.L >= p.M) T.tapUpConflicts++; }
                    if (worst > 2u) T.tapOver2++;
                }
            for (uint32_t lane = 0; lane < rs::kTile; ++lane) {
                const uint32_t f = fFirst + lane;
                if (f >= validOut) continue;
                const uint64_t n = n0 + f;
                const uint32_t base = rs::lane_base(p, rowBase, t, n);
                float acc[rs::kGroup];
                auto fetch = [&](int ch, uint32_t k) {
                    const size_t at = (size_t)ch * rowFloats + rs::skew(base + k);
                    if (base + k >= t.span || !written[at]) { bad = true; return 0.0f; }
                    return rows[at];
                };
                if (C == 1u) rs::tap_sum<1>(table + (uint32_t)(n % p.L), p.L, p.T, fetch, acc);
                else rs::tap_sum<(int)rs::kGroup>(table + (uint32_t)(n % p.L), p.L, p.T, fetch, acc);
                for (uint32_t ch = 0; ch < C; ++ch)
                    if (g0 + ch < G) {
                        const size_t at = (size_t)out0 + f;
                        if (at >= R.floats) { bad = true; continue; }
                        std::memcpy(&R.row[g0 + ch][at], &acc[ch], 4);
                        R.writes[g0 + ch][at]++;
                    }
            }
        }
    return !bad;
}

static void run_case(Totals& T, const Case& c) {
    T.cases++;
    const uint32_t G = c.G, fmt = c.fmt, B = pp::sample_bytes(fmt);
    const uint64_t N = c.N;
    // the file: exactly its bytes
    std::vector<unsigned char> file((size_t)N * G * B);
    for (unsigned char& b : file) b = (unsigned char)rnd();
    if (fmt == pp::F32)                                  // finite floats of moderate size, with a few denormals and signed zeros
        for (size_t i = 0; i + 4 <= file.size(); i += 4) {
            const uint32_t r = rnd();
            uint32_t u = (r & 0x80000000u) | (0x3C000000u + (rnd() & 0x03FFFFFFu));
            if (r % 61u == 0u) u = r & 0x807FFFFFu;
            std::memcpy(&file[i], &u, 4);
        }
    rs::Plan plan{};
    const bool convert = c.fin != c.fout;
    if (convert && !rs::make_plan((double)c.fin, (double)c.fout, plan)) { fail(T, "plan", c); return; }
    std::vector<float> table(convert ? (size_t)plan.T * plan.L : 1);
    std::vector<int32_t> rowBase(convert ? plan.L : 1);
    if (convert) rs::make_tables(plan, table.data(), rowBase.data());
    const rs::Plan* pl = convert ? &plan : nullptr;
    const uint64_t outN = rl::out_frames(pl, N);

    // the scalar loop over the whole file
    std::vector<std::vector<float>> ref(G, std::vector<float>((size_t)outN));
    std::vector<float*> refRows(G);
    for (uint32_t g = 0; g < G; ++g) refRows[g] = ref[g].data();
    rl::load_host(fmt, G, N, file.data(), pl, table.data(), rowBase.data(), refRows.data());

    Rows R;
    R.make(G, (size_t)outN);
    bool ok = true;
    uint64_t nextOut = 0;
    for (uint64_t j = 0; j < rl::piece_count(N, c.P); ++j) {
        T.pieces++;
        const rl::Piece pc = rl::piece_of(pl, N, c.P, j);
        if (pc.out0 != nextOut || pc.in1 <= pc.in0 || pc.in1 > N) ok = false;
        nextOut = pc.out1;
        const uint32_t head = rl::piece_head(pc.in0, G, fmt), validIn = (uint32_t)(pc.in1 - pc.in0);
        const size_t srcBytes = (size_t)rl::piece_bytes(head, validIn, G, fmt);
        if (srcBytes > rl::staging_bytes(pl, c.P, G, fmt)) ok = false;
        unsigned char* staged = static_cast<unsigned char*>(std::aligned_alloc(64, (srcBytes + 63) / 64 * 64));
        std::memset(staged, 0xC3, srcBytes);
        const uint64_t from = rl::piece_begin(pc.in0, G, fmt) - head, have = srcBytes < file.size() - from ? srcBytes : file.size() - from;
        std::memcpy(staged, file.data() + from, (size_t)have);
        if (convert) ok = convert_piece(T, c, plan, table.data(), rowBase.data(), staged, srcBytes, head, pc.in0, validIn, pc.out0, (uint32_t)(pc.out1 - pc.out0), R) && ok;
        else ok = copy_piece(T, c, staged, srcBytes, head, validIn, pc.out0, R) && ok;
        std::free(staged);
    }
    if (nextOut != outN) ok = false;
    if (!ok) fail(T, "schedule", c);
    bool same = true;
    for (uint32_t g = 0; g < G; ++g) {
        for (size_t i = 0; i < R.floats; ++i) {
            if (i < outN) { uint32_t u; std::memcpy(&u, &ref[g][i], 4); if (R.writes[g][i] != 1 || R.row[g][i] != u) same = false; }
            else if (R.writes[g][i] != 0 || R.row[g][i] != kPoison) same = false;
        }
        for (size_t i = 0; i < Rows::guard; ++i) if (R.all[g][i] != kPoison || R.all[g][Rows::guard + R.floats + i] != kPoison) same = false;
    }
    if (!same) fail(T, "floats", c);
}

int main() {
    Totals T;
    const uint32_t groups[] = {1u, 2u, 3u, 8u}, formats[] = {pp::S16, pp::S24, pp::F32}, sizes[] = {1u, 63u, 257u, 1000u};
    const uint32_t rates[][2] = {{44100u, 44100u}, {48000u, 44100u}, {44100u, 48000u}, {96000u, 44100u}, {22050u, 44100u}};
    const uint32_t cuts[] = {64u, 256u, 1u << 20};
    for (uint32_t G : groups) for (uint32_t fmt : formats) for (uint32_t N : sizes) for (auto& r : rates) for (uint32_t P : cuts)
        run_case(T, Case{G, fmt, N, r[0], r[1], P});
    // the widest source, both kernels; a tile's worth of frames and more in one piece
    run_case(T, Case{32u, pp::S24, 300u, 44100u, 44100u, 128u});
    run_case(T, Case{32u, pp::S16, 300u, 48000u, 44100u, 128u});
    run_case(T, Case{2u, pp::S16, 5000u, 44100u, 44100u, 1u << 20});
    run_case(T, Case{2u, pp::S24, 5000u, 44100u, 96000u, 4096u});
    // the plan of the third pair is the one the issue names
    rs::Plan p96{};
    rs::make_plan(96000.0, 44100.0, p96);
    std::printf("{\"cases\":%ld,\"failures\":%ld,\"pieces\":%ld,\"wide_loads\":%ld,\"wide_stores\":%ld,\"narrow_stores\":%ld,\"half_wave_writes\":%ld,"
                "\"write_conflicts\":%ld,\"half_wave_reads\":%ld,\"read_conflicts\":%ld,\"tap_reads\":%ld,\"tap_conflicts\":%ld,\"tap_over_2way\":%ld,"
                "\"tap_upsampling_conflicts\":%ld,\"stage_writes\":%ld,\"stage_max_way\":%ld,\"taps_96000_44100\":%u,\"ok\":%s}\n",
                T.cases, T.failures, T.pieces, T.wideLoads, T.wideStores, T.narrowStores, T.halfWaveWrites, T.writeConflicts, T.halfWaveReads,
                T.readConflicts, T.tapReads, T.tapConflicts, T.tapOver2, T.tapUpConflicts, T.stageWrites, T.stageMaxWay, p96.T,
                T.failures == 0 ? "true" : "false");
    return T.failures == 0 ? 0 : 1;
}
