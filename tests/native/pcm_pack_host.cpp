// pcm_pack_host.cpp — the PCM pack kernel's tile and lane schedule on the CPU (elementary_amd/csrc/pcm_pack.h, the header pcm_pack.hip
// takes every index from): 256 emulated threads per tile run the three stages in the kernel's order over block sizes 32, 341, 350 and
// 512, G = 1, 2, 3, 6 and 8, all three formats, sets of 1 and 3 blocks, whole and with the last block cut. Checked: every delivered
// byte written exactly once and nothing else touched (guard bands around the streams, the bytes between a stream's end and its
// stride), every 16-byte load aligned and inside its row, every LDS access inside the launch's LDS, stage B's half-wave reads free of
// bank conflicts, bytes and statistics equal to a plain scalar loop. The last line is JSON; it also carries the codes of an edge
// vector and of 4096 dithered samples around t = 2^32 for the Python side to compare with its own restatement.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "pcm_pack.h"

namespace pp = pcm_pack;

static uint32_t rng = 0x1234567u;
static uint32_t rnd() { rng = rng * 1664525u + 1013904223u; return rng >> 8; }

struct Totals { long cases = 0, failures = 0, wideStores = 0, narrowStores = 0, wideLoads = 0, narrowLoads = 0, bankConflicts = 0, halfWaveReads = 0; };

static void fail(Totals& t, const char* what, uint32_t bs, uint32_t G, uint32_t fmt, uint32_t nb, uint32_t valid) {
    if (t.failures < 20) std::fprintf(stderr, "FAIL %s: bs %u G %u fmt %u blocks %u valid %u\n", what, bs, G, fmt, nb, valid);
    t.failures++;
}

static void run_case(Totals& T, uint32_t bs, uint32_t G, uint32_t fmt, uint32_t nb, uint32_t valid, bool dith) {
    T.cases++;
    const uint32_t nStreams = 2, nCh = nStreams * G, B = pp::sample_bytes(fmt), seed = 0xC0FFEEu + G;
    const int64_t time0 = ((int64_t)1 << 32) - (int64_t)(bs + 5);            // the set straddles 2^32
    const size_t srcFloats = (size_t)nb * nCh * bs;
    float* src = static_cast<float*>(std::aligned_alloc(64, (srcFloats * 4 + 63) / 64 * 64));
    for (size_t i = 0; i < srcFloats; ++i) {
        const uint32_t r = rnd();
        float x = ((float)(r & 0xFFFFu) - 32768.0f) / 26000.0f;           // some beyond full scale
        if ((r >> 16) % 97u == 0u) x = std::numeric_limits<float>::quiet_NaN();
        if ((r >> 16) % 101u == 0u) x = (r & 1u) ? INFINITY : -INFINITY;
        if ((r >> 16) % 89u == 0u) x = (r & 1u) ? 3e38f : -3e38f;
        src[i] = x;
    }
    const uint64_t stride = pp::stream_stride(valid, G, fmt);
    const size_t guard = 64, dstBytes = (size_t)nStreams * stride;
    unsigned char* dstAll = static_cast<unsigned char*>(std::aligned_alloc(64, (dstBytes + 2 * guard + 63) / 64 * 64));
    std::memset(dstAll, 0xA5, dstBytes + 2 * guard);
    unsigned char* dst = dstAll + guard;
    std::vector<uint8_t> writes(dstBytes, 0);
    std::vector<pp::ChannelStats> stats(nCh, pp::ChannelStats{0u, 0u, 0u});

    std::vector<uint16_t> rowBase(G);
    const uint32_t rowDwords = pp::row_bases(G, rowBase.data());
    const uint32_t ldsBytes = pp::lds_bytes(rowDwords, G);
    if (ldsBytes > 65536u) fail(T, "lds size", bs, G, fmt, nb, valid);
    const uint32_t tilesPerBlock = pp::tiles_per_block(bs, G), blocks = (valid + bs - 1) / bs;
    bool bad = false;
    auto ldsOk = [&](uint32_t off, uint32_t bytes) { if ((size_t)off + bytes > ldsBytes) { bad = true; return false; } return true; };

    for (uint32_t s = 0; s < nStreams; ++s)
        for (uint32_t bx = 0; bx < blocks * tilesPerBlock; ++bx) {
            std::vector<unsigned char> lds(ldsBytes, 0xEE);
            std::vector<uint8_t> rowWritten(rowDwords, 0);
            uint32_t* rows = reinterpret_cast<uint32_t*>(lds.data());
            unsigned char* image = lds.data() + pp::lds_image_offset(rowDwords);
            const uint32_t b = bx / tilesPerBlock, ti = bx % tilesPerBlock;
            const uint32_t n = pp::tile_valid(bs, G, b, ti, valid);
            if (n == 0u) continue;
            const uint32_t f0 = ti * pp::tile_frames(G);
            // ---- A ----
            const uint32_t chunks = pp::row_chunks(n, bs), items = G * chunks;
            const int64_t tTile = time0 + (int64_t)((uint64_t)b * bs + f0);
            for (uint32_t wave = 0; wave < pp::kWaves; ++wave)
                for (uint32_t item = wave; item < items; item += pp::kWaves) {
                    const uint32_t g = item / chunks, c = s * G + g;
                    const float* row = src + ((size_t)b * nCh + c) * bs + f0;
                    const uint32_t m = (uint32_t)(reinterpret_cast<uintptr_t>(row) >> 2) & 3u;
                    if (pp::row_quads(n, m) > chunks * 64u) bad = true;          // a quad no chunk covers
                    pp::ChannelStats acc{0u, 0u, 0u};
                    const uint32_t k0 = pp::channel_key(seed, c);
                    for (uint32_t lane = 0; lane < 64; ++lane) {
                        const uint32_t q = (item % chunks) * 64u + lane;
                        const int32_t first = pp::quad_first(q, m);
                        const bool whole = pp::quad_whole(first, n);
                        if (whole) {
                            if (reinterpret_cast<uintptr_t>(row + first) & 15u) bad = true;
                            T.wideLoads++;
                        }
                        for (int e = 0; e < 4; ++e) {
                            const int32_t f = first + e;
                            if (f < 0 || (uint32_t)f >= n) continue;
                            if (!whole) T.narrowLoads++;
                            const float x = row[f];
                            acc = pp::stats_fold(x, acc);
                            const float d = (dith && fmt != pp::F32) ? pp::dither(k0, tTile + f) : 0.0f;
                            const uint32_t at = rowBase[g] + (uint32_t)f;
                            if (at >= rowDwords || rowWritten[at]) { bad = true; continue; }
                            rowWritten[at] = 1;
                            rows[at] = pp::encode(fmt, x, d);
                        }
                    }
                    if (acc.peakBits > stats[c].peakBits) stats[c].peakBits = acc.peakBits;
                    stats[c].over += acc.over; stats[c].nonfinite += acc.nonfinite;
                }
            // ---- B ----
            const uint64_t c0 = pp::stretch_begin(bs, G, fmt, b, f0);
            const uint32_t head = pp::image_head(c0), total = n * G;
            for (uint32_t j0 = 0; j0 < total; j0 += 32u) {                 // a half-wave's read: 32 banks
                uint32_t seen = 0;
                for (uint32_t j = j0; j < total && j < j0 + 32u; ++j) {
                    const uint32_t bank = (rowBase[j % G] + j / G) & 31u;
                    if (G <= 32u && (seen & (1u << bank))) T.bankConflicts++;
                    seen |= 1u << bank;
                }
                T.halfWaveReads++;
            }
            for (uint32_t tid = 0; tid < pp::kThreads; ++tid) {
                uint32_t g = tid % G, f = tid / G;
                const uint32_t dg = pp::kThreads % G, df = pp::kThreads / G;
                for (uint32_t j = tid; j < total; j += pp::kThreads) {
                    if (g != j % G || f != j / G) bad = true;
                    const uint32_t at = rowBase[g] + f;
                    if (at >= rowDwords || !rowWritten[at]) { bad = true; break; }
                    const uint32_t code = rows[at], o = pp::image_offset(head, j, fmt);
                    if (!ldsOk(pp::lds_image_offset(rowDwords) + o, B) || o + B > pp::image_bytes(G)) break;
                    for (uint32_t k = 0; k < B; ++k) image[o + k] = (unsigned char)(code >> (8u * k));
                    g += dg; f += df;
                    if (g >= G) { g -= G; ++f; }
                }
            }
            // ---- C ----
            const uint32_t len = total * B, pieces = pp::piece_count(head, len);
            const size_t outOff = (size_t)s * stride + (size_t)(c0 - head);
            for (uint32_t p = 0; p < pieces; ++p) {
                if (16u * p + 16u > pp::image_bytes(G)) { bad = true; break; }
                uint32_t lo = 16u * p, hi = 16u * p + 16u;
                if (pp::piece_whole(p, head, len)) {
                    if ((outOff + lo) & 15u) bad = true;
                    T.wideStores++;
                } else {
                    lo = lo > head ? lo : head; hi = hi < head + len ? hi : head + len;
                    const uint32_t U = pp::store_unit(fmt);
                    if ((hi - lo) % U || ((outOff + lo) % U)) bad = true;
                    T.narrowStores += (hi - lo) / U;
                }
                for (uint32_t o = lo; o < hi; ++o) {
                    if (outOff + o >= dstBytes) { bad = true; break; }
                    dst[outOff + o] = image[o];
                    writes[outOff + o]++;
                }
            }
        }
    if (bad) fail(T, "schedule", bs, G, fmt, nb, valid);

    // the plain loop
    std::vector<unsigned char> ref(dstBytes, 0xA5);
    std::vector<pp::ChannelStats> refStats(nCh, pp::ChannelStats{0u, 0u, 0u});
    for (uint32_t c = 0; c < nCh; ++c)
        for (uint32_t fr = 0; fr < valid; ++fr) {
            const float x = src[((size_t)(fr / bs) * nCh + c) * bs + fr % bs];
            uint32_t u; std::memcpy(&u, &x, 4);
            uint32_t code = u;
            if (std::isfinite(x)) {
                const float a = std::fabs(x);
                float pk; std::memcpy(&pk, &refStats[c].peakBits, 4);
                if (a > pk) std::memcpy(&refStats[c].peakBits, &a, 4);
                if (a > 1.0f) refStats[c].over++;
            } else refStats[c].nonfinite++;
            if (fmt != pp::F32) {
                const uint32_t k0 = pp::hash32(seed ^ (c * 0x9E3779B9u));
                const float d = dith ? pp::dither(k0, time0 + fr) : 0.0f;
                code = (uint32_t)pp::quantise(x, fmt == pp::S16 ? 16u : 24u, d);
            }
            unsigned char* o = ref.data() + (size_t)(c / G) * stride + ((size_t)fr * G + c % G) * B;
            for (uint32_t k = 0; k < B; ++k) o[k] = (unsigned char)(code >> (8u * k));
        }
    bool ok = true;
    for (uint32_t s = 0; s < nStreams; ++s)
        for (uint64_t o = 0; o < stride; ++o) {
            const size_t at = (size_t)s * stride + o;
            const bool delivered = o < (uint64_t)valid * G * B;
            if (writes[at] != (delivered ? 1 : 0) || dst[at] != ref[at]) ok = false;
        }
    for (size_t i = 0; i < guard; ++i) if (dstAll[i] != 0xA5 || dstAll[guard + dstBytes + i] != 0xA5) ok = false;
    for (uint32_t c = 0; c < nCh; ++c)
        if (stats[c].peakBits != refStats[c].peakBits || stats[c].over != refStats[c].over || stats[c].nonfinite != refStats[c].nonfinite) ok = false;
    if (!ok) fail(T, "bytes / stats", bs, G, fmt, nb, valid);
    std::free(src); std::free(dstAll);
}

int main() {
    Totals T;
    const uint32_t sizes[] = {32u, 341u, 350u, 512u}, groups[] = {1u, 2u, 3u, 6u, 8u}, formats[] = {pp::S16, pp::S24, pp::F32}, sets[] = {1u, 3u};
    for (uint32_t bs : sizes) for (uint32_t G : groups) for (uint32_t fmt : formats) for (uint32_t nb : sets) {
        const uint32_t cut = bs > 37u ? 37u : bs - 1u;
        run_case(T, bs, G, fmt, nb, nb * bs, true);
        run_case(T, bs, G, fmt, nb, (nb - 1u) * bs + cut, (G & 1u) != 0u);
    }
    // a wide group (rows on an odd stride, tiles of 124 frames) and the widest
    run_case(T, 350u, 33u, pp::S24, 2u, 350u + 37u, true);
    run_case(T, 64u, 1024u, pp::S16, 1u, 37u, true);
    // conflict-free skews for EVERY group up to 32 (any window of 32 samples that starts at a multiple of 32)
    long skewConflicts = 0;
    for (uint32_t G = 1; G <= 32u; ++G) {
        std::vector<uint16_t> rb(G);
        pp::row_bases(G, rb.data());
        for (uint32_t w = 0; w < G; ++w) {
            uint32_t seen = 0;
            for (uint32_t j = 32u * w; j < 32u * w + 32u; ++j) {
                const uint32_t bank = (rb[j % G] + j / G) & 31u;
                if (seen & (1u << bank)) skewConflicts++;
                seen |= 1u << bank;
            }
        }
    }

    // the edge vector, dither off
    const float edge[] = {0.0f, 1.0f, -1.0f, 0.5f / 32768.0f, 1.5f / 32768.0f, -0.5f / 32768.0f, 2.5f / 32768.0f, 3e38f, -3e38f,
                          std::numeric_limits<float>::quiet_NaN(), INFINITY, 0.99999f};
    std::printf("{\"edge_s16\":[");
    for (size_t i = 0; i < sizeof(edge) / 4; ++i) std::printf("%s%d", i ? "," : "", pp::quantise(edge[i], 16u, 0.0f));
    std::printf("],\"edge_s24\":[");
    for (size_t i = 0; i < sizeof(edge) / 4; ++i) std::printf("%s%d", i ? "," : "", pp::quantise(edge[i], 24u, 0.0f));
    // 4096 dithered samples, channel 3, seed 12345, t = 2^32 - 2048 + i, x = ((37 i) mod 201 - 100) / 128
    const uint32_t k0 = pp::channel_key(12345u, 3u);
    for (uint32_t bits : {16u, 24u}) {
        std::printf("],\"dither_s%u\":[", bits);
        for (uint32_t i = 0; i < 4096u; ++i) {
            const float x = (float)((int)((37u * i) % 201u) - 100) / 128.0f;
            std::printf("%s%d", i ? "," : "", pp::quantise(x, bits, pp::dither(k0, ((int64_t)1 << 32) - 2048 + (int64_t)i)));
        }
    }
    std::printf("],\"cases\":%ld,\"failures\":%ld,\"wide_stores\":%ld,\"narrow_stores\":%ld,\"wide_loads\":%ld,\"narrow_loads\":%ld,"
                "\"half_wave_reads\":%ld,\"bank_conflicts\":%ld,\"skew_conflicts\":%ld,\"ok\":%s}\n",
                T.cases, T.failures, T.wideStores, T.narrowStores, T.wideLoads, T.narrowLoads, T.halfWaveReads, T.bankConflicts, skewConflicts,
                T.failures == 0 ? "true" : "false");
    return T.failures == 0 ? 0 : 1;
}
