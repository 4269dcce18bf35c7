// pcm_unpack_host.cpp — the PCM unpack kernel's tile and lane schedule on the CPU (elementary_amd/csrc/pcm_unpack.h and pcm_pack.h, the
// headers pcm_unpack.hip takes every index from): 256 emulated threads per tile run the three stages in the kernel's order over block
// sizes 32, 341, 350 and 512, G = 1, 2, 3, 6 and 8, all three formats, sets of 1 and 3 blocks, whole and with the last block cut at 37
// frames, and sets whose last block lies wholly behind the valid frames. The destination is poisoned first. Checked: every float of
// every row the set owns written exactly once and nothing else touched (a channel row that belongs to nobody, guard bands), the bits
// those of the scalar loop with zeros behind the cut, every 16-byte load aligned and inside its stream's stride, every 16-byte store
// aligned, every LDS access inside the launch's LDS, stage B's half-wave writes and stage C's half-wave reads free of bank conflicts.
// The last line is JSON; it also carries the decoded bits of all 65 536 s16 codes, of 4096 strided s24 codes and of a vector of
// float32 bit patterns for the Python side to compare with its own restatement.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pcm_unpack.h"

namespace pp = pcm_pack;
namespace pu = pcm_unpack;

static uint32_t rng = 0x7654321u;
static uint32_t rnd() { rng = rng * 1664525u + 1013904223u; return rng >> 8; }

struct Totals { long cases = 0, failures = 0, wideLoads = 0, wideStores = 0, narrowStores = 0, halfWaveWrites = 0, writeConflicts = 0,
                halfWaveReads = 0, readConflicts = 0, zeroFloats = 0; };

static void fail(Totals& t, const char* what, uint32_t bs, uint32_t G, uint32_t fmt, uint32_t nb, uint32_t valid) {
    if (t.failures < 20) std::fprintf(stderr, "FAIL %s: bs %u G %u fmt %u blocks %u valid %u\n", what, bs, G, fmt, nb, valid);
    t.failures++;
}

static const uint32_t kPoison = 0xA5A5A5A5u;

static void run_case(Totals& T, uint32_t bs, uint32_t G, uint32_t fmt, uint32_t nb, uint32_t valid) {
    T.cases++;
    const uint32_t nStreams = 2, nCh = nStreams * G + 1u, B = pp::sample_bytes(fmt);      // (the last channel row belongs to nobody)
    const uint64_t stride = pp::stream_stride(valid, G, fmt);
    const size_t srcBytes = (size_t)nStreams * stride;
    // exactly the staging buffer's bytes: a load beyond them is the sanitizer's to catch
    unsigned char* src = static_cast<unsigned char*>(std::aligned_alloc(64, (srcBytes + 63) / 64 * 64));
    for (size_t i = 0; i < srcBytes; ++i) src[i] = (unsigned char)rnd();
    if (fmt == pp::F32)                                                   // some NaNs (with payloads), infinities and denormals
        for (size_t i = 0; i + 4 <= srcBytes; i += 4) {
            const uint32_t r = rnd();
            uint32_t u = 0;
            if (r % 53u == 0u) u = 0x7F800001u | (r & 0x807FFFFEu);
            else if (r % 59u == 0u) u = (r & 0x80000000u) | 0x7F800000u;
            else if (r % 61u == 0u) u = r & 0x807FFFFFu;
            if (u) std::memcpy(src + i, &u, 4);
        }
    const size_t dstFloats = (size_t)nb * nCh * bs, guard = 16;
    uint32_t* dstAll = static_cast<uint32_t*>(std::aligned_alloc(64, ((dstFloats + 2 * guard) * 4 + 63) / 64 * 64));
    for (size_t i = 0; i < dstFloats + 2 * guard; ++i) dstAll[i] = kPoison;
    uint32_t* dst = dstAll + guard;                                       // (16 floats: the destination stays 64-byte aligned)
    std::vector<uint8_t> writes(dstFloats, 0);

    std::vector<uint16_t> rowBase(G);
    const uint32_t rowDwords = pp::row_bases(G, rowBase.data());
    const uint32_t ldsBytes = pp::lds_bytes(rowDwords, G);
    if (ldsBytes > 65536u) fail(T, "lds size", bs, G, fmt, nb, valid);
    const uint32_t tilesPerBlock = pp::tiles_per_block(bs, G);
    bool bad = false;

    for (uint32_t s = 0; s < nStreams; ++s)
        for (uint32_t bx = 0; bx < nb * tilesPerBlock; ++bx) {
            std::vector<unsigned char> lds(ldsBytes, 0xEE);
            std::vector<uint8_t> rowWritten(rowDwords, 0);
            uint32_t* rows = reinterpret_cast<uint32_t*>(lds.data());
            const uint32_t imageAt = pp::lds_image_offset(rowDwords);
            unsigned char* image = lds.data() + imageAt;
            const uint32_t b = bx / tilesPerBlock, ti = bx % tilesPerBlock;
            const uint32_t n = pp::tile_valid(bs, G, b, ti, valid), span = pu::tile_span(bs, G, ti);
            const uint32_t f0 = ti * pp::tile_frames(G);
            if (span == 0u || n > span) { bad = true; continue; }
            if (n != 0u) {
                // ---- A ----
                const uint64_t c0 = pp::stretch_begin(bs, G, fmt, b, f0);
                const uint32_t head = pp::image_head(c0), total = n * G, len = total * B, pieces = pp::piece_count(head, len);
                const size_t inOff = (size_t)s * stride + (size_t)(c0 - head);
                for (uint32_t p = 0; p < pieces; ++p) {
                    const size_t at = inOff + 16u * p;
                    if ((at & 15u) || at + 16u > ((size_t)s + 1u) * stride || 16u * p + 16u > pp::image_bytes(G) || imageAt + 16u * p + 16u > ldsBytes) { bad = true; break; }
                    std::memcpy(image + 16u * p, src + at, 16);
                    T.wideLoads++;
                }
                // ---- B ----
                for (uint32_t j0 = 0; j0 < total; j0 += 32u) {             // a half-wave's write: 32 banks
                    uint32_t seen = 0;
                    for (uint32_t j = j0; j < total && j < j0 + 32u; ++j) {
                        const uint32_t bank = (rowBase[j % G] + j / G) & 31u;
                        if (G <= 32u && (seen & (1u << bank))) T.writeConflicts++;
                        seen |= 1u << bank;
                    }
                    T.halfWaveWrites++;
                }
                for (uint32_t tid = 0; tid < pp::kThreads; ++tid) {
                    uint32_t g = tid % G, f = tid / G;
                    const uint32_t dg = pp::kThreads % G, df = pp::kThreads / G;
                    for (uint32_t j = tid; j < total; j += pp::kThreads) {
                        if (g != j % G || f != j / G) bad = true;
                        const uint32_t o = pp::image_offset(head, j, fmt), at = rowBase[g] + f;
                        if (o < head || o + B > head + len || at >= rowDwords || rowWritten[at]) { bad = true; break; }
                        rowWritten[at] = 1;
                        rows[at] = pu::decode_bits(fmt, pu::load_raw(fmt, image + o));
                        g += dg; f += df;
                        if (g >= G) { g -= G; ++f; }
                    }
                }
            }
            // ---- C ----
            const uint32_t chunks = pp::row_chunks(span, bs), items = G * chunks;
            for (uint32_t wave = 0; wave < pp::kWaves; ++wave)
                for (uint32_t item = wave; item < items; item += pp::kWaves) {
                    const uint32_t g = item / chunks, c = s * G + g;
                    const size_t rowAt = ((size_t)b * nCh + c) * bs + f0;
                    const uint32_t m = (uint32_t)(reinterpret_cast<uintptr_t>(dst + rowAt) >> 2) & 3u;
                    if (pp::row_quads(span, m) > chunks * 64u) bad = true;          // a quad no chunk covers
                    for (uint32_t e = 0; e < 4u; ++e)                            // read instruction e: the banks of each half-wave
                        for (uint32_t halfWave = 0; halfWave < 2u; ++halfWave) {
                            uint32_t seen = 0;
                            bool any = false;
                            for (uint32_t lane = 32u * halfWave; lane < 32u * halfWave + 32u; ++lane) {
                                const int32_t f = pp::quad_first((item % chunks) * 64u + lane, m) + (int32_t)pu::quad_slot(e, lane);
                                if (f < 0 || (uint32_t)f >= n) continue;
                                const uint32_t bank = (rowBase[g] + (uint32_t)f) & 31u;
                                if (seen & (1u << bank)) T.readConflicts++;
                                seen |= 1u << bank; any = true;
                            }
                            if (any) T.halfWaveReads++;
                        }
                    for (uint32_t lane = 0; lane < 64u; ++lane) {
                        const uint32_t q = (item % chunks) * 64u + lane;
                        const int32_t first = pp::quad_first(q, m);
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
                        const bool whole = pp::quad_whole(first, span);
                        if (whole) {
                            if (reinterpret_cast<uintptr_t>(dst + rowAt + first) & 15u) bad = true;
                            T.wideStores++;
                        }
                        for (int32_t x = 0; x < 4; ++x) {
                            const int32_t f = first + x;
                            if (f < 0 || (uint32_t)f >= span) continue;
                            if (!whole) T.narrowStores++;
                            if (rowAt + (size_t)f >= dstFloats) { bad = true; continue; }
                            dst[rowAt + f] = v[x];
                            writes[rowAt + f]++;
                        }
                    }
                }
        }
    if (bad) fail(T, "schedule", bs, G, fmt, nb, valid);

    // the scalar loop, block by block as the engine's host path runs it: frames [n, bs) of every row are zero
    std::vector<uint32_t> ref(dstFloats, kPoison);
    std::vector<float> blockRows((size_t)nStreams * G * bs);
    for (uint32_t b = 0; b < nb; ++b) {
        const size_t fb = (size_t)b * bs;
        const size_t n = fb >= valid ? 0 : (valid - fb < bs ? valid - fb : bs);
        const unsigned char* sp[2] = {src + fb * G * B, src + stride + fb * G * B};
        for (float& x : blockRows) x = 123.0f;
        pu::unpack_host(fmt, G, nStreams, sp, n, blockRows.data(), bs, bs);
        for (uint32_t c = 0; c < nStreams * G; ++c) std::memcpy(&ref[((size_t)b * nCh + c) * bs], &blockRows[(size_t)c * bs], bs * 4);
    }
    bool ok = true;
    for (size_t i = 0; i < dstFloats; ++i) {
        const bool owned = (i / bs) % nCh != nCh - 1u;
        if (writes[i] != (owned ? 1 : 0) || dst[i] != ref[i]) ok = false;
        if (owned && ((i / bs) / nCh) * (size_t)bs + i % bs >= valid) { if (dst[i] != 0u) ok = false; T.zeroFloats++; }
    }
    for (size_t i = 0; i < guard; ++i) if (dstAll[i] != kPoison || dstAll[guard + dstFloats + i] != kPoison) ok = false;
    if (!ok) fail(T, "floats", bs, G, fmt, nb, valid);
    std::free(src); std::free(dstAll);
}

int main() {
    Totals T;
    const uint32_t sizes[] = {32u, 341u, 350u, 512u}, groups[] = {1u, 2u, 3u, 6u, 8u}, formats[] = {pp::S16, pp::S24, pp::F32}, sets[] = {1u, 3u};
    for (uint32_t bs : sizes) for (uint32_t G : groups) for (uint32_t fmt : formats) for (uint32_t nb : sets) {
        const uint32_t cut = bs > 37u ? 37u : bs - 1u;
        run_case(T, bs, G, fmt, nb, nb * bs);
        run_case(T, bs, G, fmt, nb, (nb - 1u) * bs + cut);
    }
    // the last block of the set only fills up a host block: wholly zero
    for (uint32_t fmt : formats) { run_case(T, 350u, 3u, fmt, 3u, 350u + 37u); run_case(T, 512u, 2u, fmt, 2u, 512u); }
    // a wide group (rows on an odd stride, tiles of 124 frames) and the widest
    run_case(T, 350u, 33u, pp::S24, 2u, 350u + 37u);
    run_case(T, 64u, 1024u, pp::S16, 1u, 37u);
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

    // decode: the bits of every s16 code (index = code + 32768), of the s24 codes -2^23 + 4097 i (i < 4096: both extremes) and of
    // some float32 bit patterns
    std::printf("{\"s16\":[");
    for (int32_t v = -32768; v <= 32767; ++v) std::printf("%s%u", v > -32768 ? "," : "", pu::decode_bits(pp::S16, (uint32_t)v & 0xFFFFu));
    std::printf("],\"s24\":[");
    for (int32_t i = 0; i < 4096; ++i) std::printf("%s%u", i ? "," : "", pu::decode_bits(pp::S24, (uint32_t)(-8388608 + 4097 * i) & 0xFFFFFFu));
    const uint32_t patterns[] = {0x00000000u, 0x80000000u, 0x3F800000u, 0xBF800000u, 0x7F800000u, 0xFF800000u, 0x7FC00000u, 0xFFC00001u,
                                 0x7F800001u, 0x7FA5A5A5u, 0xFFFFFFFFu, 0x00000001u, 0x807FFFFFu, 0x00800000u, 0x7F7FFFFFu, 0x3EAAAAABu};
    std::printf("],\"f32_in\":[");
    for (size_t i = 0; i < sizeof(patterns) / 4; ++i) std::printf("%s%u", i ? "," : "", patterns[i]);
    std::printf("],\"f32_out\":[");
    {   // through the scalar loop, one stream of 4 channels, rows padded to 8 frames
        const size_t count = sizeof(patterns) / 4, frames = count / 4;
        const unsigned char* sp[1] = {reinterpret_cast<const unsigned char*>(patterns)};
        std::vector<float> rows(4 * 8, 5.0f);
        pu::unpack_host(pp::F32, 4u, 1u, sp, frames, rows.data(), 8, 8);
        for (size_t i = 0; i < count; ++i) { uint32_t u; std::memcpy(&u, &rows[(i % 4) * 8 + i / 4], 4); std::printf("%s%u", i ? "," : "", u); }
        for (size_t g = 0; g < 4; ++g) for (size_t f = frames; f < 8; ++f) if (rows[g * 8 + f] != 0.0f) T.failures++;
    }
    std::printf("],\"cases\":%ld,\"failures\":%ld,\"wide_loads\":%ld,\"wide_stores\":%ld,\"narrow_stores\":%ld,\"half_wave_writes\":%ld,"
                "\"write_conflicts\":%ld,\"half_wave_reads\":%ld,\"read_conflicts\":%ld,\"skew_conflicts\":%ld,\"zero_floats\":%ld,\"ok\":%s}\n",
                T.cases, T.failures, T.wideLoads, T.wideStores, T.narrowStores, T.halfWaveWrites, T.writeConflicts, T.halfWaveReads,
                T.readConflicts, skewConflicts, T.zeroFloats, T.failures == 0 ? "true" : "false");
    return T.failures == 0 ? 0 : 1;
}
