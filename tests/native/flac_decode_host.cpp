// Host emulation of the FLAC input kernels (elementary_amd/csrc/flac_decode.hip) with the header's own lane functions: per frame the
// parse lane, the restore waves (the chunked prefix sums with carry, lane for lane), the CRC-16 from lane chunks, the stereo undo and
// the store kernel's 16-byte pieces — against decode_host() / image_host(), the scalar twin, code for code and byte for byte.
//
//   flac_decode_host <corpus file>
// The file: u32 cases; per case u32 channels, bps, block size, strict, u64 bytes, the bytes. A strict case has to index and decode;
// any other (the corrupt corpus) has to end in a reason or a decode, the same one on both sides, without touching anything outside its
// buffers — which is what the sanitizer build of this program checks.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "flac_decode.h"

namespace fd = flac_decode;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++fails <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// the restore kernel's wave c, lane for lane: 64 lanes in lockstep, positions lane, lane + 64, ...
static void wave_restore(const fd::Sub& sub, int32_t* s, uint32_t n) {
    uint32_t* u = reinterpret_cast<uint32_t*>(s);
    const uint32_t order = sub.order, wasted = sub.wasted;
    if (sub.kind == fd::CONSTANT) {
        const uint32_t v = n ? u[0] << wasted : 0u;
        for (uint32_t lane = 0; lane < 64u; ++lane) for (uint32_t i = lane; i < n; i += 64u) u[i] = v;
    } else if (sub.kind == fd::VERBATIM || (sub.kind == fd::FIXED && order == 0u)) {
        for (uint32_t lane = 0; lane < 64u; ++lane) for (uint32_t i = lane; i < n; i += 64u) u[i] <<= wasted;
    } else if (sub.kind == fd::FIXED) {
        const uint32_t s0 = u[0], s1 = order > 1u ? u[1] : 0u, s2 = order > 2u ? u[2] : 0u, s3 = order > 3u ? u[3] : 0u;
        for (uint32_t p = order; p >= 1u; --p) {
            const uint32_t seed = fd::fixed_seed(s0, s1, s2, s3, p), sh = p == 1u ? wasted : 0u;
            uint32_t carry = 0u;
            for (uint32_t base = 0; base < n; base += 64u) {
                uint32_t v[64], up[64];
                for (uint32_t lane = 0; lane < 64u; ++lane) {
                    const uint32_t i = base + lane;
                    v[lane] = i < n && i + 1u >= p ? (i + 1u == p ? seed : u[i]) : 0u;
                }
                for (uint32_t o = 1u; o < 64u; o <<= 1) {      // __shfl_up by o, added where lane >= o
                    for (uint32_t lane = 0; lane < 64u; ++lane) up[lane] = lane >= o ? v[lane - o] : v[lane];
                    for (uint32_t lane = 0; lane < 64u; ++lane) if (lane >= o) v[lane] += up[lane];
                }
                for (uint32_t lane = 0; lane < 64u; ++lane) {
                    const uint32_t i = base + lane;
                    v[lane] += carry;
                    if (i < n && i + 1u >= p) u[i] = v[lane] << sh;
                }
                carry = v[63];
            }
        }
    } else {
        for (uint32_t i = order; i < n; ++i) s[i] = fd::lpc_sample(sub, s, i);
        if (wasted) for (uint32_t i = 0; i < n; ++i) s[i] = fd::unwaste(s[i], wasted);
    }
}

// one frame the way the kernels decode it: out[c * stride + [0, n)]; the reason
static uint32_t kernel_frame(const uint8_t* f, uint32_t len, uint32_t G, uint32_t bps, uint32_t n, int32_t* out, size_t stride) {
    fd::Sub subs[fd::kMaxChannels];
    uint32_t assignment;
    const uint32_t parsed = fd::parse_lane(f, len, G, bps, n, subs, out, stride, &assignment);
    const uint32_t threads = 64u * G, total = len >= 2u ? len - 2u : 0u;
    uint32_t crc = 0;
    for (uint32_t t = 0; t < threads; ++t) crc ^= fd::lane_crc(f, total, t, threads);
    uint32_t reason = parsed;
    if (len < 2u) reason = fd::BITS_MISSING;
    else if (crc != (((uint32_t)f[total] << 8) | f[total + 1u])) reason = fd::BAD_CRC;
    if (reason != fd::OK) return reason;
    for (uint32_t c = 0; c < G; ++c) wave_restore(subs[c], out + c * stride, n);
    bool ok = true;
    if (assignment != fd::INDEPENDENT) for (uint32_t i = 0; i < n; ++i) ok = fd::stereo_pair(assignment, bps, out[i], out[stride + i]) && ok;
    else for (uint32_t c = 0; c < G; ++c) for (uint32_t i = 0; i < n; ++i) ok = fd::in_range(out[c * stride + i], bps) && ok;
    return ok ? fd::OK : fd::OUT_OF_RANGE;
}

static void run_case(uint32_t id, const std::vector<uint8_t>& data, uint32_t G, uint32_t bps, uint32_t blockSize, bool strict) {
    size_t entries = 0;
    std::vector<uint64_t> off(data.size() / 6u + 2u), first(off.size());
    const uint32_t ri = fd::index_host(data.data(), data.size(), G, bps, blockSize, off.data(), first.data(), off.size(), &entries);
    CHECK(!strict || ri == fd::OK, "case %u: index answers %u", id, ri);
    if (ri == fd::OK && entries >= 2u && entries <= off.size()) {
        const size_t frames = entries - 1u, total = (size_t)first[frames];
        // a second pass with a small capacity needs the same entries
        size_t again = 0;
        uint64_t o2[2], f2[2];
        (void)fd::index_host(data.data(), data.size(), G, bps, blockSize, o2, f2, 2, &again);
        CHECK(again == entries && o2[0] == off[0], "case %u: the index depends on the capacity", id);
        std::vector<int32_t> twin((size_t)G * (total + 1u)), mine((size_t)G * (total + 1u), 0);
        int32_t* rows[fd::kMaxChannels];
        for (uint32_t c = 0; c < G; ++c) rows[c] = twin.data() + (size_t)c * (total + 1u);
        size_t bad = 0;
        const uint32_t rt = fd::decode_host(data.data(), off.data(), first.data(), frames, G, bps, 0, total, rows, &bad);
        CHECK(!strict || rt == fd::OK, "case %u: decode_host answers %u at frame %zu", id, rt, bad);
        uint32_t rk = fd::OK;
        size_t badK = 0;
        for (size_t j = 0; j < frames && rk == fd::OK; ++j) {
            const uint32_t n = (uint32_t)(first[j + 1] - first[j]);
            rk = kernel_frame(data.data() + off[j], (uint32_t)(off[j + 1] - off[j]), G, bps, n, mine.data() + first[j], total + 1u);
            badK = j;
        }
        CHECK(rk == rt && (rk == fd::OK || badK == bad), "case %u: the lanes answer %u at frame %zu, the twin %u at %zu", id, rk, badK, rt, bad);
        if (rk == fd::OK && rt == fd::OK) {
            CHECK(mine == twin, "case %u: the lanes' codes differ from the twin's", id);
            // a range that starts and ends inside frames, and runs past the end: the twin's cut, and the store kernel's pieces
            const uint64_t p0 = total / 3u;
            const size_t cnt = total - (size_t)p0 + 5u;
            std::vector<int32_t> part((size_t)G * cnt);
            int32_t* prow[fd::kMaxChannels];
            for (uint32_t c = 0; c < G; ++c) prow[c] = part.data() + (size_t)c * cnt;
            CHECK(fd::decode_host(data.data(), off.data(), first.data(), frames, G, bps, p0, cnt, prow, nullptr) == fd::OK, "case %u: the cut fails", id);
            for (uint32_t c = 0; c < G; ++c)
                for (size_t i = 0; i < cnt; ++i)
                    CHECK(prow[c][i] == (p0 + i < total ? rows[c][p0 + i] : 0), "case %u: the cut differs at %zu", id, i);
            const size_t stride = (size_t)pcm_pack::stream_stride(cnt, G, fd::image_format(bps));
            std::vector<uint8_t> image(stride, 0xAA), want(stride, 0);
            fd::image_host(bps, G, prow, cnt, want.data());
            for (uint32_t piece = 0; piece < stride / 16u; ++piece)
                fd::image_piece(bps, G, (uint32_t)cnt, (uint32_t)(total - p0), piece,
                                [&](uint32_t g, uint32_t frame) { return rows[g][p0 + frame]; }, image.data() + 16u * piece);
            CHECK(image == want, "case %u: the image's pieces differ", id);
        }
    }
    // the blob as one frame of 16 samples, whatever it is: a reason or a decode, the same on both sides
    std::vector<int32_t> a((size_t)G * 16u, 0), b((size_t)G * 16u, 0);
    const uint32_t len = (uint32_t)(data.size() < 0x7FFFFFFFu ? data.size() : 0x7FFFFFFFu);
    const uint32_t r1 = fd::decode_frame_host(data.data(), len, G, bps, 16u, a.data(), 16u), r2 = kernel_frame(data.data(), len, G, bps, 16u, b.data(), 16u);
    CHECK(r1 == r2 && (r1 != fd::OK || a == b), "case %u: as one frame the twin answers %u, the lanes %u", id, r1, r2);
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: flac_decode_host <corpus file>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    uint32_t cases = 0;
    if (std::fread(&cases, 4, 1, f) != 1) return 2;
    for (uint32_t k = 0; k < cases; ++k) {
        uint32_t head[4];
        uint64_t bytes = 0;
        if (std::fread(head, 4, 4, f) != 4 || std::fread(&bytes, 8, 1, f) != 1) { std::printf("short corpus file\n"); return 2; }
        // (an exact-size heap block: the sanitizers see every byte read behind a frame's end)
        std::vector<uint8_t> data((size_t)bytes);
        if (bytes && std::fread(data.data(), 1, (size_t)bytes, f) != bytes) { std::printf("short corpus file\n"); return 2; }
        data.shrink_to_fit();
        run_case(k, data, head[0], head[1], head[2], head[3] != 0u);
    }
    std::fclose(f);
    std::printf("%u cases, %d failures\n", cases, fails);
    return fails ? 1 : 0;
}
