// flac_in_md5_host.cpp — elementary_amd/csrc/flac_in_md5.h compiled for the host: the kernel's walk of a job emulated lane by lane
// (flac_md5_wave.h's steps: 64 lanes gather a chunk's words, the chain runs over its blocks, the lanes write the tail back) against
// the scalar twin (run_job) and against RFC 1321 over the plainly packed bytes, for streams that are decoded set by set with the
// boundary frames decoded twice (flac_in_md5::advance decides what is new). The scratch of every set is exactly as large as its
// covered frames, so a read outside it is the sanitizers' to find. Prints one JSON line.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "flac_in_md5.h"

namespace fm = flac_md5;
namespace fi = flac_in_md5;

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// the kernel's steps, a lane at a time
static void lanes_job(fm::Record& rec, const int32_t* scratch, const fi::Job& job, uint32_t G, uint32_t bits, uint8_t* digest) {
    if (job.count == 0u && job.finish == 0u) return;
    const int32_t* rows = scratch + job.base;
    const uint32_t stride = job.stride;
    auto codes = [rows, stride](uint32_t g, uint32_t f) { return rows[(size_t)g * stride + f]; };
    const fm::Job j = fm::make_job(rec.bytes, G, job.first, job.count, bits, job.finish != 0u);
    std::vector<uint32_t> m(fm::kChunkWords);
    for (fm::Chunk c = fm::first_chunk(j);; fm::next_chunk(j, c)) {
        for (uint32_t lane = 0; lane < 64u; ++lane)
            for (uint32_t w = lane; w < 16u * c.blocks; w += 64u) m[w] = fm::chunk_word(j, c, rec.tail, codes, 4u * w);
        for (uint32_t b = 0; b < c.blocks; ++b) {
            uint32_t x[64], p = rec.h[0], q = rec.h[1], r = rec.h[2], t = rec.h[3];
            for (uint32_t lane = 0; lane < 64u; ++lane) x[lane] = fm::k_of(lane) + m[16u * b + fm::word_of(lane)];
            for (uint32_t i = 0; i < 64u; ++i) fm::round(i, x[i], p, q, r, t);
            rec.h[0] += p; rec.h[1] += q; rec.h[2] += r; rec.h[3] += t;
        }
        if (!fm::last_chunk(j, c)) continue;
        const uint32_t n = fm::leftover(j);
        uint8_t keep[64] = {};
        for (uint32_t lane = 0; lane < n; ++lane) keep[lane] = (uint8_t)fm::chunk_byte(j, c, rec.tail, codes, 64u * c.blocks + lane);
        for (uint32_t lane = 0; lane < n; ++lane) rec.tail[lane] = keep[lane];
        break;
    }
    rec.bytes += (uint64_t)job.count * j.FB;
    if (job.finish) fm::put_digest(rec.h, digest);
}

// RFC 1321 over a byte string, padded here
static void plain_md5(const std::vector<uint8_t>& msg, uint8_t digest[16]) {
    std::vector<uint8_t> p(msg);
    p.push_back(0x80u);
    while (p.size() % 64u != 56u) p.push_back(0u);
    const uint64_t bitsLen = (uint64_t)msg.size() * 8u;
    for (uint32_t i = 0; i < 8u; ++i) p.push_back((uint8_t)(bitsLen >> (8u * i)));
    fm::Record r; fm::init(r);
    for (size_t at = 0; at < p.size(); at += 64u) {
        uint32_t m[16];
        for (uint32_t w = 0; w < 16u; ++w) m[w] = p[at + 4u * w] | (p[at + 4u * w + 1u] << 8) | (p[at + 4u * w + 2u] << 16) | ((uint32_t)p[at + 4u * w + 3u] << 24);
        fm::block(r.h, m);
    }
    fm::put_digest(r.h, digest);
}

int main() {
    unsigned cases = 0, failures = 0, twice = 0, gaps = 0;
    const uint32_t sizes[] = {8u, 12u, 16u, 20u, 24u}, groups[] = {1u, 2u, 3u, 8u};
    for (uint32_t bits : sizes) for (uint32_t G : groups) for (uint32_t fb : {16u, 192u}) for (uint32_t setLen : {64u, 100u, 512u, 5000u}) {
        const uint32_t B = (bits + 7u) / 8u;
        const uint64_t total = 11u * fb + (fb == 16u ? 1u : 17u) + (rnd() % 3u) * fb;
        std::vector<std::vector<int32_t>> x(G, std::vector<int32_t>(total));
        const int32_t lim = 1 << (bits - 1u);
        for (auto& row : x) for (auto& v : row) v = (int32_t)(rnd() % (2u * (uint32_t)lim)) - lim;
        x[0][0] = -lim; x[G - 1u][total - 1u] = lim - 1; x[0][total / 2u] = -1;
        std::vector<uint8_t> msg;
        for (uint64_t t = 0; t < total; ++t) for (uint32_t g = 0; g < G; ++g) for (uint32_t k = 0; k < B; ++k) msg.push_back((uint8_t)((uint32_t)x[g][t] >> (8u * k)));
        uint8_t want[16], gotLanes[16] = {}, gotTwin[16] = {};
        plain_md5(msg, want);
        fm::Record a, b; fm::init(a); fm::init(b);
        fi::Slot slot{};
        // set by set: samples [p0, p1) are asked for, the covering frames [c0, c1) are decoded into a scratch of exactly their size,
        // which starts at a base of its own as a second stream's would
        for (uint64_t p0 = 0; p0 < total + setLen; p0 += setLen) {
            if (p0 >= total) break;
            const uint64_t p1 = p0 + setLen < total ? p0 + setLen : total;
            const uint64_t c0 = p0 / fb * fb, c1 = ((p1 - 1u) / fb + 1u) * fb < total ? ((p1 - 1u) / fb + 1u) * fb : total;
            const uint32_t covered = (uint32_t)(c1 - c0), base = 7u;
            std::vector<int32_t> scratch((size_t)base + (size_t)G * covered);
            for (uint32_t g = 0; g < G; ++g) for (uint32_t f = 0; f < covered; ++f) scratch[base + (size_t)g * covered + f] = x[g][c0 + f];
            uint64_t lo = 0; bool finish = false;
            if (c0 < slot.hashedTo) ++twice;
            if (!fi::advance(slot, bits, G, total, c0, c1, lo, finish)) continue;
            fi::Job job{};
            job.base = base; job.stride = covered; job.first = (uint32_t)(lo - c0); job.count = (uint32_t)(c1 - lo); job.finish = finish ? 1u : 0u;
            lanes_job(a, scratch.data(), job, G, bits, gotLanes);
            fi::run_job(b, scratch.data(), job, G, bits, gotTwin);
        }
        ++cases;
        bool ok = slot.state == fi::kComplete && slot.hashedTo == total;
        for (uint32_t i = 0; i < 16u; ++i) ok = ok && gotLanes[i] == want[i] && gotTwin[i] == want[i];
        if (!ok) { ++failures; std::fprintf(stderr, "bits %u G %u frame %u set %u: digest or state wrong\n", bits, G, fb, setLen); }
        // the rule's refusals: a gap breaks the slot for good, another stream under a complete one too
        fi::Slot s2{}; uint64_t lo = 0; bool fin = false;
        (void)fi::advance(s2, bits, G, total, 0u, fb, lo, fin);
        if (fi::advance(s2, bits, G, total, 2u * fb, 3u * fb, lo, fin) || s2.state != fi::kBroken || fi::advance(s2, bits, G, total, fb, 2u * fb, lo, fin)) ++failures; else ++gaps;
        if (fi::advance(slot, bits, G, total + 1u, 0u, fb, lo, fin) || slot.state != fi::kBroken) ++failures;
    }
    std::printf("{\"ok\": %s, \"cases\": %u, \"failures\": %u, \"decoded_twice\": %u, \"gaps\": %u}\n", failures ? "false" : "true", cases, failures, twice, gaps);
    return failures ? 1 : 0;
}
