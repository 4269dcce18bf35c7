// flac_md5.h — the STREAMINFO MD5 of FLAC delivery (option "flac_md5"; flac_md5.hip, engine_flac.cpp): RFC 1321 over the bytes
// process_blocks_pcm would deliver for the stream in s16 / s24 — for frame f, then channel g, the low B = (bits + 7) / 8 bytes of the
// two's-complement code, little-endian (delivery: 16 / 24 bits; the input side, flac_in_md5.h, walks the same schedule at 8 .. 24). One Record per stream carries the digest from launch set to launch set: the chaining value,
// the byte count and the bytes behind the last whole 64-byte block.
//
// MD5 is a serial chain of 64-byte blocks inside one stream; what is parallel is the gather of the message words and, per block, the
// 64 sums K[i] + M[g(i)]. An update is therefore laid out as a Job cut into Chunks of up to 64 blocks: every word of a chunk is a
// function of its position alone (chunk_word: the carried tail, then the codes, then — when the digest is finished — the padding and the
// bit length), the chain runs over the chunk, and the bytes past the last block are the new tail. update_codes() walks that schedule
// serially and is what the host uses (elemhip_flac_md5_update, the host-encoded fallback); the kernel walks the same schedule with
// the same functions, one wave per stream, a lane per word. Byte counts are 64-bit throughout.
//
// Plain C++ for host and device alike.
#ifndef ELEMHIP_FLAC_MD5_H
#define ELEMHIP_FLAC_MD5_H
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#include "pcm_pack.h"

namespace flac_md5 {

constexpr uint32_t kChunkBlocks = 64;                   // MD5 blocks gathered at a time
constexpr uint32_t kChunkBytes = 64u * kChunkBlocks, kChunkWords = 16u * kChunkBlocks;
constexpr uint32_t kNowhere = 0xFFFFFFFFu;

struct alignas(16) Record {
    uint32_t h[4];          // the chaining value behind the last whole block
    uint64_t bytes;         // message bytes so far
    uint32_t pad[2];
    uint8_t  tail[64];      // the bytes % 64 bytes behind the last whole block
};
static_assert(sizeof(Record) == 96, "a multiple of 16 bytes");

PCM_CX bool bits_ok(uint32_t bits) { return bits == 16u || bits == 24u; }

PCM_FD void init(Record& r) {
    r.h[0] = 0x67452301u; r.h[1] = 0xefcdab89u; r.h[2] = 0x98badcfeu; r.h[3] = 0x10325476u;
    r.bytes = 0; r.pad[0] = r.pad[1] = 0u;
    for (uint32_t i = 0; i < 64u; ++i) r.tail[i] = 0u;
}

// ---- RFC 1321 ------------------------------------------------------------------------------------------------------------------------
PCM_FD uint32_t k_of(uint32_t i) {          // floor(2^32 |sin(i + 1)|)
    constexpr uint32_t k[64] = {
        0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u,
        0x698098d8u, 0x8b44f7afu, 0xffff5bb1u, 0x895cd7beu, 0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u,
        0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau, 0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u,
        0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u, 0x676f02d9u, 0x8d2a4c8au,
        0xfffa3942u, 0x8771f681u, 0x6d9d6122u, 0xfde5380cu, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u,
        0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u, 0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u,
        0xf4292244u, 0x432aff97u, 0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du, 0x85845dd1u,
        0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u, 0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u,
    };
    return k[i & 63u];
}
// the message word round i reads, and its rotation
PCM_CX uint32_t word_of(uint32_t i) { return (i < 16u ? i : i < 32u ? 5u * i + 1u : i < 48u ? 3u * i + 5u : 7u * i) & 15u; }
PCM_CX uint32_t shift_of(uint32_t i) {
    return i < 16u ? ((i & 3u) == 0u ? 7u : (i & 3u) == 1u ? 12u : (i & 3u) == 2u ? 17u : 22u)
         : i < 32u ? ((i & 3u) == 0u ? 5u : (i & 3u) == 1u ? 9u : (i & 3u) == 2u ? 14u : 20u)
         : i < 48u ? ((i & 3u) == 0u ? 4u : (i & 3u) == 1u ? 11u : (i & 3u) == 2u ? 16u : 23u)
                   : ((i & 3u) == 0u ? 6u : (i & 3u) == 1u ? 10u : (i & 3u) == 2u ? 15u : 21u);
}
// round i of a block; x = k_of(i) + M[word_of(i)], which does not depend on the chain
PCM_FD void round(uint32_t i, uint32_t x, uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
    const uint32_t f = i < 16u ? ((b & c) | (~b & d)) : i < 32u ? ((d & b) | (~d & c)) : i < 48u ? (b ^ c ^ d) : (c ^ (b | ~d));
    const uint32_t t = a + f + x, s = shift_of(i);
    a = d; d = c; c = b;
    b = b + ((t << s) | (t >> (32u - s)));
}
PCM_FD void block(uint32_t h[4], const uint32_t* m) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
    for (uint32_t i = 0; i < 64u; ++i) round(i, k_of(i) + m[word_of(i)], a, b, c, d);
    h[0] += a; h[1] += b; h[2] += c; h[3] += d;
}

// ---- the schedule of one update -----------------------------------------------------------------------------------------------------------
// `count` frames of G channels enter behind the record's tail; with `finish` the padding and the bit length follow them
struct Job {
    uint64_t total;         // the carried tail and the new bytes
    uint64_t blocks;        // whole blocks to chain (finish: the padded message's)
    uint64_t bitLen;        // the message's bits with this update
    uint32_t fill, G, B, FB /* bytes of a frame */, first, finish;
};
PCM_FD Job make_job(uint64_t bytesSoFar, uint32_t G, uint32_t first, uint64_t count, uint32_t bits, bool finish) {
    Job j;
    j.G = G; j.B = (bits + 7u) / 8u; j.FB = G * j.B; j.first = first; j.finish = finish ? 1u : 0u;
    j.fill = (uint32_t)(bytesSoFar & 63u);
    j.total = j.fill + count * j.FB;
    j.bitLen = (bytesSoFar + count * j.FB) * 8u;
    j.blocks = finish ? (j.total + 9u + 63u) / 64u : j.total / 64u;
    return j;
}
PCM_FD uint32_t leftover(const Job& j) { return j.finish ? 0u : (uint32_t)(j.total - j.blocks * 64u); }

// A chunk: blocks [block0, block0 + blocks) of the job. Positions inside it are 32-bit offsets v from its first byte; the chunk's last
// one also answers for the leftover bytes behind its blocks (v < kChunkBytes + 64).
struct Chunk {
    uint64_t block0;
    uint32_t blocks;
    uint32_t fillc;         // v < fillc: the carried tail (the first chunk only)
    uint32_t end;           // v < end: code bytes (clamped: far beyond the chunk is all the same)
    uint32_t frame, rem;    // the code byte at v = fillc is byte `rem` of frame `frame`
    uint32_t mark, lenAt;   // where the 0x80 and the bit length stand (kNowhere: not in this chunk)
};
PCM_FD void settle(const Job& j, Chunk& c) {
    const uint64_t left = j.blocks - c.block0, base = c.block0 * 64u, far = 2u * kChunkBytes;
    c.blocks = left < kChunkBlocks ? (uint32_t)left : kChunkBlocks;
    const uint64_t toEnd = j.total > base ? j.total - base : 0u;
    c.end = (uint32_t)(toEnd < far ? toEnd : far);
    c.mark = j.finish && j.total >= base && j.total - base < far ? (uint32_t)(j.total - base) : kNowhere;
    const uint64_t lenAt = j.blocks * 64u - 8u - base;          // (finish: blocks >= 1 and base < blocks * 64)
    c.lenAt = j.finish && lenAt < far ? (uint32_t)lenAt : kNowhere;
}
PCM_FD Chunk first_chunk(const Job& j) {
    Chunk c;
    c.block0 = 0; c.fillc = j.fill; c.frame = j.first; c.rem = 0u;
    settle(j, c);
    return c;
}
PCM_FD bool last_chunk(const Job& j, const Chunk& c) { return c.block0 + c.blocks == j.blocks; }
PCM_FD void next_chunk(const Job& j, Chunk& c) {
    c.rem += kChunkBytes - c.fillc;
    c.frame += c.rem / j.FB; c.rem %= j.FB;
    c.fillc = 0u; c.block0 += kChunkBlocks;
    settle(j, c);
}

// byte r of a frame's G * B bytes; codes(g, f): the code of channel g at frame f
template <class Codes> PCM_FD uint32_t frame_byte(const Job& j, const Codes& codes, uint32_t f, uint32_t r) {
    const uint32_t g = j.B == 2u ? r >> 1 : j.B == 1u ? r : r / 3u, k = r - g * j.B;
    return ((uint32_t)codes(g, f) >> (8u * k)) & 0xFFu;
}
template <class Codes> PCM_FD uint32_t chunk_byte(const Job& j, const Chunk& c, const uint8_t* tail, const Codes& codes, uint32_t v) {
    if (v < c.fillc) return tail[v];
    if (v < c.end) {
        const uint32_t t = c.rem + (v - c.fillc), f = t / j.FB;
        return frame_byte(j, codes, c.frame + f, t - f * j.FB);
    }
    if (v == c.mark) return 0x80u;
    if (v >= c.lenAt && v - c.lenAt < 8u) return (uint32_t)(j.bitLen >> (8u * (v - c.lenAt))) & 0xFFu;
    return 0u;
}
// the little-endian message word at v (a multiple of 4): one division where all four bytes are code bytes
template <class Codes> PCM_FD uint32_t chunk_word(const Job& j, const Chunk& c, const uint8_t* tail, const Codes& codes, uint32_t v) {
    uint32_t w = 0u;
    if (v >= c.fillc && v + 3u < c.end) {
        const uint32_t t = c.rem + (v - c.fillc);
        uint32_t f = t / j.FB, r = t - f * j.FB;
        for (uint32_t k = 0; k < 4u; ++k) {
            w |= frame_byte(j, codes, c.frame + f, r) << (8u * k);
            if (++r == j.FB) { r = 0u; ++f; }
        }
        return w;
    }
    for (uint32_t k = 0; k < 4u; ++k) w |= chunk_byte(j, c, tail, codes, v + k) << (8u * k);
    return w;
}
PCM_FD void put_digest(const uint32_t h[4], uint8_t* digest) {
    for (uint32_t i = 0; i < 16u; ++i) digest[i] = (uint8_t)(h[i >> 2] >> (8u * (i & 3u)));
}

// ---- the schedule walked serially (the host's update; the kernel's twin) ----------------------------------------------------------------------
// `count` frames from `first` on of codes(g, f) enter the record's digest; with `digest` the message ends here: padded, chained, written out
template <class Codes> inline void run(Record& r, const Codes& codes, uint32_t G, uint32_t first, uint64_t count, uint32_t bits, uint8_t* digest) {
    const Job j = make_job(r.bytes, G, first, count, bits, digest != nullptr);
    uint32_t m[kChunkWords];
    for (Chunk c = first_chunk(j);; next_chunk(j, c)) {
        for (uint32_t w = 0; w < 16u * c.blocks; ++w) m[w] = chunk_word(j, c, r.tail, codes, 4u * w);
        for (uint32_t b = 0; b < c.blocks; ++b) block(r.h, m + 16u * b);
        if (!last_chunk(j, c)) continue;
        uint8_t left[64];
        const uint32_t n = leftover(j);
        for (uint32_t i = 0; i < n; ++i) left[i] = (uint8_t)chunk_byte(j, c, r.tail, codes, 64u * c.blocks + i);
        memcpy(r.tail, left, n);
        break;
    }
    r.bytes += count * j.FB;
    if (digest) put_digest(r.h, digest);
}
// planar int32 codes of one stream: frames [first, first + count) of planar[0 .. G)
inline void update_codes(Record& r, const int32_t* const* planar, uint32_t G, uint32_t first, uint64_t count, uint32_t bits) {
    run(r, [planar](uint32_t g, uint32_t f) { return planar[g][f]; }, G, first, count, bits, nullptr);
}
// the digest of what has entered so far; the record goes on as it was
inline void final(const Record& r, uint8_t digest[16]) {
    Record t = r;
    run(t, [](uint32_t, uint32_t) { return (int32_t)0; }, 1u, 0u, 0u, 16u, digest);
}

} // namespace flac_md5
#endif
