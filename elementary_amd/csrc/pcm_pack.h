// pcm_pack.h — the arithmetic and the lane schedule of PCM delivery (pcm_pack.hip, Engine::processBlocksPcm).
//
// A launch set's output lies in HBM as [block][channel][blockSize] float32. Delivery turns it into `nStreams` streams of
// `G` interleaved channels each (sample (frame, g) of stream s = output channel s * G + g), as 16-bit or packed 24-bit
// little-endian integers with optional TPDF dither, or as the float bits unchanged, and counts per channel what a
// mastering caller asks first: the peak, the samples over full scale and the non-finite ones.
//
// The dither is keyed on the ABSOLUTE frame time and the channel, so the bytes of a render do not depend on how it is cut
// into calls, relay windows or launch sets.
//
// One workgroup packs one TILE: up to tile_frames(G) frames of one block of one stream.
//   stage A  a wave takes 64 quads (4 frames, one 16-byte load where the quad is whole and the row's address allows) of one
//            channel row, folds the statistics, quantises and stores the codes to that channel's LDS row
//   stage B  thread <-> sample of the tile in STREAM order: the transposed read of the LDS rows (rows start at skewed banks,
//            row_bases: a half-wave's 32 reads hit 32 banks for every G up to 32), the code's bytes go to an LDS image of the
//            tile's stretch of the stream that is aligned like the stream itself (image_head)
//   stage C  thread <-> 16-byte piece of the image: whole pieces leave with one 16-byte store, the pieces a tile shares
//            with its neighbours (a stretch need not start or end on 16 bytes: odd block sizes, 3-byte samples) in sample units
//
// Plain index arithmetic for host and device alike: tests/native/pcm_pack_host.cpp runs the three stages with these functions,
// lane by lane, and checks every byte against a scalar loop. pack_host() below is that scalar loop's production twin: the engine
// uses it where a render's floats are already on the host (taps under a sliced host block) — same functions, same bits.
#ifndef ELEMHIP_PCM_PACK_H
#define ELEMHIP_PCM_PACK_H
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define PCM_FD __host__ __device__ __forceinline__
#define PCM_CX __host__ __device__ constexpr __forceinline__
#else
#define PCM_FD inline
#define PCM_CX constexpr inline
#endif

namespace pcm_pack {

// ---- formats -------------------------------------------------------------------------------------------------------------------
constexpr uint32_t S16 = 1;       // little-endian int16
constexpr uint32_t S24 = 2;       // 3 bytes per sample, little-endian two's complement, packed
constexpr uint32_t F32 = 3;       // the float unchanged

PCM_CX bool format_ok(uint32_t fmt) { return fmt >= S16 && fmt <= F32; }
PCM_CX uint32_t sample_bytes(uint32_t fmt) { return fmt == S16 ? 2u : fmt == S24 ? 3u : 4u; }

// ---- dither ----------------------------------------------------------------------------------------------------------------------
PCM_FD uint32_t hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
PCM_FD uint32_t channel_key(uint32_t seed, uint32_t channel) { return hash32(seed ^ (channel * 0x9E3779B9u)); }
// (the upper half of the time changes once in 2^32 frames: a caller that walks a row keeps hi_key and recomputes it on a change)
PCM_FD uint32_t hi_key(uint32_t k0, uint32_t hi) { return hash32(hi ^ k0); }
PCM_FD float dither_lo(uint32_t hiKey, uint32_t lo) {
    const uint32_t k = hash32(lo ^ hiKey);
    const uint32_t r1 = hash32(k), r2 = hash32(k ^ 0x85EBCA6Bu);
    return (float)((int32_t)(r1 >> 8) - (int32_t)(r2 >> 8)) * 5.9604644775390625e-8f;      // 2^-24: (-1, 1), exact in float32
}
PCM_FD float dither(uint32_t k0, int64_t t) {
    return dither_lo(hi_key(k0, (uint32_t)((uint64_t)t >> 32)), (uint32_t)((uint64_t)t & 0xFFFFFFFFu));
}

// ---- one sample ------------------------------------------------------------------------------------------------------------------
PCM_FD uint32_t float_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
PCM_FD bool finite_bits(uint32_t u) { return (u & 0x7F800000u) != 0x7F800000u; }

// x * 2^(bits-1) + d, rounded to nearest even, clamped to [-2^(bits-1), 2^(bits-1) - 1]; a non-finite x counts as 0
PCM_FD int32_t quantise(float x, uint32_t bits, float d) {
    const float S = bits == 16u ? 32768.0f : 8388608.0f;
    if (!finite_bits(float_bits(x))) x = 0.0f;
    const float v = x * S + d;               // (the product is exact: a contracted form gives the same bits)
    float q = __builtin_rintf(v);
    q = q < -S ? -S : (q > S - 1.0f ? S - 1.0f : q);
    return (int32_t)q;
}
// what stage A leaves in LDS for a sample: the integer code (its low 2 or 3 bytes are the sample), or the float's bits
PCM_FD uint32_t encode(uint32_t fmt, float x, float d) {
    return fmt == F32 ? float_bits(x) : (uint32_t)quantise(x, fmt == S16 ? 16u : 24u, d);
}

struct ChannelStats { uint32_t peakBits, over, nonfinite; };      // one per channel on the device: pcm_pack.hip adds into it per wave
// (peakBits: the bit pattern of a non-negative float orders like the float)
PCM_FD ChannelStats stats_fold(float x, ChannelStats s) {
    const uint32_t a = float_bits(x) & 0x7FFFFFFFu;
    const bool fin = a < 0x7F800000u;
    s.peakBits = fin && a > s.peakBits ? a : s.peakBits;
    s.over += fin && a > 0x3F800000u ? 1u : 0u;            // |x| > 1.0f
    s.nonfinite += fin ? 0u : 1u;
    return s;
}

// ---- tiles -----------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kTileSamples = 4096;       // samples of a tile at most (frames x G) while a tile holds 4 frames or more
constexpr uint32_t kMaxBlock = 512;
constexpr uint32_t kMaxGroup = 1024;          // channels per stream (the output bus has no more)

// frames per tile: whole quads, as many as kTileSamples allows, a block at most
PCM_FD uint32_t tile_frames(uint32_t G) {
    uint32_t t = (kTileSamples / (G ? G : 1u)) & ~3u;
    return t < 4u ? 4u : (t > kMaxBlock ? kMaxBlock : t);
}
PCM_FD uint32_t tiles_per_block(uint32_t bs, uint32_t G) { const uint32_t t = tile_frames(G); return (bs + t - 1u) / t; }
// frames of tile `ti` of block `b` that are delivered (0: the tile lies behind the set's valid frames)
PCM_FD uint32_t tile_valid(uint32_t bs, uint32_t G, uint32_t b, uint32_t ti, uint32_t validFrames) {
    const uint32_t f0 = ti * tile_frames(G);
    if (f0 >= bs) return 0u;
    const uint64_t abs0 = (uint64_t)b * bs + f0;
    if (abs0 >= validFrames) return 0u;
    uint32_t n = bs - f0 < tile_frames(G) ? bs - f0 : tile_frames(G);
    if ((uint64_t)n > validFrames - abs0) n = (uint32_t)(validFrames - abs0);
    return n;
}

// ---- stage A: quads of a channel row ---------------------------------------------------------------------------------------------
// `m` = (address of the row's first frame / 4) mod 4: quad q holds the frames 4q - m .. 4q - m + 3 of the tile, so that a whole
// quad is one aligned 16-byte load whatever the block size (350: every other row starts 8 bytes off; 341: rows start anywhere)
PCM_FD uint32_t row_quads(uint32_t n, uint32_t m) { return (n + m + 3u) / 4u; }
PCM_FD int32_t quad_first(uint32_t q, uint32_t m) { return (int32_t)(4u * q) - (int32_t)m; }
PCM_FD bool quad_whole(int32_t first, uint32_t n) { return first >= 0 && (uint32_t)first + 4u <= n; }
// chunks of 64 quads a row is cut into — the same for every row of a tile (rows of a block size that is a multiple of 4 all start
// on 16 bytes, tiles do; otherwise m = 3 at worst), so that work items are (row, chunk)
PCM_FD uint32_t row_chunks(uint32_t n, uint32_t bs) { return (row_quads(n, (bs & 3u) ? 3u : 0u) + 63u) / 64u; }

// ---- stage B / C: the LDS image of the tile's stretch of its stream ----------------------------------------------------------------
// the stretch starts at byte `c0` of the stream; the image starts at the 16-byte line below it
PCM_FD uint64_t stretch_begin(uint32_t bs, uint32_t G, uint32_t fmt, uint32_t b, uint32_t f0) {
    return ((uint64_t)b * bs + f0) * G * sample_bytes(fmt);
}
PCM_FD uint32_t image_head(uint64_t c0) { return (uint32_t)(c0 & 15u); }
PCM_FD uint32_t image_offset(uint32_t head, uint32_t j, uint32_t fmt) { return head + j * sample_bytes(fmt); }
PCM_FD uint32_t piece_count(uint32_t head, uint32_t len) { return (head + len + 15u) / 16u; }
PCM_FD bool piece_whole(uint32_t p, uint32_t head, uint32_t len) { return 16u * p >= head && 16u * p + 16u <= head + len; }
// narrow stores of a shared piece: the unit (a sample; a byte for 3-byte samples)
PCM_CX uint32_t store_unit(uint32_t fmt) { return fmt == S16 ? 2u : fmt == S24 ? 1u : 4u; }
PCM_FD uint32_t image_bytes(uint32_t G) { return tile_frames(G) * G * 4u + 32u; }

// ---- LDS rows: where each channel's row of codes starts (dwords) -----------------------------------------------------------------
// Stage B's half-wave reads 32 consecutive samples j of the stream order, sample j from row j % G at frame j / G. With row g starting
// at bank skew[g] the read hits bank skew[j % G] + j / G. The skews below make that a bijection onto the 32 banks for every window
// of 32 samples that starts at a multiple of 32: walk the rows in steps of -32 (mod G; blocks of D = gcd(32, G) neighbouring rows
// behave alike, a walk visits one row of each block and the next walk the next row), giving each row the bank interval behind its
// predecessor's: floor(32 / G) banks, one more for the rows of the first (32 mod G) / D blocks. Over the G rows that is 32 banks.
// For G <= 32 rows are laid out one after another, each moved up to its bank (at most 31 dwords lost per row); above 32 a tile's rows
// are too short to pay for that: an odd stride, two-way conflicts at worst.
inline uint32_t gcd32(uint32_t g) { uint32_t d = 1; while (d < 32u && g % (2u * d) == 0u) d *= 2u; return d; }
// out[g] = first dword of row g; returns the dwords all rows take
inline uint32_t row_bases(uint32_t G, uint16_t* out) {
    const uint32_t tf = tile_frames(G);
    if (G > 32u) { for (uint32_t g = 0; g < G; ++g) out[g] = (uint16_t)(g * (tf + 1u)); return G * (tf + 1u); }
    uint8_t skew[32];
    const uint32_t D = gcd32(G), Gp = G / D, q = 32u / G, rp = (32u % G) / D;
    uint32_t P = 0, i = 0, o = 0;
    for (uint32_t step = 0; step < G; ++step) {
        skew[P * D + i] = (uint8_t)(o & 31u);
        o += q + (P < rp ? 1u : 0u);
        P = (P + Gp - rp % Gp) % Gp;
        if (P == 0u) ++i;
    }
    uint32_t end = 0;
    for (uint32_t g = 0; g < G; ++g) {
        const uint32_t base = end + ((skew[g] + 32u - (end & 31u)) & 31u);
        out[g] = (uint16_t)base;
        end = base + tf;
    }
    return end;
}
// dynamic LDS of a launch: the rows, the image (16-byte aligned), the row table
PCM_FD uint32_t lds_image_offset(uint32_t rowDwords) { return (rowDwords * 4u + 15u) & ~15u; }
PCM_FD uint32_t lds_table_offset(uint32_t rowDwords, uint32_t G) { return lds_image_offset(rowDwords) + ((image_bytes(G) + 15u) & ~15u); }
PCM_FD uint32_t lds_bytes(uint32_t rowDwords, uint32_t G) { return lds_table_offset(rowDwords, G) + G * 4u; }

// ---- streams ---------------------------------------------------------------------------------------------------------------------
// bytes between two streams of a packed set in the staging buffers: the set's frames, up to the next 16-byte line
PCM_FD uint64_t stream_stride(uint64_t frames, uint32_t G, uint32_t fmt) { return (frames * G * sample_bytes(fmt) + 15u) & ~(uint64_t)15u; }

// ---- the scalar loop ---------------------------------------------------------------------------------------------------------------
// planar[c] + frame -> streams[s] at frame * G + g, frames [0, n) at absolute time t0; stats (peakBits / over / nonfinite per channel)
// are ADDED to. `planar` rows are `stride` floats apart. `shaped` (null: none): the s16 / s24 codes of the same frames, laid out like
// `planar` (noise_shape.h), taken in place of quantising; the statistics are still the floats'.
inline void pack_host(uint32_t fmt, uint32_t G, uint32_t nStreams, bool dith, uint32_t seed, const float* planar, size_t stride,
                      size_t n, int64_t t0, uint8_t* const* streams, uint32_t* peakBits, uint64_t* over, uint64_t* nonfinite,
                      const int32_t* shaped = nullptr) {
    const uint32_t B = sample_bytes(fmt);
    for (uint32_t s = 0; s < nStreams; ++s)
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t c = s * G + g, k0 = channel_key(seed, c);
            const float* row = planar + (size_t)c * stride;
            ChannelStats st{peakBits ? peakBits[c] : 0u, 0u, 0u};
            for (size_t f = 0; f < n; ++f) {
                const float x = row[f];
                st = stats_fold(x, st);
                const uint32_t code = shaped && fmt != F32 ? (uint32_t)shaped[(size_t)c * stride + f]
                                                           : encode(fmt, x, dith && fmt != F32 ? dither(k0, t0 + (int64_t)f) : 0.0f);
                uint8_t* d = streams[s] + (f * G + g) * B;
                for (uint32_t k = 0; k < B; ++k) d[k] = (uint8_t)(code >> (8u * k));
            }
            if (peakBits) peakBits[c] = st.peakBits;
            if (over) over[c] += st.over;
            if (nonfinite) nonfinite[c] += st.nonfinite;
        }
}

} // namespace pcm_pack

#endif // ELEMHIP_PCM_PACK_H
