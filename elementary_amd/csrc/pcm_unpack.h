// pcm_unpack.h — the arithmetic and the lane schedule of PCM input (pcm_unpack.hip, Engine::processBlocksPcmIo): pcm_pack.h backwards.
//
// An offline render's input arrives as `nStreams` streams of `G` interleaved channels each (sample (frame, g) of stream s = input
// channel s * G + g), 16-bit or packed 24-bit little-endian integers or float32, and has to lie in HBM as the render kernels read it:
// [block][channel][blockSize] float32. The tile geometry, the LDS rows with their skewed start banks and the LDS image of a tile's
// stretch of its stream are pcm_pack.h's — one layout for both directions.
//
// One workgroup unpacks one TILE: up to tile_frames(G) frames of one block of one stream.
//   stage A  thread <-> 16-byte piece of the tile's stretch of the stream: one aligned 16-byte load into the LDS image (the staging
//            buffer is padded to whole 16-byte lines per stream, stream_stride, so EVERY piece is loaded whole; the bytes a piece
//            shares with a neighbouring tile are loaded and never decoded)
//   stage B  thread <-> sample of the tile in STREAM order: its 2 / 3 / 4 bytes from the image, decode, the float's bits to LDS row
//            j % G at frame j / G. Rows start at row_bases' skewed banks: a half-wave's 32 writes hit 32 banks for every G up to 32,
//            as the pack kernel's transposed reads do
//   stage C  a wave per (row, chunk of 64 quads): quad q of a row holds the frames 4q - m .. 4q - m + 3 (`m` from the destination's
//            address, as in pack's stage A), one 16-byte store where the quad is whole, dword stores at a row's two ends. The frames
//            behind the valid ones — a cut last block, the engine blocks that only fill up the last host block — are written as
//            zero: a tile covers every frame of its block whatever `validFrames` is.
//            The four dwords of a quad are read from the (skewed, so not 16-byte aligned) LDS row with four 32-bit reads. Lane l
//            reads them in the order quad_slot(e, l): the lanes l, l + 8, l + 16, l + 24 of a half-wave, whose quads start on one
//            bank, then read four different banks, and every read instruction is conflict-free.
//
// decode is exact: an int16 or a 24-bit integer times a power of two is a float32. Nothing rounds, nothing to tolerate; and
// pcm_pack::quantise(decode(v)) == v without dither.
//
// unpack_host() is the scalar loop: the yardstick of tests/native/pcm_unpack_host.cpp, which runs the three stages lane by lane, and
// the production twin where a render's inputs are needed on the host (taps under a sliced host block).
#ifndef ELEMHIP_PCM_UNPACK_H
#define ELEMHIP_PCM_UNPACK_H
#include "pcm_pack.h"

namespace pcm_unpack {

using pcm_pack::S16;
using pcm_pack::S24;
using pcm_pack::F32;
using pcm_pack::kThreads;
using pcm_pack::kWaves;
using pcm_pack::format_ok;
using pcm_pack::sample_bytes;

// ---- one sample ------------------------------------------------------------------------------------------------------------------
// `raw`: the sample's bytes, little-endian, in the low bits (what lies above them is ignored). Returns the bits of the float:
// an f32 sample passes through as bits — NaN payloads, infinities and denormals included.
PCM_FD uint32_t decode_bits(uint32_t fmt, uint32_t raw) {
    if (fmt == F32) return raw;
    const float x = fmt == S16 ? (float)(int16_t)(uint16_t)(raw & 0xFFFFu) * 3.0517578125e-05f                     // 2^-15
                               : (float)((int32_t)(raw << 8) >> 8) * 1.1920928955078125e-07f;                       // 2^-23
    return pcm_pack::float_bits(x);
}
PCM_FD float decode(uint32_t fmt, uint32_t raw) { const uint32_t u = decode_bits(fmt, raw); float x; memcpy(&x, &u, 4); return x; }
// the sample at `p` (any alignment)
PCM_FD uint32_t load_raw(uint32_t fmt, const unsigned char* p) {
    uint32_t raw = (uint32_t)p[0] | ((uint32_t)p[1] << 8);
    if (fmt != S16) raw |= (uint32_t)p[2] << 16;
    if (fmt == F32) raw |= (uint32_t)p[3] << 24;
    return raw;
}

// ---- tiles -----------------------------------------------------------------------------------------------------------------------
// frames of tile `ti` that lie in the block at all: stage C writes them all, the first tile_valid() of them from the stream
PCM_FD uint32_t tile_span(uint32_t bs, uint32_t G, uint32_t ti) {
    const uint32_t tf = pcm_pack::tile_frames(G), f0 = ti * tf;
    return f0 >= bs ? 0u : (bs - f0 < tf ? bs - f0 : tf);
}

// ---- stage C: the order in which a lane reads its quad's four dwords ---------------------------------------------------------------
// read e of lane l fetches element quad_slot(e, l) of the quad; element x therefore sits in read (x - (l >> 3)) & 3
PCM_FD uint32_t quad_slot(uint32_t e, uint32_t lane) { return (e + (lane >> 3)) & 3u; }
PCM_FD uint32_t quad_read_of(uint32_t x, uint32_t lane) { return (x - (lane >> 3)) & 3u; }

// ---- the scalar loop ---------------------------------------------------------------------------------------------------------------
// streams[s] at frame * G + g -> planar[c] + frame (rows `stride` floats apart, c = s * G + g), frames [0, n); frames [n, padTo)
// of every row are zero
inline void unpack_host(uint32_t fmt, uint32_t G, uint32_t nStreams, const unsigned char* const* streams, size_t n, float* planar,
                        size_t stride, size_t padTo) {
    const uint32_t B = sample_bytes(fmt);
    for (uint32_t s = 0; s < nStreams; ++s)
        for (uint32_t g = 0; g < G; ++g) {
            float* row = planar + ((size_t)s * G + g) * stride;
            for (size_t f = 0; f < n; ++f) {
                const uint32_t u = decode_bits(fmt, load_raw(fmt, streams[s] + (f * G + g) * B));
                memcpy(row + f, &u, 4);
            }
            for (size_t f = n; f < padTo; ++f) row[f] = 0.0f;
        }
}

} // namespace pcm_unpack

#endif // ELEMHIP_PCM_UNPACK_H
