// pcm_unpack.hip — the first stage of an offline render fed with PCM (Engine::processBlocksPcmIo): a launch set's input, `nStreams`
// interleaved streams of 16-bit, packed 24-bit or float samples in HBM, becomes float32 [block][channel][blockSize], the layout the
// render kernels read. One workgroup per tile (pcm_unpack.h / pcm_pack.h: the arithmetic, the tile and lane schedule and the LDS
// layout all come from those headers, which tests/native/pcm_unpack_host.cpp runs on the CPU):
//   A  one aligned 16-byte load per 16-byte piece of the tile's stretch of the stream, into an LDS image aligned like the stream
//   B  thread <-> sample in stream order: decode, conflict-free transposed write to the skewed LDS rows
//   C  a wave per (row, 64 quads): four conflict-free 32-bit LDS reads per lane, one 16-byte store per whole quad, zeros behind the
//      valid frames
#include <hip/hip_runtime.h>

#include "pcm_unpack.h"
#include "launch.h"

namespace elemhip {

namespace {

namespace pp = pcm_pack;
namespace pu = pcm_unpack;

template <uint32_t FMT>
__global__ __launch_bounds__(pp::kThreads) void elemhip_pcm_unpack(PcmUnpackArgs a) {
    extern __shared__ __align__(16) unsigned char pcmInLds[];
    uint32_t* rows = reinterpret_cast<uint32_t*>(pcmInLds);
    unsigned char* image = pcmInLds + pp::lds_image_offset(a.rowDwords);
    uint32_t* table = reinterpret_cast<uint32_t*>(pcmInLds + pp::lds_table_offset(a.rowDwords, a.G));

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t b = blockIdx.x / a.tilesPerBlock, ti = blockIdx.x % a.tilesPerBlock, s = blockIdx.y;
    const uint32_t G = a.G, bs = a.blockSize;
    const uint32_t n = pp::tile_valid(bs, G, b, ti, a.validFrames);      // frames that come from the stream (uniform) ...
    const uint32_t span = pu::tile_span(bs, G, ti);                      // ... of the frames this tile writes
    const uint32_t f0 = ti * pp::tile_frames(G);

#pragma clang loop vectorize(disable) unroll(disable)
    for (uint32_t g = tid; g < G; g += pp::kThreads) table[g] = a.rowBase[g];

    if (n != 0u) {
        // ---- A: thread <-> 16-byte piece. The stream's staging stride is a multiple of 16 and the stretch ends inside it, so every
        // piece is loaded whole — the narrow edge accesses of the pack kernel's stage C have no counterpart here: a byte that belongs
        // to the neighbouring tile is loaded and not decoded ----
        const uint64_t c0 = pp::stretch_begin(bs, G, FMT, b, f0);
        const uint32_t head = pp::image_head(c0), total = n * G;
        const uint32_t len = total * pp::sample_bytes(FMT), pieces = pp::piece_count(head, len);
        const unsigned char* in = a.src + (size_t)s * a.streamStride + (size_t)(c0 - head);
        for (uint32_t p = tid; p < pieces; p += pp::kThreads)
            *reinterpret_cast<uint4*>(image + 16u * p) = *reinterpret_cast<const uint4*>(in + 16u * p);
        __syncthreads();

        // ---- B: thread <-> sample in stream order ----
        uint32_t g = tid % G, f = tid / G;
        const uint32_t dg = pp::kThreads % G, df = pp::kThreads / G;
        for (uint32_t j = tid; j < total; j += pp::kThreads) {
            const unsigned char* p = image + pp::image_offset(head, j, FMT);
            uint32_t raw;
            if (FMT == pp::S16) raw = *reinterpret_cast<const uint16_t*>(p);
            else if (FMT == pp::S24) raw = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
            else raw = *reinterpret_cast<const uint32_t*>(p);
            rows[table[g] + f] = pu::decode_bits(FMT, raw);
            g += dg; f += df;
            if (g >= G) { g -= G; ++f; }
        }
    }
    __syncthreads();

    // ---- C: (row, chunk of 64 quads) items over the waves ----
    const uint32_t chunks = pp::row_chunks(span, bs), items = G * chunks;
    for (uint32_t item = wave; item < items; item += pp::kWaves) {
        const uint32_t g = item / chunks, q = (item % chunks) * 64u + lane;
        float* row = a.dst + ((size_t)b * a.numChannels + (size_t)s * G + g) * bs + f0;
        const uint32_t m = (uint32_t)(reinterpret_cast<uintptr_t>(row) >> 2) & 3u;
        const int32_t first = pp::quad_first(q, m);
        const uint32_t* src = rows + table[g];
        uint32_t t[4];
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) {
            const int32_t f = first + (int32_t)pu::quad_slot(e, lane);
            t[e] = (f >= 0 && (uint32_t)f < n) ? src[f] : 0u;              // (behind the valid frames: zero)
        }
        // element x of the quad sits in t[quad_read_of(x, lane)]: rotate the four registers back by (lane >> 3) & 3
        const uint32_t r = (lane >> 3) & 3u;
        const uint32_t u0 = (r & 1u) ? t[3] : t[0], u1 = (r & 1u) ? t[0] : t[1], u2 = (r & 1u) ? t[1] : t[2], u3 = (r & 1u) ? t[2] : t[3];
        const uint4 v = make_uint4((r & 2u) ? u2 : u0, (r & 2u) ? u3 : u1, (r & 2u) ? u0 : u2, (r & 2u) ? u1 : u3);
        if (pp::quad_whole(first, span)) { *reinterpret_cast<uint4*>(row + first) = v; continue; }
        auto in = [&](int32_t f) { return f >= 0 && (uint32_t)f < span; };
        uint32_t* out = reinterpret_cast<uint32_t*>(row);
        if (in(first)) out[first] = v.x;
        if (in(first + 1)) out[first + 1] = v.y;
        if (in(first + 2)) out[first + 2] = v.z;
        if (in(first + 3)) out[first + 3] = v.w;
    }
}

} // namespace

hipError_t launch_pcm_unpack(hipStream_t s, const PcmUnpackArgs& a, uint32_t format) {
    if (!pp::format_ok(format) || a.G == 0u || a.G > pp::kMaxGroup || a.blockSize == 0u || a.blockSize > pp::kMaxBlock) return hipErrorInvalidValue;
    if (a.numStreams == 0u || a.numBlocks == 0u) return hipSuccess;
    // every block of the set is written (zeros behind validFrames), every row lies inside [numBlocks][numChannels][blockSize]
    if ((uint64_t)a.numStreams * a.G > a.numChannels || (uint64_t)a.validFrames > (uint64_t)a.numBlocks * a.blockSize) return hipErrorInvalidValue;
    if (a.streamStride % 16u != 0u || a.streamStride < (uint64_t)a.validFrames * a.G * pp::sample_bytes(format)) return hipErrorInvalidValue;
    const uint32_t lds = pp::lds_bytes(a.rowDwords, a.G);
    if (lds > 65536u || a.tilesPerBlock != pp::tiles_per_block(a.blockSize, a.G)) return hipErrorInvalidValue;
    const dim3 grid(a.numBlocks * a.tilesPerBlock, a.numStreams);
    switch (format) {
        case pp::S16: hipLaunchKernelGGL(elemhip_pcm_unpack<pp::S16>, grid, dim3(pp::kThreads), lds, s, a); break;
        case pp::S24: hipLaunchKernelGGL(elemhip_pcm_unpack<pp::S24>, grid, dim3(pp::kThreads), lds, s, a); break;
        default:      hipLaunchKernelGGL(elemhip_pcm_unpack<pp::F32>, grid, dim3(pp::kThreads), lds, s, a); break;
    }
    return hipGetLastError();
}

} // namespace elemhip
