// pcm_pack.hip — the last stage of an offline render delivered as PCM (Engine::processBlocksPcm): a launch set's output, float32
// [block][channel][blockSize] in HBM, becomes `nStreams` interleaved streams of 16-bit, packed 24-bit or float samples, and the
// per-channel statistics of the delivered frames. One workgroup per tile (pcm_pack.h: the arithmetic, the tile and lane schedule and
// the LDS layout all come from that header, which tests/native/pcm_pack_host.cpp runs on the CPU):
//   A  16-byte loads along the channel rows, statistics folded per wave (one atomic per wave and channel), codes to skewed LDS rows
//   B  conflict-free transposed read, the sample's bytes into an LDS image aligned like the stream
//   C  one 16-byte store per whole 16-byte piece of the image; only the pieces shared with a neighbouring tile go out in sample units
#include <hip/hip_runtime.h>

#include "pcm_pack.h"
#include "launch.h"

namespace elemhip {

namespace {

namespace pp = pcm_pack;

template <uint32_t FMT>
__global__ __launch_bounds__(pp::kThreads) void elemhip_pcm_pack(PcmPackArgs a) {
    extern __shared__ __align__(16) unsigned char pcmLds[];
    uint32_t* rows = reinterpret_cast<uint32_t*>(pcmLds);
    unsigned char* image = pcmLds + pp::lds_image_offset(a.rowDwords);
    uint32_t* table = reinterpret_cast<uint32_t*>(pcmLds + pp::lds_table_offset(a.rowDwords, a.G));

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t b = blockIdx.x / a.tilesPerBlock, ti = blockIdx.x % a.tilesPerBlock, s = blockIdx.y;
    const uint32_t G = a.G, bs = a.blockSize;
    const uint32_t n = pp::tile_valid(bs, G, b, ti, a.validFrames);
    if (n == 0u) return;                                      // (uniform: the tile lies behind the last delivered frame)
    const uint32_t f0 = ti * pp::tile_frames(G);

#pragma clang loop vectorize(disable) unroll(disable)
    for (uint32_t g = tid; g < G; g += pp::kThreads) table[g] = a.rowBase[g];

    // ---- A: (row, chunk of 64 quads) items over the waves ----
    const uint32_t chunks = pp::row_chunks(n, bs), items = G * chunks;
    const int64_t tTile = a.time0 + (int64_t)((uint64_t)b * bs + f0);
    for (uint32_t item = wave; item < items; item += pp::kWaves) {
        const uint32_t g = item / chunks, q = (item % chunks) * 64u + lane;
        const uint32_t c = s * G + g;
        const float* row = a.src + ((size_t)b * a.numChannels + c) * bs + f0;
        const uint32_t m = (uint32_t)(reinterpret_cast<uintptr_t>(row) >> 2) & 3u;
        const int32_t first = pp::quad_first(q, m);
        uint32_t* dst = rows + a.rowBase[g];
        const int32_t* shaped = FMT != pp::F32 && a.shaped ? a.shaped + ((size_t)b * a.numChannels + c) * bs + f0 : nullptr;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        auto in = [&](int32_t f) { return f >= 0 && (uint32_t)f < n; };
        if (pp::quad_whole(first, n)) v = *reinterpret_cast<const float4*>(row + first);
        else {
            if (in(first)) v.x = row[first];
            if (in(first + 1)) v.y = row[first + 1];
            if (in(first + 2)) v.z = row[first + 2];
            if (in(first + 3)) v.w = row[first + 3];
        }
        pp::ChannelStats acc{0u, 0u, 0u};
        const uint32_t k0 = pp::channel_key(a.seed, c);
        const uint32_t hi0 = (uint32_t)((uint64_t)tTile >> 32), hk0 = pp::hi_key(k0, hi0);
        auto sample = [&](int32_t f, float x) {
            if (!in(f)) return;
            acc = pp::stats_fold(x, acc);
            if (shaped) { dst[f] = (uint32_t)shaped[f]; return; }       // (noise_shape.hip has quantised the set)
            float d = 0.0f;
            if (FMT != pp::F32 && a.dither) {
                const uint64_t t = (uint64_t)(tTile + f);
                const uint32_t hi = (uint32_t)(t >> 32);
                d = pp::dither_lo(hi == hi0 ? hk0 : pp::hi_key(k0, hi), (uint32_t)(t & 0xFFFFFFFFu));
            }
            dst[f] = pp::encode(FMT, x, d);
        };
        sample(first, v.x); sample(first + 1, v.y); sample(first + 2, v.z); sample(first + 3, v.w);
        uint32_t peak = acc.peakBits, over = acc.over, nonf = acc.nonfinite;
#pragma unroll
        for (uint32_t o = 32u; o > 0u; o >>= 1) {
            peak = max(peak, (uint32_t)__shfl_xor((int)peak, (int)o));
            over += (uint32_t)__shfl_xor((int)over, (int)o);
            nonf += (uint32_t)__shfl_xor((int)nonf, (int)o);
        }
        if (lane == 0u) {
            pp::ChannelStats* st = a.stats + c;
            if (peak) atomicMax(&st->peakBits, peak);
            if (over) atomicAdd(&st->over, over);
            if (nonf) atomicAdd(&st->nonfinite, nonf);
        }
    }
    __syncthreads();

    // ---- B: thread <-> sample in stream order ----
    const uint64_t c0 = pp::stretch_begin(bs, G, FMT, b, f0);
    const uint32_t head = pp::image_head(c0), total = n * G;
    {
        uint32_t g = tid % G, f = tid / G;
        const uint32_t dg = pp::kThreads % G, df = pp::kThreads / G;
        for (uint32_t j = tid; j < total; j += pp::kThreads) {
            const uint32_t code = rows[table[g] + f];
            unsigned char* p = image + pp::image_offset(head, j, FMT);
            if (FMT == pp::S16) *reinterpret_cast<uint16_t*>(p) = (uint16_t)code;
            else if (FMT == pp::S24) { p[0] = (unsigned char)code; p[1] = (unsigned char)(code >> 8); p[2] = (unsigned char)(code >> 16); }
            else *reinterpret_cast<uint32_t*>(p) = code;
            g += dg; f += df;
            if (g >= G) { g -= G; ++f; }
        }
    }
    __syncthreads();

    // ---- C: thread <-> 16-byte piece ----
    const uint32_t len = total * pp::sample_bytes(FMT), pieces = pp::piece_count(head, len);
    unsigned char* out = a.dst + (size_t)s * a.streamStride + (size_t)(c0 - head);
    for (uint32_t p = tid; p < pieces; p += pp::kThreads) {
        if (pp::piece_whole(p, head, len)) {
            *reinterpret_cast<uint4*>(out + 16u * p) = *reinterpret_cast<const uint4*>(image + 16u * p);
            continue;
        }
        const uint32_t lo = 16u * p > head ? 16u * p : head, hi = 16u * p + 16u < head + len ? 16u * p + 16u : head + len;
        constexpr uint32_t U = pp::store_unit(FMT);
#pragma clang loop vectorize(disable) unroll(disable)
        for (uint32_t o = lo; o < hi; o += U) {
            if (U == 2u) *reinterpret_cast<uint16_t*>(out + o) = *reinterpret_cast<const uint16_t*>(image + o);
            else if (U == 4u) *reinterpret_cast<uint32_t*>(out + o) = *reinterpret_cast<const uint32_t*>(image + o);
            else out[o] = image[o];
        }
    }
}

} // namespace

uint32_t pcm_pack_row_table(uint32_t G, uint16_t* out) { return pp::row_bases(G, out); }

hipError_t launch_pcm_pack(hipStream_t s, const PcmPackArgs& a, uint32_t format) {
    if (!pp::format_ok(format) || a.G == 0u || a.G > pp::kMaxGroup || a.blockSize == 0u || a.blockSize > pp::kMaxBlock) return hipErrorInvalidValue;
    if (a.numStreams == 0u || a.validFrames == 0u) return hipSuccess;
    const uint32_t blocks = (a.validFrames + a.blockSize - 1u) / a.blockSize;
    const dim3 grid(blocks * a.tilesPerBlock, a.numStreams);
    const uint32_t lds = pp::lds_bytes(a.rowDwords, a.G);
    if (lds > 65536u || a.tilesPerBlock != pp::tiles_per_block(a.blockSize, a.G)) return hipErrorInvalidValue;
    switch (format) {
        case pp::S16: hipLaunchKernelGGL(elemhip_pcm_pack<pp::S16>, grid, dim3(pp::kThreads), lds, s, a); break;
        case pp::S24: hipLaunchKernelGGL(elemhip_pcm_pack<pp::S24>, grid, dim3(pp::kThreads), lds, s, a); break;
        default:      hipLaunchKernelGGL(elemhip_pcm_pack<pp::F32>, grid, dim3(pp::kThreads), lds, s, a); break;
    }
    return hipGetLastError();
}

} // namespace elemhip
