// resource_load.hip — shared resources made on the GPU from the file's bytes (Engine::addSharedResourcePcm): a piece of an interleaved
// source of 16-bit, packed 24-bit or float samples, staged in HBM as it lies in the file, becomes planar float rows — one per channel,
// the resource's own device buffers. The arithmetic, the pieces and both tile schedules are resource_load.h's (with pcm_pack.h,
// pcm_unpack.h and resample.h behind it), which tests/native/resource_load_host.cpp runs on the CPU lane by lane.
//   resource_copy     the file's rate is the engine's. Workgroup <-> tile of tile_frames(G) frames x G: pcm_unpack.hip's stages with
//                     another destination.
//                     A  one aligned 16-byte load per 16-byte piece of the tile's stretch, into an LDS image aligned like the file
//                     B  thread <-> sample in stream order: decode, conflict-free transposed write to the skewed LDS rows
//                     C  a wave per (row, 64 quads): four conflict-free 32-bit LDS reads per lane, one 16-byte store per whole quad,
//                        dword stores at a row's two ends
//   resource_convert  another rate. Workgroup <-> tile of 256 resource frames x C channels (C = 4; 1 for one-channel sources and where
//                     four rows and their image would not fit 64 KB of LDS): resample_in.hip's tile without carried frames — what a
//                     tile reads outside the file is silence, what it reads inside is in the staged piece.
//                     A/B  the tile's input stretch, decoded, into C padded LDS rows: a narrow source (G <= C) through an aligned LDS
//                          image, thread <-> sample in stream order; a wide one sample by sample, thread <-> frame
//                     C    lane <-> resource frame: one coefficient load (output order: consecutive lanes, consecutive floats) serves
//                          the C channels' fused multiply-adds (resample::tap_sum)
// LDS conflicts: the copy kernel's are pcm_unpack.hip's (none for G <= 32); the converting kernel's are resample_in.hip's (stage C free
// of them when upsampling and at 160:147, up to 2-way per half-wave when downsampling; the narrow staging 2-way at worst).
// The rows are zeroed before the first piece, so the floats behind the last frame stay zero. Plain vector stores, no atomics.
#include <hip/hip_runtime.h>

#include "resource_load.h"
#include "launch.h"

namespace elemhip {

namespace {

namespace rl = resource_load;
namespace rs = resample;
namespace pp = pcm_pack;
namespace pu = pcm_unpack;

template <uint32_t FMT>
__global__ __launch_bounds__(pp::kThreads) void elemhip_resource_copy(ResourceLoadArgs a) {
    extern __shared__ __align__(16) unsigned char resCopyLds[];
    uint32_t* rows = reinterpret_cast<uint32_t*>(resCopyLds);
    unsigned char* image = resCopyLds + pp::lds_image_offset(a.rowDwords);
    uint32_t* table = reinterpret_cast<uint32_t*>(resCopyLds + pp::lds_table_offset(a.rowDwords, a.G));

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t G = a.G, ti = blockIdx.x;
    const uint32_t n = rl::copy_tile_frames(a.validIn, G, ti), f0 = rl::copy_tile_first(ti, G);      // (uniform; n > 0: the grid ends with the piece)

#pragma clang loop vectorize(disable) unroll(disable)
    for (uint32_t g = tid; g < G; g += pp::kThreads) table[g] = a.rowTable[g];

    // ---- A: thread <-> 16-byte piece; the staged copy is padded to whole lines, a byte of a neighbouring tile is loaded and not decoded ----
    const uint64_t c0 = rl::copy_stretch_begin(a.head, f0, G, FMT);
    const uint32_t head = pp::image_head(c0), total = n * G;
    const uint32_t len = total * pp::sample_bytes(FMT), pieces = pp::piece_count(head, len);
    const unsigned char* in = a.src + (size_t)(c0 - head);
    for (uint32_t p = tid; p < pieces; p += pp::kThreads)
        *reinterpret_cast<uint4*>(image + 16u * p) = *reinterpret_cast<const uint4*>(in + 16u * p);
    __syncthreads();

    // ---- B: thread <-> sample in stream order ----
    {
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
    const uint32_t chunks = rl::copy_row_chunks(n), items = G * chunks;
    for (uint32_t item = wave; item < items; item += pp::kWaves) {
        const uint32_t g = item / chunks, q = (item % chunks) * 64u + lane;
        float* row = a.rows[g] + a.out0 + f0;
        const uint32_t m = (uint32_t)(reinterpret_cast<uintptr_t>(row) >> 2) & 3u;
        const int32_t first = pp::quad_first(q, m);
        const uint32_t* src = rows + table[g];
        uint32_t t[4];
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) {
            const int32_t f = first + (int32_t)pu::quad_slot(e, lane);
            t[e] = (f >= 0 && (uint32_t)f < n) ? src[f] : 0u;
        }
        // element x of the quad sits in t[quad_read_of(x, lane)]: rotate the four registers back by (lane >> 3) & 3
        const uint32_t r = (lane >> 3) & 3u;
        const uint32_t u0 = (r & 1u) ? t[3] : t[0], u1 = (r & 1u) ? t[0] : t[1], u2 = (r & 1u) ? t[1] : t[2], u3 = (r & 1u) ? t[2] : t[3];
        const uint4 v = make_uint4((r & 2u) ? u2 : u0, (r & 2u) ? u3 : u1, (r & 2u) ? u0 : u2, (r & 2u) ? u1 : u3);
        if (pp::quad_whole(first, n)) { *reinterpret_cast<uint4*>(row + first) = v; continue; }
        auto inside = [&](int32_t f) { return f >= 0 && (uint32_t)f < n; };
        uint32_t* out = reinterpret_cast<uint32_t*>(row);
        if (inside(first)) out[first] = v.x;
        if (inside(first + 1)) out[first + 1] = v.y;
        if (inside(first + 2)) out[first + 2] = v.z;
        if (inside(first + 3)) out[first + 3] = v.w;
    }
}

// sample (frame, g) of the staged piece, decoded; `stream` = the piece's first sample (aligned like a sample: the file's offset of a
// frame is a multiple of the sample size, and the staged copy starts on a 16-byte line of the file)
template <uint32_t FMT>
__device__ __forceinline__ float staged_at(const unsigned char* stream, uint32_t G, uint64_t frame, uint32_t g) {
    const unsigned char* p = stream + (size_t)(frame * G + g) * pp::sample_bytes(FMT);
    uint32_t raw;
    if (FMT == pp::S16) raw = *reinterpret_cast<const uint16_t*>(p);
    else if (FMT == pp::S24) raw = pu::load_raw(FMT, p);
    else raw = *reinterpret_cast<const uint32_t*>(p);
    return __uint_as_float(pu::decode_bits(FMT, raw));
}

template <uint32_t FMT, int C>
__global__ __launch_bounds__(rs::kTile) void elemhip_resource_convert(ResourceLoadArgs a) {
    extern __shared__ __align__(16) unsigned char resConvLds[];
    float* rows = reinterpret_cast<float*>(resConvLds);
    const rs::Plan& p = a.plan;
    const uint32_t G = a.G, lane = threadIdx.x, fFirst = blockIdx.x * rs::kTile, g0 = blockIdx.y * (uint32_t)C;
    const uint32_t f = fFirst + lane, rowFloats = rs::row_floats(p);
    const uint64_t n0 = rl::programme_output(p, a.out0);
    // (fFirst < validOut: the grid ends with the piece's outputs)
    const rs::Tile t = rs::tile_of(p, a.rowBase, n0, fFirst, a.validOut);
    const int64_t rel0 = t.jlo - (int64_t)a.in0;
    const rs::StreamPart part = rs::stream_part(rel0, t.span, a.validIn);
    // the slots the piece does not fill lie outside the file: silence; so does a row behind the source's last channel
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        const bool live = g0 + ch < G;
        for (uint32_t i = lane; i < t.span; i += rs::kTile)
            if (!live || i < part.lo || i >= part.hi) rows[ch * rowFloats + rs::skew(i)] = 0.0f;
    }
    if (part.hi > part.lo) {                        // (uniform)
        const uint64_t frame0 = (uint64_t)(rel0 + (int64_t)part.lo);
        if (G <= (uint32_t)C) {
            // ---- A: thread <-> 16-byte piece ----
            unsigned char* image = resConvLds + rs::in_image_offset(p, (uint32_t)C);
            const uint64_t c0 = (uint64_t)a.head + frame0 * G * pp::sample_bytes(FMT);
            const uint32_t head = pp::image_head(c0), total = (part.hi - part.lo) * G;
            const uint32_t pieces = pp::piece_count(head, total * pp::sample_bytes(FMT));
            const unsigned char* in = a.src + (size_t)(c0 - head);
            for (uint32_t q = lane; q < pieces; q += rs::kTile)
                *reinterpret_cast<uint4*>(image + 16u * q) = *reinterpret_cast<const uint4*>(in + 16u * q);
            __syncthreads();
            // ---- B: thread <-> sample in stream order ----
            for (uint32_t j = lane; j < total; j += rs::kTile) {
                const unsigned char* q = image + pp::image_offset(head, j, FMT);
                uint32_t raw;
                if (FMT == pp::S16) raw = *reinterpret_cast<const uint16_t*>(q);
                else if (FMT == pp::S24) raw = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
                else raw = *reinterpret_cast<const uint32_t*>(q);
                rows[(j % G) * rowFloats + rs::skew(part.lo + j / G)] = __uint_as_float(pu::decode_bits(FMT, raw));
            }
        } else {
            // ---- a wide source: thread <-> frame, the group's channels ----
            const unsigned char* stream = a.src + a.head;
#pragma unroll
            for (int ch = 0; ch < C; ++ch)
                if (g0 + ch < G)
                    for (uint32_t i = part.lo + lane; i < part.hi; i += rs::kTile)
                        rows[ch * rowFloats + rs::skew(i)] = staged_at<FMT>(stream, G, frame0 + (i - part.lo), g0 + ch);
        }
    }
    __syncthreads();
    if (f >= a.validOut) return;
    float acc[C];
    const uint64_t n = n0 + f;
    const uint32_t base = rs::lane_base(p, a.rowBase, t, n);
    rs::tap_sum<C>(a.table + (uint32_t)(n % p.L), p.L, p.T, [&](int ch, uint32_t k) { return rows[ch * rowFloats + rs::skew(base + k)]; }, acc);
#pragma unroll
    for (int ch = 0; ch < C; ++ch)
        if (g0 + ch < G) a.rows[g0 + ch][a.out0 + f] = acc[ch];
}

template <uint32_t FMT>
hipError_t convert_fmt(hipStream_t s, const ResourceLoadArgs& a) {
    const rs::Plan& p = a.plan;
    const uint32_t tiles = (a.validOut + rs::kTile - 1u) / rs::kTile, C = rl::convert_channels(p, a.G);
    if (C == rs::kGroup)
        hipLaunchKernelGGL((elemhip_resource_convert<FMT, (int)rs::kGroup>), dim3(tiles, (a.G + rs::kGroup - 1u) / rs::kGroup), dim3(rs::kTile), rs::in_lds_bytes(p, rs::kGroup), s, a);
    else if (C == 1u)
        hipLaunchKernelGGL((elemhip_resource_convert<FMT, 1>), dim3(tiles, a.G), dim3(rs::kTile), rs::in_lds_bytes(p, 1u), s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// what both launches require of a piece: the staged samples inside the staged bytes, the written frames inside every row
bool piece_ok(const ResourceLoadArgs& a, uint32_t format) {
    if (!pp::format_ok(format) || a.G == 0u || a.G > rl::kMaxChannels || !a.src) return false;
    if (a.srcBytes % 16u != 0u || a.head > 15u || (uint64_t)a.head + (uint64_t)a.validIn * a.G * pp::sample_bytes(format) > a.srcBytes) return false;
    if (a.out0 + a.validOut > a.rowFloats) return false;
    for (uint32_t g = 0; g < a.G; ++g) if (!a.rows[g]) return false;
    return true;
}

} // namespace

hipError_t launch_resource_copy(hipStream_t s, const ResourceLoadArgs& a, uint32_t format) {
    if (!piece_ok(a, format) || a.validIn != a.validOut || !a.rowTable) return hipErrorInvalidValue;
    if (a.validIn == 0u) return hipSuccess;
    const uint32_t lds = pp::lds_bytes(a.rowDwords, a.G);
    if (lds > 65536u) return hipErrorInvalidValue;
    const dim3 grid(rl::copy_tiles(a.validIn, a.G));
    switch (format) {
        case pp::S16: hipLaunchKernelGGL(elemhip_resource_copy<pp::S16>, grid, dim3(pp::kThreads), lds, s, a); break;
        case pp::S24: hipLaunchKernelGGL(elemhip_resource_copy<pp::S24>, grid, dim3(pp::kThreads), lds, s, a); break;
        default:      hipLaunchKernelGGL(elemhip_resource_copy<pp::F32>, grid, dim3(pp::kThreads), lds, s, a); break;
    }
    return hipGetLastError();
}

hipError_t launch_resource_convert(hipStream_t s, const ResourceLoadArgs& a, uint32_t format) {
    const rs::Plan& p = a.plan;
    if (!piece_ok(a, format) || !a.table || !a.rowBase) return hipErrorInvalidValue;
    if (p.L == 0u || p.M == 0u || p.L > rs::kMaxL || p.T == 0u || p.T > rs::kMaxT || p.T != 2u * p.Wc) return hipErrorInvalidValue;
    if (a.validOut == 0u) return hipSuccess;
    // the piece's outputs are those whose centre lies at or behind its first own frame, and what they read inside the file is staged:
    // every index the kernel forms follows from that
    const uint64_t lowest = a.out0 * p.M / p.L, highest = (a.out0 + a.validOut - 1u) * p.M / p.L;
    if (a.in0 != 0u && lowest + 1u < a.in0 + p.Wc) return hipErrorInvalidValue;
    if (a.totalIn < a.in0 + a.validIn || (a.in0 + a.validIn != a.totalIn && highest + p.Wc >= a.in0 + a.validIn)) return hipErrorInvalidValue;
    if ((uint64_t)a.validOut > 0xFFFFFFFFull - rs::kTile) return hipErrorInvalidValue;      // (a lane's frame number is 32 bits)
    switch (format) {
        case pp::S16: return convert_fmt<pp::S16>(s, a);
        case pp::S24: return convert_fmt<pp::S24>(s, a);
        default:      return convert_fmt<pp::F32>(s, a);
    }
}

} // namespace elemhip
