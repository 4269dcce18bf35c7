// resample_in.hip — the input-rate converter of an offline render (Engine option "input_rate"): in front of a launch set's first level
// one kernel reads the set's stretch of the input where the H2D left it — interleaved streams of 16-bit, packed 24-bit or float
// samples at the INPUT's rate — decodes it (pcm_unpack.h) and converts it to the engine's rate, writing float32
// [block][channel][blockSize], the layout the render kernels read. It stands in the unpack kernel's place; only input-rate bytes cross
// the host link. The plan, the tables, the tap sum, the pull schedule (inputs_before) and the tile's index functions all come from
// resample.h, which tests/native/resample_in_host.cpp runs on the CPU lane by lane.
//   resample_in  workgroup <-> tile of 256 engine frames x one stream x C of its channels (C = 4; 1 for one-channel streams and where
//                four rows and their image would not fit 64 KB of LDS).
//                A/B  the tile's input stretch, decoded, into C padded LDS rows: the slots in front of the set come from the carried
//                     floats. A narrow stream (G <= C: every byte of it is this workgroup's) is loaded in aligned 16-byte pieces into
//                     an LDS image aligned like the stream and decoded from there, thread <-> sample in stream order; a wide one
//                     (G > C) is read sample by sample, thread <-> frame, the group's channels only. LDS is sized by C alone.
//                C    lane <-> engine frame: one coefficient load (rows in output order, consecutive lanes consecutive floats) serves
//                     the C channels' fused multiply-adds. Frames behind the call's last up to the set's last block's end: zeros.
//   history      thread <-> carried frame: the H decoded frames behind this set's stretch, from the stream and the old copy into the
//                OTHER copy — the kernel above only ever reads the old one. The host flips the copies.
// LDS conflicts (ds_read_b32 / ds_write_b32: bank = dword address mod 32 within a 32-lane half, equal addresses broadcast). Stage C at
// 1:4 (44100 into 176400): four neighbouring lanes share an address, a half-wave reads 8 or 9 consecutive dwords — conflict-free. At
// 160:147 (44100 into 48000) neighbours are 0 or 1 dword apart, a half-wave covers at most 30 dwords plus one pad — conflict-free too.
// When downsampling on this side (48000 into 44100) the picture is the output side's at the same ratio (resample.h: up to 2-way for
// that half-wave's read). Staging: the carried and the wide-stream writes are consecutive (one 2-way clash per pad crossed); stage B of
// a narrow stream writes G rows side by side, 32 / G consecutive slots each, and two rows' stretches can share banks depending on
// row_floats mod 32: 2-way at worst for G = 2, once per sample staged against T reads of it.
// Plain vector stores, no atomics.
#include <hip/hip_runtime.h>

#include "resample.h"
#include "pcm_unpack.h"
#include "launch.h"

namespace elemhip {

namespace {

namespace rs = resample;
namespace pp = pcm_pack;
namespace pu = pcm_unpack;

// sample (frame, g) of a stream of G channels, decoded
template <uint32_t FMT>
__device__ __forceinline__ float sample_at(const unsigned char* stream, uint32_t G, uint64_t frame, uint32_t g) {
    const unsigned char* p = stream + (size_t)(frame * G + g) * pp::sample_bytes(FMT);
    uint32_t raw;
    if (FMT == pp::S16) raw = *reinterpret_cast<const uint16_t*>(p);
    else if (FMT == pp::S24) raw = pu::load_raw(FMT, p);
    else raw = *reinterpret_cast<const uint32_t*>(p);
    return __uint_as_float(pu::decode_bits(FMT, raw));
}

template <uint32_t FMT, int C>
__global__ __launch_bounds__(rs::kTile) void elemhip_resample_in(ResampleInArgs a) {
    extern __shared__ __align__(16) unsigned char inLds[];
    float* rows = reinterpret_cast<float*>(inLds);
    const rs::Plan& p = a.plan;
    const uint32_t G = a.G, groups = (G + (uint32_t)C - 1u) / (uint32_t)C;
    const uint32_t lane = threadIdx.x, fFirst = blockIdx.x * rs::kTile, s = blockIdx.y / groups, g0 = (blockIdx.y % groups) * (uint32_t)C;
    const uint32_t f = fFirst + lane, bs = a.blockSize, nCh = a.numChannels, rowFloats = rs::row_floats(p);
    const unsigned char* stream = a.src + (size_t)s * a.streamStride;
    rs::Tile t{0, 0u};
    if (fFirst < a.validOut) {                      // (uniform: the barriers inside are met by every lane or by none)
        t = rs::tile_of(p, a.rowBase, a.n0, fFirst, a.validOut);
        const int64_t rel0 = t.jlo - (int64_t)a.t0;
        const rs::StreamPart part = rs::stream_part(rel0, t.span, a.validIn);
        // the slots the stream does not fill: carried frames in front, silence behind; a row behind the stream's last channel is silent
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const bool live = g0 + ch < G;
            const float* hist = a.histIn + ((size_t)s * G + (live ? g0 + ch : 0u)) * p.H;
            for (uint32_t i = lane; i < t.span; i += rs::kTile)
                if (!live || i < part.lo || i >= part.hi) rows[ch * rowFloats + rs::skew(i)] = live && i < part.lo ? rs::carried_at(hist, p.H, rel0 + (int64_t)i) : 0.0f;
        }
        if (part.hi > part.lo) {
            const uint64_t frame0 = (uint64_t)(rel0 + (int64_t)part.lo);
            if (G <= (uint32_t)C) {
                // ---- A: thread <-> 16-byte piece. The staging stride is a multiple of 16 and the stretch ends inside it, so every piece
                // is loaded whole; a byte in front of or behind the stretch is loaded and not decoded ----
                unsigned char* image = inLds + rs::in_image_offset(p, (uint32_t)C);
                const uint64_t c0 = frame0 * G * pp::sample_bytes(FMT);
                const uint32_t head = pp::image_head(c0), total = (part.hi - part.lo) * G;
                const uint32_t pieces = pp::piece_count(head, total * pp::sample_bytes(FMT));
                const unsigned char* in = stream + (size_t)(c0 - head);
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
                // ---- a wide stream: thread <-> frame, the group's channels ----
#pragma unroll
                for (int ch = 0; ch < C; ++ch)
                    if (g0 + ch < G)
                        for (uint32_t i = part.lo + lane; i < part.hi; i += rs::kTile)
                            rows[ch * rowFloats + rs::skew(i)] = sample_at<FMT>(stream, G, frame0 + (i - part.lo), g0 + ch);
            }
        }
    }
    __syncthreads();
    if ((uint64_t)f >= (uint64_t)a.numBlocks * bs) return;
    float acc[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) acc[ch] = 0.0f;
    if (f < a.validOut) {
        const uint64_t n = a.n0 + f;
        const uint32_t base = rs::lane_base(p, a.rowBase, t, n);
        rs::tap_sum<C>(a.table + (uint32_t)(n % p.L), p.L, p.T, [&](int ch, uint32_t k) { return rows[ch * rowFloats + rs::skew(base + k)]; }, acc);
    }
    float* out = a.dst + ((size_t)(f / bs) * nCh + (size_t)s * G + g0) * bs + f % bs;
#pragma unroll
    for (int ch = 0; ch < C; ++ch)
        if (g0 + ch < G) out[(size_t)ch * bs] = acc[ch];
}

template <uint32_t FMT>
__global__ __launch_bounds__(256) void elemhip_resample_in_history(ResampleInArgs a) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x, c = blockIdx.y, H = a.plan.H, G = a.G;
    if (j >= H) return;
    const unsigned char* stream = a.src + (size_t)(c / G) * a.streamStride;
    a.histOut[(size_t)c * H + j] = rs::history_pull([&](uint32_t fr) { return sample_at<FMT>(stream, G, fr, c % G); }, a.histIn + (size_t)c * H, a.validIn, H, j);
}

template <uint32_t FMT>
hipError_t launch_fmt(hipStream_t s, const ResampleInArgs& a) {
    const rs::Plan& p = a.plan;
    if (a.numBlocks) {
        const uint32_t tiles = (uint32_t)rs::ceil_div((uint64_t)a.numBlocks * a.blockSize, rs::kTile);
        if (a.G > 1u && rs::in_lds_bytes(p, rs::kGroup) <= 65536u)
            hipLaunchKernelGGL((elemhip_resample_in<FMT, (int)rs::kGroup>), dim3(tiles, a.numStreams * ((a.G + rs::kGroup - 1u) / rs::kGroup)), dim3(rs::kTile),
                               rs::in_lds_bytes(p, rs::kGroup), s, a);
        else if (rs::in_lds_bytes(p, 1u) <= 65536u)
            hipLaunchKernelGGL((elemhip_resample_in<FMT, 1>), dim3(tiles, a.numStreams * a.G), dim3(rs::kTile), rs::in_lds_bytes(p, 1u), s, a);
        else return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(elemhip_resample_in_history<FMT>, dim3((p.H + 255u) / 256u, a.numStreams * a.G), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace

hipError_t launch_resample_in(hipStream_t s, const ResampleInArgs& a, uint32_t format) {
    const rs::Plan& p = a.plan;
    if (!pp::format_ok(format) || a.G == 0u || a.G > pp::kMaxGroup || a.blockSize == 0u) return hipErrorInvalidValue;
    if (p.L == 0u || p.M == 0u || p.L > rs::kMaxL || p.M > (uint64_t)rs::kMaxGrowth * p.L || p.T == 0u || p.T > rs::kMaxT || p.H < p.T) return hipErrorInvalidValue;
    if (a.numStreams == 0u) return hipSuccess;
    // the set's engine frames are the programme's [n0, n0 + validOut), its stretch the inputs those pull and nothing else: every index
    // the kernels form follows from that
    if (a.t0 != rs::inputs_before(p, a.n0) || a.t0 + a.validIn != rs::inputs_before(p, a.n0 + a.validOut)) return hipErrorInvalidValue;
    // every block of the set is written (zeros behind validOut), every row lies inside [numBlocks][numChannels][blockSize]
    if ((uint64_t)a.numStreams * a.G > a.numChannels || (uint64_t)a.validOut > (uint64_t)a.numBlocks * a.blockSize) return hipErrorInvalidValue;
    if ((uint64_t)a.numBlocks * a.blockSize > 0xFFFFFFFFull - rs::kTile) return hipErrorInvalidValue;      // (a lane's frame number is 32 bits)
    if (a.streamStride % 16u != 0u || a.streamStride < (uint64_t)a.validIn * a.G * pp::sample_bytes(format)) return hipErrorInvalidValue;
    if ((uint64_t)a.numStreams * a.G > 65535u) return hipErrorInvalidValue;
    switch (format) {
        case pp::S16: return launch_fmt<pp::S16>(s, a);
        case pp::S24: return launch_fmt<pp::S24>(s, a);
        default:      return launch_fmt<pp::F32>(s, a);
    }
}

} // namespace elemhip
