// noise_shape.hip — noise-shaped requantisation in front of s16 / s24 / FLAC delivery (elemhip_noise_shape_set; the arithmetic, the
// tile schedule and the LDS layout: noise_shape.h, which tests/native/noise_shape_host.cpp runs on the CPU). A launch set's delivered
// frames, float32 [block][channel][blockSize] in HBM, become int32 codes in a buffer of the same shape, which the pack kernel and the
// FLAC stage kernel then read in place of quantising for themselves.
//
// The quantiser sits inside its own feedback loop: a channel is serial in time, channels are independent. One workgroup takes
// kChannels channels and walks the set's tiles in order, three phases per tile:
//   A  all lanes, along the rows: the float's split and the dither's three hashes — everything that does not depend on the loop —
//      as (xi, xf + dq | dq) pairs into the channels' LDS rows
//   B  a lane per channel: K multiply-adds and a dozen integer operations per frame, the errors in registers (the frame loop is
//      unrolled K times, so the shift of e[] is a renaming), pairs read 8 bytes at a time from rows skewed onto distinct banks
//   C  all lanes, along the rows: the codes to HBM
// The channels' states are read at the workgroup's start and written back at its end, in place: only this stream touches them.
#include <hip/hip_runtime.h>

#include "noise_shape.h"
#include "launch.h"

namespace elemhip {

namespace {

namespace ns = noise_shape;
namespace pp = pcm_pack;

template <uint32_t K>
__global__ __launch_bounds__(ns::kThreads) void elemhip_noise_shape(NoiseShapeArgs a) {
    __shared__ __align__(8) int32_t pairs[ns::kPairDwords];
    __shared__ int32_t codes[ns::kCodeDwords];

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t bs = a.blockSize, c0 = blockIdx.x * ns::kChannels, chn = ns::group_channels(a.numChannels, blockIdx.x);
    const uint32_t tpb = ns::tiles_per_block(bs), tiles = ns::tile_count(bs, a.validFrames);
    const int32_t lo = ns::code_min(a.bits), hi = ns::code_max(a.bits);
    const bool walker = tid < chn;                 // phase B's lanes: the first chn of wave 0

    int32_t cq[K], e[K];
    uint32_t sat = 0u;
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) { cq[k] = a.cq[k]; e[k] = walker ? a.state[c0 + tid].e[k] : 0; }

    for (uint32_t j = 0; j < tiles; ++j) {
        const uint32_t b = j / tpb, ti = j % tpb, f0 = ns::tile_first(ti);
        const uint32_t n = ns::tile_valid(bs, b, ti, a.validFrames);
        if (n == 0u) continue;                     // (uniform: the tile lies behind the last delivered frame)
        const int64_t tTile = a.time0 + (int64_t)((uint64_t)b * bs + f0);

        // ---- A ----
        for (uint32_t i = 0, g = ns::sweep_row(wave, 0u); g < chn; g = ns::sweep_row(wave, ++i)) {
            const float* row = a.src + ns::sample_index(bs, a.numChannels, b, c0 + g, f0);
            const uint32_t k0 = pp::channel_key(a.seed, c0 + g);
            const uint32_t hi0 = (uint32_t)((uint64_t)tTile >> 32), hk0 = pp::hi_key(k0, hi0);
            for (uint32_t q = 0, f = ns::sweep_frame(lane, 0u); f < n; f = ns::sweep_frame(lane, ++q)) {
                int32_t dq = 0;
                if (a.dither) {
                    const uint64_t t = (uint64_t)(tTile + (int64_t)f);
                    const uint32_t th = (uint32_t)(t >> 32);
                    dq = ns::dither_q8(th == hi0 ? hk0 : pp::hi_key(k0, th), (uint32_t)(t & 0xFFFFFFFFu));
                }
                const ns::Split s = ns::split(row[f], a.bits, dq);
                *reinterpret_cast<int2*>(pairs + ns::pair_dword(g, f)) = make_int2(s.xi, s.packed);
            }
        }
        __syncthreads();

        // ---- B ----
        if (walker) {
            const int32_t* in = pairs + ns::pair_dword(tid, 0u);
            int32_t* out = codes + ns::code_dword(tid, 0u);
#pragma unroll K
            for (uint32_t f = 0; f < n; ++f) {
                const int2 p = *reinterpret_cast<const int2*>(in + 2u * f);
                int32_t acc = 0;
#pragma unroll
                for (uint32_t k = 0; k < K; ++k) acc += __mul24(cq[k], e[k]);
                const ns::Step s = ns::step(ns::Split{p.x, p.y}, acc, lo, hi);
#pragma unroll
                for (uint32_t k = K - 1u; k > 0u; --k) e[k] = e[k - 1u];
                e[0] = s.err;
                sat += s.sat;
                out[f] = s.code;
            }
        }
        __syncthreads();

        // ---- C ----
        for (uint32_t i = 0, g = ns::sweep_row(wave, 0u); g < chn; g = ns::sweep_row(wave, ++i)) {
            int32_t* row = a.dst + ns::sample_index(bs, a.numChannels, b, c0 + g, f0);
            for (uint32_t q = 0, f = ns::sweep_frame(lane, 0u); f < n; f = ns::sweep_frame(lane, ++q)) row[f] = codes[ns::code_dword(g, f)];
        }
        // (the next tile's phase A writes `pairs`, which phase B has left behind the barrier above; its phase B writes `codes` behind
        //  the barrier that follows that phase A, which every lane passes only after this phase C)
    }

    if (walker) {
        ns::ChannelState* st = a.state + c0 + tid;
#pragma unroll
        for (uint32_t k = 0; k < K; ++k) st->e[k] = e[k];
        st->saturated += sat;
    }
}

template <uint32_t K> void launch_k(hipStream_t s, const NoiseShapeArgs& a) {
    hipLaunchKernelGGL(elemhip_noise_shape<K>, dim3(ns::group_count(a.numChannels)), dim3(ns::kThreads), 0, s, a);
}

} // namespace

hipError_t launch_noise_shape(hipStream_t s, const NoiseShapeArgs& a) {
    if (!ns::taps_ok(a.taps) || !ns::bits_ok(a.bits) || a.blockSize == 0u || a.blockSize > ns::kMaxBlock) return hipErrorInvalidValue;
    if (a.numChannels == 0u || a.validFrames == 0u) return hipSuccess;
    switch (a.taps) {
        case 1: launch_k<1>(s, a); break;   case 2: launch_k<2>(s, a); break;   case 3: launch_k<3>(s, a); break;
        case 4: launch_k<4>(s, a); break;   case 5: launch_k<5>(s, a); break;   case 6: launch_k<6>(s, a); break;
        case 7: launch_k<7>(s, a); break;   case 8: launch_k<8>(s, a); break;   case 9: launch_k<9>(s, a); break;
        case 10: launch_k<10>(s, a); break; case 11: launch_k<11>(s, a); break; default: launch_k<12>(s, a); break;
    }
    return hipGetLastError();
}

} // namespace elemhip
