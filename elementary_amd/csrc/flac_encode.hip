// flac_encode.hip — the last stage of an offline render delivered as FLAC (Engine::processBlocksFlac), in the pack kernel's place: a
// launch set's delivered frames, float32 [block][channel][blockSize] in HBM, become whole RFC 9639 frames per stream. The arithmetic,
// the decision rules, the lane schedule and the shared-memory layout come from flac_encode.h, which tests/native/flac_encode_host.cpp
// runs on the CPU lane by lane:
//   stage     thread <-> frame of a channel row: the carried codes, then the set's floats quantised as pcm_pack quantises them
//   encode    one workgroup per (FLAC frame, subframe candidate): exact bit counts up the partition tree, the decision, the bits
//             ORed into a zeroed LDS image, the image's words to the candidate's slot. With an LPC order (flac_lpc.h) the second
//             instantiation runs: windowed samples, the lanes' lags reduced over the workgroup, lane 0's recursion and quantisation,
//             and the same leaf / tree passes once more per priced LPC order
//   assemble  one workgroup per (stream, FLAC frame): stereo mode, header, subframes shift-copied, CRC-16 of lane chunks combined,
//             16-byte stores where a piece of the stream is whole
#include <hip/hip_runtime.h>

#include "flac_encode.h"
#include "launch.h"

namespace elemhip {

namespace {

namespace fe = flac_encode;
namespace pp = pcm_pack;

struct OrLds { __device__ void operator()(uint32_t* p, uint32_t v) const { atomicOr(p, v); } };
struct AddLds { __device__ void operator()(uint32_t* p, uint32_t v) const { atomicAdd(p, v); } };

// frames of a channel row a workgroup stages: kStageRun rounds of 256 consecutive frames, the statistics folded once per workgroup
constexpr uint32_t kStageRun = 8;

__global__ __launch_bounds__(fe::kThreads) void elemhip_flac_stage(FlacStageArgs a) {
    __shared__ uint32_t red[3][4];
    const uint32_t c = blockIdx.y, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t total = a.open + a.validFrames, k0 = pp::channel_key(a.seed, c);
    int32_t* codes = a.codes + (size_t)c * a.cap;
    pp::ChannelStats acc{0u, 0u, 0u};
#pragma unroll
    for (uint32_t r = 0; r < kStageRun; ++r) {
        const uint32_t i = (blockIdx.x * kStageRun + r) * fe::kThreads + threadIdx.x;
        if (i < a.open) codes[i] = a.carry[(size_t)c * fe::kMaxFrame + i];
        else if (i < total) {
            const uint32_t f = i - a.open + a.srcOffset, b = f / a.blockSize;
            const size_t at = ((size_t)b * a.numChannels + c) * a.blockSize + (f - b * a.blockSize);
            const float x = a.src[at];
            acc = pp::stats_fold(x, acc);
            codes[i] = a.shaped ? a.shaped[at] : pp::quantise(x, a.bits, a.dither ? pp::dither(k0, a.time0 + (int64_t)f) : 0.0f);
        }
    }
    uint32_t peak = acc.peakBits, over = acc.over, nonf = acc.nonfinite;
#pragma unroll
    for (uint32_t o = 32u; o > 0u; o >>= 1) {
        peak = max(peak, (uint32_t)__shfl_xor((int)peak, (int)o));
        over += (uint32_t)__shfl_xor((int)over, (int)o);
        nonf += (uint32_t)__shfl_xor((int)nonf, (int)o);
    }
    if (lane == 0u) { red[0][wave] = peak; red[1][wave] = over; red[2][wave] = nonf; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        pp::ChannelStats* st = a.stats + c;
        peak = max(max(red[0][0], red[0][1]), max(red[0][2], red[0][3]));
        over = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        nonf = red[2][0] + red[2][1] + red[2][2] + red[2][3];
        if (peak) atomicMax(&st->peakBits, peak);
        if (over) atomicAdd(&st->over, over);
        if (nonf) atomicAdd(&st->nonfinite, nonf);
    }
}

__global__ __launch_bounds__(fe::kThreads) void elemhip_flac_carry(const int32_t* codes, int32_t* carry, uint32_t cap, uint32_t from, uint32_t count) {
    const uint32_t i = blockIdx.x * fe::kThreads + threadIdx.x, c = blockIdx.y;
    if (i < count) carry[(size_t)c * fe::kMaxFrame + i] = codes[(size_t)c * cap + from + i];
}

// sum over the block (every lane gets it); `red` = 4 words of LDS
__device__ uint32_t block_sum(uint32_t v, uint32_t* red) {
#pragma unroll
    for (uint32_t o = 32u; o > 0u; o >>= 1) v += (uint32_t)__shfl_xor((int)v, (int)o);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// The priced LPC orders' plan into w.lpc (every lane returns behind a barrier that publishes it). The windowed samples live in w.sums,
// which is free until the first leaf; the waves' partial lags pass through w.maxU as halves, [wave][lag] low words then high words.
__device__ void lpc_prepare(fe::Work& w, uint32_t n, uint32_t bits, uint32_t P, uint32_t lane) {
    for (uint32_t i = lane; i < n; i += fe::kThreads) w.sums[i] = (uint32_t)fe::lpc_windowed(w.codes[i], i, n);
    __syncthreads();
    int64_t acc[fe::kLpcLags];
#pragma unroll
    for (uint32_t k = 0; k < fe::kLpcLags; ++k) acc[k] = 0;
    fe::lpc_lags(w.sums, n, P, lane, fe::kThreads, acc);
#pragma unroll
    for (uint32_t k = 0; k < fe::kLpcLags; ++k) {
        long long v = acc[k];
#pragma unroll
        for (uint32_t o = 32u; o > 0u; o >>= 1) v += __shfl_xor(v, (int)o);
        if ((lane & 63u) == 0u) {
            w.maxU[(lane >> 6) * fe::kLpcLags + k] = (uint32_t)(uint64_t)v;
            w.maxU[(4u + (lane >> 6)) * fe::kLpcLags + k] = (uint32_t)((uint64_t)v >> 32);
        }
    }
    __syncthreads();            // the windowed samples are read, the halves written: the workspace may take the samples' place
    if (lane < fe::kLpcLags) {
        uint64_t sum = 0;
        for (uint32_t v = 0; v < 4u; ++v) sum += (uint64_t)w.maxU[v * fe::kLpcLags + lane] | ((uint64_t)w.maxU[(4u + v) * fe::kLpcLags + lane] << 32);
        w.lpcWork.lag[lane] = (int64_t)sum;
    }
    __syncthreads();
    if (lane == 0u) fe::lpc_design(w.lpcWork, P, n, bits, w.lpc);
    __syncthreads();
}

// kLpc: a.lpcOrder > 0 (launch_flac_encode chooses the instantiation: without an LPC order the kernel is the one it was)
template <bool kLpc>
__global__ __launch_bounds__(fe::kThreads) void elemhip_flac_encode(FlacEncodeArgs a) {
    __shared__ fe::Work w;
    __shared__ uint32_t waveSum[4];
    const uint32_t lane = threadIdx.x, frame = blockIdx.x, cands = fe::candidates(a.G);
    const uint32_t s = blockIdx.y / cands, cand = blockIdx.y % cands;
    const uint32_t n = a.n, bits = a.bits, bps = fe::candidate_bps(a.G, bits, cand);
    {
        const int32_t* c0 = a.codes + (size_t)(s * a.G + (a.G == 2u ? 0u : cand)) * a.cap + (size_t)frame * a.flacFrame;
        const int32_t* c1 = a.G == 2u ? c0 + a.cap : c0;
        for (uint32_t i = lane; i < n; i += fe::kThreads) w.codes[i] = fe::candidate_sample(a.G, cand, c0[i], c1[i]);
        uint32_t* tot = &w.total[0][0];
        if (lane < fe::kRows * fe::kLevels) tot[lane] = 0u;
        if (lane < fe::kRows) w.rootMax[lane] = 0u;
    }
    __syncthreads();
    const fe::Shape sh = fe::shape(n);
    for (uint32_t order = 0; order <= fe::max_order(n); ++order) {
        fe::leaf(w, sh, bits, order, lane);
        __syncthreads();
        for (uint32_t L = 9u; L-- > 0u;) {
            fe::tree_level(w, sh, bits, order, L, lane, AddLds{});
            __syncthreads();
        }
    }
    if (kLpc) {
        lpc_prepare(w, n, bits, a.lpcOrder, lane);
        for (uint32_t slot = 0; slot < w.lpc.count; ++slot) {
            if (w.lpc.drop[slot] != fe::LPC_OK) continue;
            fe::leaf_lpc(w, sh, bits, slot, lane);
            __syncthreads();
            for (uint32_t L = 9u; L-- > 0u;) {
                fe::tree_level(w, sh, bits, fe::lpc_row(slot), L, lane, AddLds{});
                __syncthreads();
            }
        }
    }
    const fe::Decision d = fe::decide(sh, bps, w.total, w.rootMax, kLpc ? &w.lpc : nullptr);
    if (!kLpc && d.kind == fe::LPC) __builtin_unreachable();      // (no LPC code in the instantiation without)
    // exclusive scan of the lanes' code lengths: inside the wave by shuffles, the waves' sums through LDS
    const uint32_t len = fe::lane_bits(w, sh, bits, d, lane);
    uint32_t incl = len;
#pragma unroll
    for (uint32_t o = 1u; o < 64u; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
        if ((lane & 63u) >= o) incl += up;
    }
    if ((lane & 63u) == 63u) waveSum[lane >> 6] = incl;
    uint32_t* image = w.sums;
    const uint32_t words = (d.bits + 31u) / 32u + 1u;
    for (uint32_t i = lane; i < words; i += fe::kThreads) image[i] = 0u;
    __syncthreads();
    uint32_t start = incl - len;
    for (uint32_t v = 0; v < (lane >> 6); ++v) start += waveSum[v];
    fe::lane_emit(w, image, sh, bits, bps, d, lane, start, OrLds{});
    __syncthreads();
    const size_t slot = ((size_t)s * a.numFrames + frame) * cands + cand;
    uint32_t* out = a.slots + slot * a.slotWords;
    for (uint32_t i = lane; i < words; i += fe::kThreads) out[i] = image[i];
    if (lane == 0u) a.subBits[slot] = d.bits;
}

// the stereo mode and the subframes' bits of frame j of stream s
__device__ uint32_t frame_sub_bits(const FlacEncodeArgs& a, uint32_t s, uint32_t j, uint32_t* modeOut) {
    const uint32_t cands = fe::candidates(a.G);
    const uint32_t* sb = a.subBits + ((size_t)s * a.numFrames + j) * cands;
    uint32_t mode = fe::INDEPENDENT, sum = 0;
    if (a.G == 2u) {
        mode = fe::choose_stereo(sb[0], sb[1], sb[2], sb[3]);
        sum = sb[fe::stereo_candidate(mode, 0u)] + sb[fe::stereo_candidate(mode, 1u)];
    } else for (uint32_t c = 0; c < a.G; ++c) sum += sb[c];
    if (modeOut) *modeOut = mode;
    return sum;
}

__global__ __launch_bounds__(fe::kThreads) void elemhip_flac_assemble(FlacEncodeArgs a) {
    __shared__ fe::FrameParts parts;
    __shared__ uint32_t red[4];
    const uint32_t lane = threadIdx.x, frame = blockIdx.x, s = blockIdx.y, cands = fe::candidates(a.G);
    // where the frame starts in its stream's buffer: the bytes of the frames in front of it
    uint32_t mine = 0;
    for (uint32_t j = lane; j < frame; j += fe::kThreads)
        mine += fe::frame_bytes(fe::header_bytes(a.n, a.flacFrame, a.rate, a.firstNumber + j), frame_sub_bits(a, s, j, nullptr));
    const uint32_t at = block_sum(mine, red);
    if (lane == 0u) {
        uint32_t mode;
        (void)frame_sub_bits(a, s, frame, &mode);
        parts.headerBytes = fe::header_put(a.n, a.flacFrame, a.rate, a.G, a.bits, mode, a.firstNumber + frame, parts.header);
        parts.count = a.G;
        uint64_t off = 0;
        for (uint32_t c = 0; c < a.G; ++c) {
            const uint32_t q = a.G == 2u ? fe::stereo_candidate(mode, c) : c;
            const size_t slot = ((size_t)s * a.numFrames + frame) * cands + q;
            parts.words[c] = a.slots + slot * a.slotWords;
            parts.offset[c] = off;
            off += a.subBits[slot];
        }
        parts.offset[a.G] = off;
    }
    __syncthreads();
    const uint32_t body = parts.headerBytes + (uint32_t)((parts.offset[parts.count] + 7u) / 8u), len = body + 2u;
    // CRC-16: every lane its chunk, advanced over what follows it; the XOR of all is the frame's
    uint32_t crc = fe::lane_crc(parts, body, lane);
#pragma unroll
    for (uint32_t o = 32u; o > 0u; o >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, (int)o);
    __syncthreads();
    if ((lane & 63u) == 0u) red[lane >> 6] = crc;
    __syncthreads();
    crc = red[0] ^ red[1] ^ red[2] ^ red[3];
    auto byteAt = [&](uint32_t i) -> uint32_t { return i < body ? fe::frame_byte(parts, i) : i == body ? (crc >> 8) & 0xFFu : crc & 0xFFu; };
    // the stretch [at, at + len) of the stream in 16-byte pieces of the buffer
    unsigned char* base = a.dst + (size_t)s * a.streamStride;
    const uint32_t head = fe::piece_first(at), pieces = pp::piece_count(head, len);
    for (uint32_t p = lane; p < pieces; p += fe::kThreads) {
        const uint32_t lo = 16u * p > head ? 16u * p : head, hi = 16u * p + 16u < head + len ? 16u * p + 16u : head + len;
        unsigned char* out = base + (size_t)(at - head);
        if (pp::piece_whole(p, head, len)) {
            uint32_t v[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                const uint32_t i = 16u * p + 4u * k - head;
                v[k] = byteAt(i) | (byteAt(i + 1u) << 8) | (byteAt(i + 2u) << 16) | (byteAt(i + 3u) << 24);
            }
            *reinterpret_cast<uint4*>(out + 16u * p) = make_uint4(v[0], v[1], v[2], v[3]);
            continue;
        }
#pragma clang loop vectorize(disable) unroll(disable)
        for (uint32_t o = lo; o < hi; ++o) out[o] = (unsigned char)byteAt(o - head);
    }
    if (lane == 0u) a.frameBytes[(size_t)s * a.numFrames + frame] = len;
}

} // namespace

hipError_t launch_flac_stage(hipStream_t s, const FlacStageArgs& a) {
    if (!fe::bits_ok(a.bits) || a.blockSize == 0u || a.open >= fe::kMaxFrame || (uint64_t)a.open + a.validFrames > a.cap) return hipErrorInvalidValue;
    const uint32_t total = a.open + a.validFrames;
    if (total == 0u || a.numChannels == 0u) return hipSuccess;
    hipLaunchKernelGGL(elemhip_flac_stage, dim3((total + fe::kThreads * kStageRun - 1u) / (fe::kThreads * kStageRun), a.numChannels), dim3(fe::kThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_flac_carry(hipStream_t s, const int32_t* codes, int32_t* carry, uint32_t numChannels, uint32_t cap, uint32_t flacFrame, uint32_t from, uint32_t count) {
    if (count >= flacFrame || flacFrame > fe::kMaxFrame || (uint64_t)from + count > cap) return hipErrorInvalidValue;
    if (count == 0u || numChannels == 0u) return hipSuccess;
    hipLaunchKernelGGL(elemhip_flac_carry, dim3((count + fe::kThreads - 1u) / fe::kThreads, numChannels), dim3(fe::kThreads), 0, s, codes, carry, cap, from, count);
    return hipGetLastError();
}

hipError_t launch_flac_encode(hipStream_t s, const FlacEncodeArgs& a) {
    if (!fe::bits_ok(a.bits) || !fe::frame_ok(a.flacFrame) || a.G == 0u || a.G > fe::kMaxChannels || a.n == 0u || a.n > a.flacFrame) return hipErrorInvalidValue;
    if (a.slotWords < fe::slot_words(a.flacFrame, a.bits) || (uint64_t)(a.numFrames - (a.numFrames ? 1u : 0u)) * a.flacFrame + a.n > a.cap) return hipErrorInvalidValue;
    if ((uint64_t)a.firstNumber + a.numFrames > 0x80000000ull || (a.n != a.flacFrame && a.numFrames > 1u)) return hipErrorInvalidValue;
    if (!fe::lpc_order_ok(a.lpcOrder)) return hipErrorInvalidValue;
    if (a.numFrames == 0u || a.numStreams == 0u) return hipSuccess;
    const dim3 grid(a.numFrames, a.numStreams * fe::candidates(a.G));
    if (a.lpcOrder > 0u) hipLaunchKernelGGL(elemhip_flac_encode<true>, grid, dim3(fe::kThreads), 0, s, a);
    else hipLaunchKernelGGL(elemhip_flac_encode<false>, grid, dim3(fe::kThreads), 0, s, a);
    hipLaunchKernelGGL(elemhip_flac_assemble, dim3(a.numFrames, a.numStreams), dim3(fe::kThreads), 0, s, a);
    return hipGetLastError();
}

} // namespace elemhip
