// flac_decode.hip — the first stage of an offline render fed with FLAC (engine_flac_in.cpp): the FLAC frames that cover a launch set's
// input frames, staged in HBM as they lie in the file, become the interleaved s16 / s24 image the H2D copy of a PCM stream of the same
// samples would leave — the unpack kernel or the input-rate converter runs behind it unchanged. The arithmetic, the bounded bit
// reader and the lane functions are flac_decode.h's, which tests/native/flac_decode_host.cpp runs on the CPU.
//   parse    one lane per (stream, FLAC frame), a wave's lanes on consecutive frames of a stream: header and subframes in bit order
//            through the lane's own 64-bit window; descriptors, warm-up samples and residuals at their sample positions in the scratch
//   restore  one workgroup per (stream, FLAC frame), one wave per channel: the CRC-16 from every lane's chunk; FIXED as prefix sums
//            across the wave in chunks of 64 with carry, LPC as lane 0's serial loop, CONSTANT a fill; wasted bits; then all lanes undo
//            the stereo decorrelation in place and check the range; the frame's reason and the set's error record
//   store    thread <-> 16-byte piece of a stream's image, one 16-byte store each: zeros past the stream's end and for a failed frame
// The entropy code is serial inside a frame, so the parallelism of `parse` is across frames and streams only; a set of C4 holds a few
// thousand frames. No LDS beyond the restore kernel's few words.
#include <hip/hip_runtime.h>

#include "flac_decode.h"
#include "launch.h"

namespace elemhip {

namespace {

namespace fd = flac_decode;

__global__ __launch_bounds__(64) void elemhip_flac_parse(FlacDecodeArgs a) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= a.numFrames) return;
    const FlacInFrame fr = a.frames[i];
    uint32_t assignment = fd::INDEPENDENT;
    const uint32_t reason = fd::parse_lane(a.staged + fr.byteOff, fr.len, a.G, a.bits, fr.n, reinterpret_cast<fd::Sub*>(a.subs) + (size_t)i * a.G,
                                           a.scratch + fr.scratchOff, fr.chStride, &assignment);
    a.state[i] = reason | (assignment << 8);
}

__device__ __forceinline__ uint32_t wave_scan(uint32_t v, uint32_t lane) {      // inclusive, mod 2^32
#pragma unroll
    for (uint32_t o = 1u; o < 64u; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)v, o);
        if (lane >= o) v += up;
    }
    return v;
}

__global__ __launch_bounds__(64 * fd::kMaxChannels) void elemhip_flac_restore(FlacDecodeArgs a) {
    __shared__ uint32_t crcOf[fd::kMaxChannels];
    __shared__ uint32_t bad;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, c = tid >> 6, threads = blockDim.x;
    const FlacInFrame fr = a.frames[blockIdx.x];
    const uint32_t st = a.state[blockIdx.x], assignment = st >> 8;
    const unsigned char* f = a.staged + fr.byteOff;
    const uint32_t n = fr.n, total = fr.len >= 2u ? fr.len - 2u : 0u;

    // ---- the CRC-16: every lane's chunk, advanced to the frame's end ----
    uint32_t crc = fd::lane_crc(f, total, tid, threads);
    for (uint32_t o = 32u; o > 0u; o >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, (int)o);
    if (lane == 0u) crcOf[c] = crc;
    if (tid == 0u) bad = 0u;
    __syncthreads();
    crc = 0u;
    for (uint32_t w = 0; w < a.G; ++w) crc ^= crcOf[w];
    uint32_t reason = st & 0xFFu;
    if (fr.len < 2u) reason = fd::BITS_MISSING;
    else if (crc != (((uint32_t)f[total] << 8) | f[total + 1u])) reason = fd::BAD_CRC;

    if (reason == fd::OK) {      // (uniform over the workgroup)
        // ---- wave c restores channel c in place; lane l owns the positions l, l + 64, ... in every pass ----
        const fd::Sub* sub = reinterpret_cast<const fd::Sub*>(a.subs) + (size_t)blockIdx.x * a.G + c;
        uint32_t* u = reinterpret_cast<uint32_t*>(a.scratch + fr.scratchOff + (size_t)c * fr.chStride);
        const uint32_t kind = sub->kind, order = sub->order, wasted = sub->wasted;
        if (kind == fd::CONSTANT) {
            const uint32_t v = n ? u[0] << wasted : 0u;
            for (uint32_t i = lane; i < n; i += 64u) u[i] = v;
        } else if (kind == fd::VERBATIM || (kind == fd::FIXED && order == 0u)) {
            if (wasted) for (uint32_t i = lane; i < n; i += 64u) u[i] <<= wasted;
        } else if (kind == fd::FIXED) {
            const uint32_t s0 = u[0], s1 = order > 1u ? u[1] : 0u, s2 = order > 2u ? u[2] : 0u, s3 = order > 3u ? u[3] : 0u;
            for (uint32_t p = order; p >= 1u; --p) {
                const uint32_t seed = fd::fixed_seed(s0, s1, s2, s3, p), sh = p == 1u ? wasted : 0u;
                uint32_t carry = 0u;
                for (uint32_t base = 0; base < n; base += 64u) {
                    const uint32_t i = base + lane;
                    uint32_t v = i < n && i + 1u >= p ? (i + 1u == p ? seed : u[i]) : 0u;
                    v = wave_scan(v, lane) + carry;
                    if (i < n && i + 1u >= p) u[i] = v << sh;
                    carry = (uint32_t)__shfl((int)v, 63);
                }
            }
            // (a lane reads in pass p - 1 what it wrote itself in pass p; pass 1 rewrites every position, shifted by the wasted bits)
        } else if (lane == 0u) {                                      // LPC: one lane, the floor shift makes it non-linear
            int32_t* x = reinterpret_cast<int32_t*>(u);
            for (uint32_t i = order; i < n; ++i) x[i] = fd::lpc_sample(*sub, x, i);
            if (wasted) for (uint32_t i = 0; i < n; ++i) x[i] = fd::unwaste(x[i], wasted);
        }
    }
    __syncthreads();
    if (reason == fd::OK) {
        // ---- all lanes: the stereo undo in place, the range check ----
        int32_t* x = a.scratch + fr.scratchOff;
        bool ok = true;
        if (assignment != fd::INDEPENDENT) {
            for (uint32_t i = tid; i < n; i += threads) {
                int32_t l = x[i], r = x[fr.chStride + i];
                ok = fd::stereo_pair(assignment, a.bits, l, r) && ok;
                x[i] = l; x[fr.chStride + i] = r;
            }
        } else {
            for (uint32_t ch = 0; ch < a.G; ++ch)
                for (uint32_t i = tid; i < n; i += threads) ok = fd::in_range(x[(size_t)ch * fr.chStride + i], a.bits) && ok;
        }
        if (!ok) atomicOr(&bad, 1u);
    }
    __syncthreads();
    if (tid == 0u) {
        if (reason == fd::OK && bad) reason = fd::OUT_OF_RANGE;
        a.state[blockIdx.x] = reason | (assignment << 8);
        if (reason != fd::OK) {
            atomicAdd(&a.error->count, 1u);
            atomicMax(&a.error->first, ~(((unsigned long long)blockIdx.x << 8) | reason));      // (zeroed: the complement's maximum)
        }
    }
}

__global__ __launch_bounds__(256) void elemhip_flac_store(FlacDecodeArgs a) {
    const uint32_t piece = blockIdx.x * 256u + threadIdx.x, s = blockIdx.y;
    if ((uint64_t)piece * 16u >= a.streamStride) return;
    const FlacInStream str = a.streams[s];
    const int32_t* x = a.scratch + str.scratchBase;
    const uint32_t* state = a.state + str.firstFrame;
    __align__(16) uint8_t out[16];
    fd::image_piece(a.bits, a.G, a.valid, str.have, piece, [&](uint32_t g, uint32_t frame) -> int32_t {
        const uint32_t at = str.skip + frame, j = at / str.blockSize;
        if (j >= str.frames || (state[j] & 0xFFu) != fd::OK) return 0;
        return x[(size_t)g * str.covered + at];
    }, out);
    *reinterpret_cast<uint4*>(a.dst + (size_t)s * a.streamStride + (size_t)piece * 16u) = *reinterpret_cast<const uint4*>(out);
}

} // namespace

hipError_t launch_flac_decode(hipStream_t s, const FlacDecodeArgs& a, const FlacInFrame* hostFrames, const FlacInStream* hostStreams,
                              size_t stagedBytes, size_t scratchInts) {
    if (!fd::bits_ok(a.bits) || a.G == 0u || a.G > fd::kMaxChannels || a.streamStride % 16u != 0u) return hipErrorInvalidValue;
    if (a.numStreams == 0u) return hipSuccess;
    if (a.streamStride < (uint64_t)a.valid * a.G * (a.bits <= 16u ? 2u : 3u) || a.streamStride / 16u > 0xFFFFFFFFull) return hipErrorInvalidValue;
    // every record inside its buffers: the kernels clamp to the record, the records are checked here
    for (uint32_t i = 0; i < a.numFrames; ++i) {
        const FlacInFrame& f = hostFrames[i];
        if ((uint64_t)f.byteOff + f.len > stagedBytes || f.n == 0u || f.n > fd::kMaxBlock || f.stream >= a.numStreams) return hipErrorInvalidValue;
        if (f.n > f.chStride || (uint64_t)f.scratchOff + (uint64_t)(a.G - 1u) * f.chStride + f.n > scratchInts) return hipErrorInvalidValue;
    }
    for (uint32_t t = 0; t < a.numStreams; ++t) {
        const FlacInStream& st = hostStreams[t];
        if ((uint64_t)st.firstFrame + st.frames > a.numFrames || st.have > a.valid) return hipErrorInvalidValue;
        if (st.have && (st.blockSize == 0u || (uint64_t)st.skip + st.have > st.covered)) return hipErrorInvalidValue;
        if ((uint64_t)st.scratchBase + (uint64_t)a.G * st.covered > scratchInts) return hipErrorInvalidValue;
    }
    if (a.numFrames) {
        hipLaunchKernelGGL(elemhip_flac_parse, dim3((a.numFrames + 63u) / 64u), dim3(64), 0, s, a);
        hipLaunchKernelGGL(elemhip_flac_restore, dim3(a.numFrames), dim3(64u * a.G), 0, s, a);
    }
    const uint32_t pieces = (uint32_t)(a.streamStride / 16u);
    if (pieces) hipLaunchKernelGGL(elemhip_flac_store, dim3((pieces + 255u) / 256u, a.numStreams), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace elemhip
