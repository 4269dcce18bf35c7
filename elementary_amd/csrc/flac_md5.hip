// flac_md5.hip — the running STREAMINFO MD5 of FLAC delivery (option "flac_md5"), behind the stage kernel of every launch set: the
// set's new codes enter their stream's digest where they lie, so no sample byte goes to the host for it. The schedule, the message
// bytes and the rounds come from flac_md5.h, whose run() walks the same chunks serially on the host.
//   one wave per stream (MD5 chains its blocks; the streams are what is parallel)
//   per chunk of up to 64 blocks: a lane per message word gathers the chunk into LDS — the carried tail, the codes, and with `finish`
//   the padding and the bit length — then per block lane i forms K[i] + M[g(i)], and the chain, the same in every lane, takes its 64
//   sums from the lanes one by one; the bytes behind the last block go back to the record
#include <hip/hip_runtime.h>

#include "flac_md5.h"
#include "launch.h"

namespace elemhip {

namespace {

namespace fm = flac_md5;

__global__ __launch_bounds__(64) void elemhip_flac_md5(FlacMd5Args a) {
    __shared__ uint32_t m[fm::kChunkWords];
    const uint32_t lane = threadIdx.x, s = blockIdx.x;
    fm::Record* rec = a.records + s;
    const int32_t* rows = a.codes + (size_t)s * a.G * a.cap;
    const uint32_t cap = a.cap;
    auto codes = [rows, cap](uint32_t g, uint32_t f) { return rows[(size_t)g * cap + f]; };
    const fm::Job j = fm::make_job(rec->bytes, a.G, a.first, a.count, a.bits, a.finish != 0u);
    // The chaining value is the same in every lane, and as such the compiler would chain on the scalar unit, where a rotation is three
    // instructions and every round pays a trip through the vector unit. Counting the lanes below this one under an empty mask adds
    // nothing to a value and keeps it in a vector register: v_bfi, v_add3, v_alignbit, v_add per round, the sum from its lane as an SGPR.
    uint32_t h0 = __builtin_amdgcn_mbcnt_lo(0u, rec->h[0]), h1 = __builtin_amdgcn_mbcnt_lo(0u, rec->h[1]);
    uint32_t h2 = __builtin_amdgcn_mbcnt_lo(0u, rec->h[2]), h3 = __builtin_amdgcn_mbcnt_lo(0u, rec->h[3]);
    const uint32_t kl = fm::k_of(lane), wl = fm::word_of(lane);
    // (every loop bound below is the same in all lanes: the barriers stand in wave-uniform control flow)
    for (fm::Chunk c = fm::first_chunk(j);; fm::next_chunk(j, c)) {
        for (uint32_t w = lane; w < 16u * c.blocks; w += 64u) m[w] = fm::chunk_word(j, c, rec->tail, codes, 4u * w);
        __syncthreads();
        for (uint32_t b = 0; b < c.blocks; ++b) {
            const int x = (int)(kl + m[16u * b + wl]);
            uint32_t p = h0, q = h1, r = h2, t = h3;
#pragma unroll
            for (uint32_t i = 0; i < 64u; ++i) fm::round(i, (uint32_t)__builtin_amdgcn_readlane(x, (int)i), p, q, r, t);
            h0 += p; h1 += q; h2 += r; h3 += t;
        }
        __syncthreads();
        if (!fm::last_chunk(j, c)) continue;
        // the bytes behind the last block: the new tail (with no whole block a lane reads the old tail's byte it then writes)
        const uint32_t n = fm::leftover(j);
        uint32_t keep = 0u;
        if (lane < n) keep = fm::chunk_byte(j, c, rec->tail, codes, 64u * c.blocks + lane);
        __syncthreads();
        if (lane < n) rec->tail[lane] = (uint8_t)keep;
        break;
    }
    if (lane == 0u) {
        rec->h[0] = h0; rec->h[1] = h1; rec->h[2] = h2; rec->h[3] = h3;
        rec->bytes += (uint64_t)a.count * j.FB;
    }
    if (a.finish && lane < 4u)          // little-endian words are the digest's bytes
        reinterpret_cast<uint32_t*>(a.digests + (size_t)s * 16u)[lane] = lane == 0u ? h0 : lane == 1u ? h1 : lane == 2u ? h2 : h3;
}

} // namespace

hipError_t launch_flac_md5(hipStream_t s, const FlacMd5Args& a) {
    if (!fm::bits_ok(a.bits) || a.G == 0u || a.G > 8u || (uint64_t)a.first + a.count > a.cap) return hipErrorInvalidValue;
    if (!a.records || (a.count && !a.codes) || (a.finish && (!a.digests || (reinterpret_cast<uintptr_t>(a.digests) & 3u)))) return hipErrorInvalidValue;
    if (a.numStreams == 0u || (a.count == 0u && !a.finish)) return hipSuccess;
    hipLaunchKernelGGL(elemhip_flac_md5, dim3(a.numStreams), dim3(64), 0, s, a);
    return hipGetLastError();
}

} // namespace elemhip
