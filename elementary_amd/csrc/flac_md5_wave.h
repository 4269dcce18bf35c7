// flac_md5_wave.h — one update of flac_md5.h's schedule walked by one wave: what flac_md5.hip (FLAC delivery) and flac_in_md5.hip (FLAC
// input) share. Device code only.
//   per chunk of up to 64 blocks: a lane per message word gathers the chunk into LDS — the carried tail, the codes, and with `finish`
//   the padding and the bit length — then per block lane i forms K[i] + M[g(i)], and the chain, the same in every lane, takes its 64
//   sums from the lanes one by one; the bytes behind the last block go back to the record
#ifndef ELEMHIP_FLAC_MD5_WAVE_H
#define ELEMHIP_FLAC_MD5_WAVE_H
#include <hip/hip_runtime.h>

#include "flac_md5.h"

namespace flac_md5 {

// `count` frames from `first` on of codes(g, f) enter the record's digest; with `finish` the message ends here and its 16 bytes go to
// `digest` (4-byte aligned). Called by all 64 lanes of a one-wave block with the same arguments; m: kChunkWords words of LDS.
template <class Codes>
__device__ __forceinline__ void wave_update(uint32_t* m, Record* rec, const Codes& codes, uint32_t G, uint32_t first, uint32_t count, uint32_t bits,
                                            bool finish, uint8_t* digest) {
    const uint32_t lane = threadIdx.x;
    const Job j = make_job(rec->bytes, G, first, count, bits, finish);
    // The chaining value is the same in every lane, and as such the compiler would chain on the scalar unit, where a rotation is three
    // instructions and every round pays a trip through the vector unit. Counting the lanes below this one under an empty mask adds
    // nothing to a value and keeps it in a vector register: v_bfi, v_add3, v_alignbit, v_add per round, the sum from its lane as an SGPR.
    uint32_t h0 = __builtin_amdgcn_mbcnt_lo(0u, rec->h[0]), h1 = __builtin_amdgcn_mbcnt_lo(0u, rec->h[1]);
    uint32_t h2 = __builtin_amdgcn_mbcnt_lo(0u, rec->h[2]), h3 = __builtin_amdgcn_mbcnt_lo(0u, rec->h[3]);
    const uint32_t kl = k_of(lane), wl = word_of(lane);
    // (every loop bound below is the same in all lanes: the barriers stand in wave-uniform control flow)
    for (Chunk c = first_chunk(j);; next_chunk(j, c)) {
        for (uint32_t w = lane; w < 16u * c.blocks; w += 64u) m[w] = chunk_word(j, c, rec->tail, codes, 4u * w);
        __syncthreads();
        for (uint32_t b = 0; b < c.blocks; ++b) {
            const int x = (int)(kl + m[16u * b + wl]);
            uint32_t p = h0, q = h1, r = h2, t = h3;
#pragma unroll
            for (uint32_t i = 0; i < 64u; ++i) round(i, (uint32_t)__builtin_amdgcn_readlane(x, (int)i), p, q, r, t);
            h0 += p; h1 += q; h2 += r; h3 += t;
        }
        __syncthreads();
        if (!last_chunk(j, c)) continue;
        // the bytes behind the last block: the new tail (with no whole block a lane reads the old tail's byte it then writes)
        const uint32_t n = leftover(j);
        uint32_t keep = 0u;
        if (lane < n) keep = chunk_byte(j, c, rec->tail, codes, 64u * c.blocks + lane);
        __syncthreads();
        if (lane < n) rec->tail[lane] = (uint8_t)keep;
        break;
    }
    if (lane == 0u) {
        rec->h[0] = h0; rec->h[1] = h1; rec->h[2] = h2; rec->h[3] = h3;
        rec->bytes += (uint64_t)count * j.FB;
    }
    if (finish && lane < 4u)            // little-endian words are the digest's bytes
        reinterpret_cast<uint32_t*>(digest)[lane] = lane == 0u ? h0 : lane == 1u ? h1 : lane == 2u ? h2 : h3;
}

} // namespace flac_md5
#endif
