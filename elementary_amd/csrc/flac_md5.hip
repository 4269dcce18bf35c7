// flac_md5.hip — the running STREAMINFO MD5 of FLAC delivery (option "flac_md5"), behind the stage kernel of every launch set: the
// set's new codes enter their stream's digest where they lie, so no sample byte goes to the host for it. The schedule, the message
// bytes and the rounds come from flac_md5.h, whose run() walks the same chunks serially on the host.
//   one wave per stream (MD5 chains its blocks; the streams are what is parallel); the wave's walk of an update — the gather into LDS,
//   the chain, the tail — is flac_md5_wave.h's, shared with the input side (flac_in_md5.hip)
#include <hip/hip_runtime.h>

#include "flac_md5_wave.h"
#include "launch.h"

namespace elemhip {

namespace {

namespace fm = flac_md5;

__global__ __launch_bounds__(64) void elemhip_flac_md5(FlacMd5Args a) {
    __shared__ uint32_t m[fm::kChunkWords];
    const uint32_t s = blockIdx.x;
    const int32_t* rows = a.codes + (size_t)s * a.G * a.cap;
    const uint32_t cap = a.cap;
    auto codes = [rows, cap](uint32_t g, uint32_t f) { return rows[(size_t)g * cap + f]; };
    fm::wave_update(m, a.records + s, codes, a.G, a.first, a.count, a.bits, a.finish != 0u, a.digests + (size_t)s * 16u);
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
