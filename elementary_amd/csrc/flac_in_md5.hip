// flac_in_md5.hip — the running STREAMINFO MD5 of FLAC inputs and resources (option "flac_in_md5"), behind the decode kernels of every
// launch set or staged piece: the samples the restore kernel left in the scratch — at the stream's own sample size, stereo undone,
// wasted bits restored, the range checked — enter their stream's digest where they lie, so no decoded sample goes to the host for it.
//   one wave per input stream, each with a job of its own (flac_in_md5.h): where its rows lie, which of its samples are new, whether
//   the stream ends here; a stream with nothing to hash and no finish does no work
//   the wave's walk of an update is flac_md5_wave.h's, shared with the delivery side (flac_md5.hip)
// The stage only reads the scratch: it runs on the decoder's stream, in front of the next set's parse that reuses it.
#include <hip/hip_runtime.h>

#include "flac_md5_wave.h"
#include "flac_in_md5.h"
#include "launch.h"

namespace elemhip {

namespace {

namespace fm = flac_md5;
namespace fi = flac_in_md5;

__global__ __launch_bounds__(64) void elemhip_flac_in_md5(FlacInMd5Args a) {
    __shared__ uint32_t m[fm::kChunkWords];
    const uint32_t s = blockIdx.x;
    const fi::Job job = a.jobs[s];
    if (job.count == 0u && job.finish == 0u) return;        // (the same in all lanes)
    const int32_t* rows = a.scratch + job.base;
    const uint32_t stride = job.stride;
    auto codes = [rows, stride](uint32_t g, uint32_t f) { return rows[(size_t)g * stride + f]; };
    fm::wave_update(m, a.records + s, codes, a.G, job.first, job.count, a.bits, job.finish != 0u, a.digests + (size_t)s * 16u);
}

} // namespace

// (the host's copy of the job table is checked against the scratch's size before anything is launched)
hipError_t launch_flac_in_md5(hipStream_t s, const FlacInMd5Args& a, const fi::Job* hostJobs, size_t scratchInts) {
    if (!fi::bits_ok(a.bits) || a.G == 0u || a.G > fi::kMaxChannels || !hostJobs) return hipErrorInvalidValue;
    if (!a.records || !a.jobs || !a.digests || (reinterpret_cast<uintptr_t>(a.digests) & 3u) || (reinterpret_cast<uintptr_t>(a.jobs) & 15u)) return hipErrorInvalidValue;
    bool work = false;
    for (uint32_t i = 0; i < a.numStreams; ++i) {
        const fi::Job& j = hostJobs[i];
        if (j.count == 0u && j.finish == 0u) continue;
        work = true;
        if (!a.scratch || (uint64_t)j.first + j.count > j.stride) return hipErrorInvalidValue;
        if ((uint64_t)j.base + (uint64_t)a.G * j.stride > scratchInts) return hipErrorInvalidValue;
    }
    if (!work) return hipSuccess;
    hipLaunchKernelGGL(elemhip_flac_in_md5, dim3(a.numStreams), dim3(64), 0, s, a);
    return hipGetLastError();
}

} // namespace elemhip
