// fft_frames.hip — the `fft` analyzer node's relay kernel (wasm/FFT.h:92-132): one launch per event relay transforms every frame
// every fft node of the window hands on, one workgroup of 128 threads per frame. A workgroup gathers `size` samples of the node's
// device ring (8192 frames, or a relay window's history) at the frame's read position (wrapped), multiplies by the Blackman-Harris table of that size, runs the
// real FFT entirely in LDS (fft_frames.h: packed complex transform of size / 2 points + split step, double arithmetic) and stores
// real[0 .. size/2] | imag[0 .. size/2] as float32 into the relay buffer. Launched on the relay's own stream, outside the render lock.
#include <hip/hip_runtime.h>

#include "fft_frames.h"
#include "launch.h"

namespace elemhip {

namespace {

constexpr uint32_t kFftLdsBytes = 2u * ffr::kBuf * (uint32_t)sizeof(ffr::c2);      // the most a launch asks for

template <uint32_t M>
__device__ __forceinline__ void fft_frame(const FftFrame& f, ffr::c2* a, ffr::c2* b) {
    const uint32_t tid = threadIdx.x;
    const ffr::c2* W = reinterpret_cast<const ffr::c2*>(f.twiddles);
    ffr::load_frame<M>(f.ring, f.read, f.window, a, tid, f.mask);
    __syncthreads();
#pragma unroll
    for (uint32_t p = 0; p < ffr::num_passes<M>(); ++p) {
        ffr::run_pass<M>(p, a, b, tid, W);
        __syncthreads();
    }
    ffr::store_bins<M>(ffr::result<M>(a, b), tid, W, f.out, f.out + (M + 1u));
}

__global__ __launch_bounds__(ffr::kThreads) void elemhip_fft_frames(const FftFrame* frames, uint32_t bufStride) {
    extern __shared__ __align__(16) unsigned char fftLds[];
    ffr::c2* a = reinterpret_cast<ffr::c2*>(fftLds);
    ffr::c2* b = a + bufStride;                // (>= buf_stride(f.size) for every frame of the launch)
    const FftFrame f = frames[blockIdx.x];
    if (ffr::buf_stride(f.size) > bufStride) return;      // (never: the launcher sizes the buffers by the largest frame it was told of)
    switch (f.size) {                       // (uniform over the workgroup; any other size: the host never queues it, nothing is written)
        case 256u:  fft_frame<128u>(f, a, b); break;
        case 512u:  fft_frame<256u>(f, a, b); break;
        case 1024u: fft_frame<512u>(f, a, b); break;
        case 2048u: fft_frame<1024u>(f, a, b); break;
        case 4096u: fft_frame<2048u>(f, a, b); break;
        default: break;
    }
}

} // namespace

hipError_t launch_fft_frames(hipStream_t s, const FftFrame* framesDev, uint32_t count, uint32_t maxSize) {
    static const hipError_t configured = hipFuncSetAttribute(reinterpret_cast<const void*>(elemhip_fft_frames),
                                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFftLdsBytes);
    if (configured != hipSuccess) return configured;
    if (!count) return hipSuccess;
    if (!ffr::size_ok(maxSize)) return hipErrorInvalidValue;
    const uint32_t stride = ffr::buf_stride(maxSize), ldsBytes = 2u * stride * (uint32_t)sizeof(ffr::c2);
    hipLaunchKernelGGL(elemhip_fft_frames, dim3(count), dim3(ffr::kThreads), ldsBytes, s, framesDev, stride);
    return hipGetLastError();
}

} // namespace elemhip
