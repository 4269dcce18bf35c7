// spectrum.hip — the spectrum analyser's kernels (elemhip_spectrum_set; the arithmetic: spectrum.h), behind a launch set's last level
// next to the meter, on the render's stream: they read the delivered block where it lies in HBM, still warm in L2.
//   elemhip_spectrum_frames  one workgroup of 128 threads per (frame, channel). It gathers the frame's `size` samples — from the carried
//                            tail for programme frames in front of the set, from the set's block rows for the rest, zero outside the
//                            programme — times the window in double, runs the real FFT in LDS (fft_frames.h: packed complex transform +
//                            split step), leaves |X|^2 as doubles in the LDS buffer the transform did not end in and stores the frame's
//                            columns as float32: the powers, or the band sums, one lane per band in ascending bin order.
//   elemhip_spectrum_carry   behind it: one lane per (channel, column) adds the set's frames to the float64 running sums in frame order,
//                            and one lane per (channel, tail entry) writes the OTHER copy of the carried frames — a set may add fewer
//                            frames than the tail holds (block 64, 8 blocks a set, size 4096: a frame spans nine sets), so the tail
//                            is shifted from one copy into the other, never in place.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "launch.h"
#include "spectrum.h"

namespace elemhip {

namespace {

constexpr uint32_t kSpectrumLdsBytes = 2u * ffr::kBuf * (uint32_t)sizeof(ffr::c2);      // the most a launch asks for
constexpr uint32_t kCarryThreads = 256;
std::atomic<uint64_t> gLaunches{0};

// frame q of the set, as the levels (or the converter, or the limiter) left it: [block][numChannels][blockSize]
__device__ __forceinline__ float set_sample(const SpectrumArgs& A, uint32_t c, uint32_t q) {
    const uint32_t blk = q / A.blockSize, f = q - blk * A.blockSize;
    return A.src[((size_t)blk * A.numChannels + c) * A.blockSize + f];
}

template <uint32_t M>
__device__ __forceinline__ void spectrum_frame(const SpectrumArgs& A, ffr::c2* a, ffr::c2* b) {
    const uint32_t tid = threadIdx.x, jl = blockIdx.x, c = blockIdx.y, T = A.plan.size - 1u;
    const ffr::c2* W = reinterpret_cast<const ffr::c2*>(A.plan.twiddles);
    const float* tail = A.tailIn + (size_t)c * T;
    // the frame's first sample, counted from the set's first frame: >= -T for every frame that was not complete before the set
    const int64_t base = (int64_t)((A.j0 + jl) * A.plan.hop) - (int64_t)A.plan.pad - (int64_t)A.n0;
    auto fetch = [&](uint32_t i) -> float {
        const int64_t q = base + (int64_t)i;
        if (q < 0) { const int64_t t = q + (int64_t)T; return t >= 0 ? tail[t] : 0.0f; }
        return q < (int64_t)A.validFrames ? set_sample(A, c, (uint32_t)q) : 0.0f;
    };
    spectrum::load_frame<M>(fetch, A.plan.window, a, tid);
    __syncthreads();
#pragma unroll
    for (uint32_t p = 0; p < ffr::num_passes<M>(); ++p) {
        ffr::run_pass<M>(p, a, b, tid, W);
        __syncthreads();
    }
    double* pw = spectrum::power_buffer<M>(a, b);
    spectrum::split_power<M>(ffr::result<M>(a, b), tid, W, pw);
    __syncthreads();
    spectrum::store_columns(A.plan, pw, tid, A.out + ((size_t)c * A.numFrames + jl) * A.plan.cols);
}

__global__ __launch_bounds__(ffr::kThreads) void elemhip_spectrum_frames(const SpectrumArgs A, uint32_t bufStride) {
    extern __shared__ __align__(16) unsigned char spectrumLds[];
    ffr::c2* a = reinterpret_cast<ffr::c2*>(spectrumLds);
    ffr::c2* b = a + bufStride;
    if (blockIdx.x >= A.numFrames || blockIdx.y >= A.numChannels || ffr::buf_stride(A.plan.size) > bufStride) return;      // (never)
    switch (A.plan.size) {                  // (uniform over the launch)
        case 256u:  spectrum_frame<128u>(A, a, b); break;
        case 512u:  spectrum_frame<256u>(A, a, b); break;
        case 1024u: spectrum_frame<512u>(A, a, b); break;
        case 2048u: spectrum_frame<1024u>(A, a, b); break;
        case 4096u: spectrum_frame<2048u>(A, a, b); break;
        default: break;
    }
}

__global__ __launch_bounds__(kCarryThreads) void elemhip_spectrum_carry(const SpectrumArgs A) {
    const uint64_t g = (uint64_t)blockIdx.x * kCarryThreads + threadIdx.x;
    const uint32_t cols = A.plan.cols, T = A.plan.size - 1u;
    if (A.numFrames && g < (uint64_t)A.numChannels * cols) {
        const uint32_t c = (uint32_t)(g / cols), k = (uint32_t)(g - (uint64_t)c * cols);
        const float* col = A.out + (size_t)c * A.numFrames * cols + k;
        double acc = A.sums[g];
        for (uint32_t j = 0; j < A.numFrames; ++j) acc += (double)col[(size_t)j * cols];
        A.sums[g] = acc;
    }
    if (A.updateTail && g < (uint64_t)A.numChannels * T) {
        const uint32_t c = (uint32_t)(g / T), i = (uint32_t)(g - (uint64_t)c * T);
        A.tailOut[g] = spectrum::tail_next(A.tailIn + (size_t)c * T, T, A.validFrames, i, [&](uint32_t q) { return set_sample(A, c, q); });
    }
}

} // namespace

hipError_t launch_spectrum(hipStream_t s, const SpectrumArgs& a) {
    static const hipError_t configured = hipFuncSetAttribute(reinterpret_cast<const void*>(elemhip_spectrum_frames),
                                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSpectrumLdsBytes);
    if (configured != hipSuccess) return configured;
    if (!ffr::size_ok(a.plan.size) || a.numChannels == 0u || a.numChannels > 65535u) return hipErrorInvalidValue;
    if (a.updateTail && a.validFrames == 0u) return hipErrorInvalidValue;
    if (a.numFrames) {
        const uint32_t stride = ffr::buf_stride(a.plan.size), ldsBytes = 2u * stride * (uint32_t)sizeof(ffr::c2);
        hipLaunchKernelGGL(elemhip_spectrum_frames, dim3(a.numFrames, a.numChannels), dim3(ffr::kThreads), ldsBytes, s, a, stride);
        gLaunches.fetch_add(1u, std::memory_order_relaxed);
    }
    const uint64_t lanes = (uint64_t)a.numChannels * std::max(a.numFrames ? a.plan.cols : 0u, a.updateTail ? a.plan.size - 1u : 0u);
    if (lanes) {
        hipLaunchKernelGGL(elemhip_spectrum_carry, dim3((uint32_t)((lanes + kCarryThreads - 1u) / kCarryThreads)), dim3(kCarryThreads), 0, s, a);
        gLaunches.fetch_add(1u, std::memory_order_relaxed);
    }
    return hipGetLastError();
}

uint64_t spectrum_launches() { return gLaunches.load(std::memory_order_relaxed); }

} // namespace elemhip
