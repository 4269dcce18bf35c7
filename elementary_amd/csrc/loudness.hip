// loudness.hip — the loudness meter of an offline render (Engine option "loudness_meter"): behind a launch set's last level, five
// small kernels read the set's output where it lies in HBM, float32 [block][channel][blockSize], and leave the K-weighted sums of the
// sub-blocks the set completed, the running peaks and the carried state (loudness.h: the arithmetic, the segment schedule and the
// carried state all come from that header, which tests/native/loudness_host.cpp runs on the CPU):
//   peaks     thread <-> frame: the three interpolated points and the sample itself, one integer atomicMax per wave and channel
//   pass one  thread <-> segment of L frames from zero state
//   scan      one wave per channel: the segments' true start states, 64 per step; the carried frames for the next set's interpolator
//   pass two  thread <-> segment from its true start state: squared output into the two sub-blocks it may straddle
//   combine   thread <-> sub-block: carried partial sum + the segments' sums in segment order
// No floating-point atomics anywhere: sums are combined in a fixed order, a maximum does not depend on the order.
#include <hip/hip_runtime.h>

#include "loudness.h"
#include "launch.h"

namespace elemhip {

namespace {

namespace ld = loudness;

__global__ __launch_bounds__(ld::kThreads) void elemhip_loudness_peaks(LoudnessArgs a) {
    const uint32_t f = blockIdx.x * ld::kThreads + threadIdx.x, c = blockIdx.y;
    ld::ChannelState* st = a.state + c;
    double best = 0.0;
    uint32_t sample = 0u;
    if (f < a.validFrames) {
        double w[ld::kPhaseTaps];
#pragma unroll
        for (uint32_t m = 0; m < ld::kPhaseTaps; ++m) w[m] = ld::window_frame(a.src, a.blockSize, a.numChannels, c, st->hist, f, m);
        best = ld::peak_at(a.plan, w);
        sample = __float_as_uint((float)w[0]) & 0x7FFFFFFFu;
    }
#pragma unroll
    for (uint32_t o = 32u; o > 0u; o >>= 1) {
        best = fmax(best, __shfl_xor(best, (int)o));
        sample = max(sample, (uint32_t)__shfl_xor((int)sample, (int)o));
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (best > 0.0) atomicMax(&st->truePeakBits, ld::double_bits(best));
        if (sample) atomicMax(&st->samplePeakBits, sample);
    }
}

__global__ __launch_bounds__(ld::kThreads) void elemhip_loudness_pass_one(LoudnessArgs a) {
    const uint32_t k = blockIdx.x * ld::kThreads + threadIdx.x, c = blockIdx.y;
    if (k + 1u >= a.numSegs) return;                           // (the last segment's end state is pass two's to leave)
    double z[4];
    ld::pass_one(a.plan, ld::cursor_at(a.src, a.blockSize, a.numChannels, c, k * a.plan.L), a.plan.L, z);
    double* out = a.segState + ((size_t)c * a.segCap + k) * 4u;
    out[0] = z[0]; out[1] = z[1]; out[2] = z[2]; out[3] = z[3];
}

__global__ __launch_bounds__(64) void elemhip_loudness_scan(LoudnessArgs a) {
    const uint32_t lane = threadIdx.x, c = blockIdx.x;
    ld::ChannelState* st = a.state + c;
    double seed[4] = {st->s[0], st->s[1], st->s[2], st->s[3]};
    for (uint32_t k0 = 0; k0 < a.numSegs; k0 += 64u) {
        const uint32_t k = k0 + lane;
        double* at = a.segState + ((size_t)c * a.segCap + k) * 4u;
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        if (k + 1u < a.numSegs) { v[0] = at[0]; v[1] = at[1]; v[2] = at[2]; v[3] = at[3]; }
        if (lane == 0u) ld::scan_fold(a.plan.power[0], v, seed);
#pragma clang loop unroll(disable)
        for (uint32_t i = 0; i < ld::kScanSteps; ++i) {       // (rolled: one step's matrix in scalar registers at a time)
            double o[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = __shfl_up(v[r], 1u << i);
            if (lane >= (1u << i)) ld::scan_fold(a.plan.power[i], v, o);
        }
        // v = the state behind segment k: segment k + 1 starts there, the group's first segment at the seed
        double start[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double up = __shfl_up(v[r], 1u);
            start[r] = lane == 0u ? seed[r] : up;
            seed[r] = __shfl(v[r], 63);
        }
        if (k < a.numSegs) { at[0] = start[0]; at[1] = start[1]; at[2] = start[2]; at[3] = start[3]; }
    }
    // the frames the next set's interpolator finds in front of it (the peaks kernel, earlier on the stream, has read the old ones)
    float next = 0.0f;
    if (lane < ld::kHistory) next = ld::history_next(a.src, a.blockSize, a.numChannels, c, st->hist, a.validFrames, lane);
    __syncthreads();
    if (lane < ld::kHistory) st->hist[lane] = next;
}

__global__ __launch_bounds__(ld::kThreads) void elemhip_loudness_pass_two(LoudnessArgs a) {
    const uint32_t k = blockIdx.x * ld::kThreads + threadIdx.x, c = blockIdx.y;
    if (k >= a.numSegs) return;
    const double* at = a.segState + ((size_t)c * a.segCap + k) * 4u;
    double s[4] = {at[0], at[1], at[2], at[3]}, e[2];
    ld::pass_two(a.plan, ld::cursor_at(a.src, a.blockSize, a.numChannels, c, k * a.plan.L), ld::segment_frames(k, a.validFrames, a.plan.L),
                 ld::segment_first(k, a.q0, a.plan.hop, a.plan.L), s, e);
    double* out = a.segEnergy + ((size_t)c * a.segCap + k) * 2u;
    out[0] = e[0]; out[1] = e[1];
    if (k + 1u == a.numSegs) { ld::ChannelState* st = a.state + c; st->s[0] = s[0]; st->s[1] = s[1]; st->s[2] = s[2]; st->s[3] = s[3]; }
}

__global__ __launch_bounds__(64) void elemhip_loudness_combine(LoudnessArgs a) {
    const uint32_t c = blockIdx.x;
    ld::ChannelState* st = a.state + c;
    const double carried = st->partial;
    __syncthreads();                                            // (every thread holds the carried sum before one of them replaces it)
    const uint32_t hop = a.plan.hop, touched = ld::subblocks_touched(a.q0, a.validFrames, hop), complete = ld::subblocks_complete(a.q0, a.validFrames, hop);
    const double* e = a.segEnergy + (size_t)c * a.segCap * 2u;
    for (uint32_t j = threadIdx.x; j < touched; j += 64u) {
        const double sum = ld::subblock_sum(e, j, carried, a.q0, a.validFrames, hop, a.plan.L);
        if (j < complete) a.out[(size_t)c * a.outStride + j] = sum;
        else st->partial = sum;
    }
    if (touched == complete && threadIdx.x == 0u) st->partial = 0.0;
}

} // namespace

hipError_t launch_loudness(hipStream_t s, const LoudnessArgs& a) {
    const ld::Plan& p = a.plan;
    if (a.blockSize == 0u || a.numChannels == 0u || p.hop == 0u || p.L == 0u || p.L > p.hop || a.q0 >= p.hop) return hipErrorInvalidValue;
    if (a.validFrames == 0u) return hipSuccess;
    if (a.numSegs != ld::segment_count(a.validFrames, p.L) || a.numSegs > a.segCap) return hipErrorInvalidValue;
    if (ld::subblocks_complete(a.q0, a.validFrames, p.hop) > a.outStride) return hipErrorInvalidValue;
    const dim3 perFrame((a.validFrames + ld::kThreads - 1u) / ld::kThreads, a.numChannels);
    const dim3 perSeg((a.numSegs + ld::kThreads - 1u) / ld::kThreads, a.numChannels);
    hipLaunchKernelGGL(elemhip_loudness_peaks, perFrame, dim3(ld::kThreads), 0, s, a);
    hipLaunchKernelGGL(elemhip_loudness_pass_one, perSeg, dim3(ld::kThreads), 0, s, a);
    hipLaunchKernelGGL(elemhip_loudness_scan, dim3(a.numChannels), dim3(64), 0, s, a);
    hipLaunchKernelGGL(elemhip_loudness_pass_two, perSeg, dim3(ld::kThreads), 0, s, a);
    hipLaunchKernelGGL(elemhip_loudness_combine, dim3(a.numChannels), dim3(64), 0, s, a);
    return hipGetLastError();
}

} // namespace elemhip
