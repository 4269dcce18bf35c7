// automation.hip — the input stage of an offline render with breakpoint lanes (Engine::automationSet): the lane channels of a launch
// set's input, float32 rows of [block][channel][blockSize], are written from the device-resident breakpoint tables where the H2D copy
// of dense control signals would have put them. One workgroup per (block, channel in [firstChannel, numChannels)); a thread per span
// of automation::kSpan frames (automation.h: the value rule, the search and the walk all come from that header, which the engine's host
// path runs as the scalar twin). A channel without a lane and every frame behind validFrames is written as zero, so nothing of an
// earlier set is left in the rows. Nothing is read but the tables, nothing is carried.
#include <hip/hip_runtime.h>

#include <atomic>

#include "automation.h"
#include "launch.h"

namespace elemhip {

namespace {

namespace au = automation;

std::atomic<uint64_t> gLaunches{0};

template <bool QUADS>
__global__ __launch_bounds__(au::kThreads) void elemhip_automation(AutomationArgs a) {
    const uint32_t b = blockIdx.x, c = a.firstChannel + blockIdx.y, bs = a.blockSize;
    float* row = a.dst + ((size_t)b * a.numChannels + c) * bs;
    const uint32_t count = a.count[c];
    const au::Point* p = a.points + a.offset[c];
    // frames of this row that lie inside the call (uniform): the others are zero, as the inputs behind a call's last frame are
    const uint64_t rowFirst = (uint64_t)b * bs;
    const uint32_t live = count == 0u || rowFirst >= a.validFrames ? 0u : (uint32_t)(a.validFrames - rowFirst < bs ? a.validFrames - rowFirst : bs);
    const int64_t t0 = a.time0 + (int64_t)rowFirst;
    constexpr uint32_t W = QUADS ? au::kSpan : 1u;
    for (uint32_t f = threadIdx.x * W; f < bs; f += au::kThreads * W) {
        float v[W];
#pragma unroll
        for (uint32_t e = 0; e < W; ++e) v[e] = 0.0f;
        if (f < live) {
            au::Cursor cur(p, count, t0 + (int64_t)f);
#pragma unroll
            for (uint32_t e = 0; e < W; ++e)
                if (f + e < live) v[e] = cur.at(t0 + (int64_t)(f + e));
        }
        if (QUADS) *reinterpret_cast<float4*>(row + f) = make_float4(v[0], v[W > 1 ? 1 : 0], v[W > 2 ? 2 : 0], v[W > 3 ? 3 : 0]);
        else row[f] = v[0];
    }
}

} // namespace

hipError_t launch_automation(hipStream_t s, const AutomationArgs& a) {
    if (a.blockSize == 0u || a.numChannels > au::kMaxChannels || a.firstChannel > a.numChannels || !a.dst) return hipErrorInvalidValue;
    if (a.numBlocks == 0u || a.firstChannel == a.numChannels) return hipSuccess;
    // every row written lies inside [numBlocks][numChannels][blockSize]; every table a row reads lies inside the points
    if ((uint64_t)a.validFrames > (uint64_t)a.numBlocks * a.blockSize) return hipErrorInvalidValue;
    for (uint32_t c = a.firstChannel; c < a.numChannels; ++c)
        if (a.count[c] && (!a.points || (uint64_t)a.offset[c] + a.count[c] > a.numPoints)) return hipErrorInvalidValue;
    const dim3 grid(a.numBlocks, a.numChannels - a.firstChannel);
    // 16-byte stores where every row starts on a 16-byte boundary and holds whole quads
    const bool quads = a.blockSize % au::kSpan == 0u && (reinterpret_cast<uintptr_t>(a.dst) & 15u) == 0u;
    if (quads) hipLaunchKernelGGL(elemhip_automation<true>, grid, dim3(au::kThreads), 0, s, a);
    else hipLaunchKernelGGL(elemhip_automation<false>, grid, dim3(au::kThreads), 0, s, a);
    gLaunches.fetch_add(1, std::memory_order_relaxed);
    return hipGetLastError();
}

uint64_t automation_launches() { return gLaunches.load(std::memory_order_relaxed); }

} // namespace elemhip
