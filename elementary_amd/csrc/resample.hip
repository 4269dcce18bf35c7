// resample.hip — the delivery-rate converter of an offline render (Engine option "resample_rate"): behind a launch set's last level
// one kernel reads the set's output where it lies in HBM, float32 [block][channel][blockSize] at the engine's rate, and writes the
// frames of the delivery rate into a second buffer of the same layout, which the pack kernel, the meter and the float copy then take
// in its place. The plan, the tables, the tap sum and the tile's index functions all come from resample.h, which
// tests/native/resample_host.cpp runs on the CPU lane by lane.
//   resample  workgroup <-> tile of 256 outputs x 4 channels (x 1 where four rows would not fit 64 KB of LDS): the tile's input
//             stretch, reaching into the carried frames where it starts in front of the set, is staged once in padded LDS rows; lane
//             <-> output frame: one coefficient load (rows in output order, consecutive lanes consecutive floats) serves the four
//             channels' fused multiply-adds. Frames behind the set's last output up to the block's end are written as zeros.
//   history   thread <-> carried frame: the H frames behind this set, from the set and the old copy into the OTHER copy — the
//             resample kernel of the same launch only ever reads the old one. The host flips the copies.
// Plain vector stores, no atomics.
#include <hip/hip_runtime.h>

#include "resample.h"
#include "launch.h"

namespace elemhip {

namespace {

namespace rs = resample;

template <int C>
__global__ __launch_bounds__(rs::kTile) void elemhip_resample(ResampleArgs a) {
    extern __shared__ float rows[];
    const rs::Plan& p = a.plan;
    const uint32_t lane = threadIdx.x, fFirst = blockIdx.x * rs::kTile, c0 = blockIdx.y * C, rowFloats = rs::row_floats(p);
    const uint32_t f = fFirst + lane, bs = a.blockSize, nCh = a.numChannels;
    rs::Tile t{0, 0u};
    if (fFirst < a.validOut) {
        t = rs::tile_of(p, a.rowBase, a.n0, fFirst, a.validOut);
        const int64_t rel0 = t.jlo - (int64_t)a.t0;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const uint32_t c = c0 + ch;
            const float* hist = a.histIn + (size_t)(c < nCh ? c : 0u) * p.H;
            for (uint32_t i = lane; i < t.span; i += rs::kTile)
                rows[ch * rowFloats + rs::skew(i)] = c < nCh ? rs::input_at(a.src, bs, nCh, c, a.validIn, hist, p.H, rel0 + (int64_t)i) : 0.0f;
        }
    }
    __syncthreads();
    if ((uint64_t)f >= (uint64_t)a.outBlocks * bs) return;
    float acc[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) acc[ch] = 0.0f;
    if (f < a.validOut) {
        const uint64_t n = a.n0 + f;
        const uint32_t base = rs::lane_base(p, a.rowBase, t, n);
        rs::tap_sum<C>(a.table + (uint32_t)(n % p.L), p.L, p.T, [&](int ch, uint32_t k) { return rows[ch * rowFloats + rs::skew(base + k)]; }, acc);
    }
    float* out = a.dst + ((size_t)(f / bs) * nCh + c0) * bs + f % bs;
#pragma unroll
    for (int ch = 0; ch < C; ++ch)
        if (c0 + ch < nCh) out[(size_t)ch * bs] = acc[ch];
}

__global__ __launch_bounds__(256) void elemhip_resample_history(ResampleArgs a) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x, c = blockIdx.y, H = a.plan.H;
    if (j >= H) return;
    a.histOut[(size_t)c * H + j] = rs::history_next(a.src, a.blockSize, a.numChannels, c, a.histIn + (size_t)c * H, a.validIn, H, j);
}

} // namespace

hipError_t launch_resample(hipStream_t s, const ResampleArgs& a) {
    const rs::Plan& p = a.plan;
    if (a.blockSize == 0u || a.numChannels == 0u || p.L == 0u || p.M == 0u || p.L > rs::kMaxL || p.T == 0u || p.T > rs::kMaxT) return hipErrorInvalidValue;
    if (a.validIn == 0u) return a.validOut == 0u ? hipSuccess : hipErrorInvalidValue;
    // the set's outputs are the programme's [n0, n0 + validOut) and nothing else: every index the kernel forms follows from that
    if (a.n0 != rs::outputs_before(p, a.t0) || a.n0 + a.validOut != rs::outputs_before(p, a.t0 + a.validIn)) return hipErrorInvalidValue;
    if ((uint64_t)a.outBlocks * a.blockSize < a.validOut || a.outBlocks > a.outBlocksCap) return hipErrorInvalidValue;
    if ((uint64_t)a.outBlocks * a.blockSize > 0xFFFFFFFFull - rs::kTile) return hipErrorInvalidValue;      // (a lane's frame number is 32 bits)
    if (a.outBlocks) {
        const uint32_t tiles = (uint32_t)rs::ceil_div((uint64_t)a.outBlocks * a.blockSize, rs::kTile);
        const uint32_t rowBytes = rs::row_floats(p) * (uint32_t)sizeof(float);
        if (rs::kGroup * rowBytes <= 65536u)
            hipLaunchKernelGGL(elemhip_resample<(int)rs::kGroup>, dim3(tiles, (a.numChannels + rs::kGroup - 1u) / rs::kGroup), dim3(rs::kTile), rs::kGroup * rowBytes, s, a);
        else if (rowBytes <= 65536u)
            hipLaunchKernelGGL(elemhip_resample<1>, dim3(tiles, a.numChannels), dim3(rs::kTile), rowBytes, s, a);
        else return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(elemhip_resample_history, dim3((p.H + 255u) / 256u, a.numChannels), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace elemhip
