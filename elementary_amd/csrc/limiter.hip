// limiter.hip — the true-peak limiter of an offline render (Engine option "limiter"): behind a launch set's last level and the
// delivery-rate converter, five kernels read the set's output where it lies in HBM, float32 [block][channel][blockSize], and write the
// limited frames into a second buffer of the same layout, which the pack kernel, the meter and the float copy then take in its place.
// The arithmetic, the carried state's layout and every lane's share of a tile come from limiter.h, which tests/native/limiter_host.cpp
// runs on the CPU workgroup by workgroup and lane by lane.
//   detect    workgroup <-> tile of 256 frames of one channel group: the reductions the true peaks ask for, held over D + 7 frames by
//             doubling in LDS; writes dm and the tile's maximum of dm + n s
//   scan      wave <-> group: exclusive prefix maximum over the tiles, seeded with the carried M; leaves M for the next set
//   release   workgroup <-> tile: in-tile prefix maximum, d in place of dm; the largest d, one integer atomicMax per wave
//   apply     workgroup <-> tile: the D + 1 sum from LDS, the delayed samples times the gain; counts the limited frames; frames
//             behind the set's last up to the block's end are written as zeros
//   history   thread <-> carried value, from the set and the old copy into the OTHER copy — the kernels above only ever read the old one
// No floating-point atomics: a maximum does not depend on the order, the sum runs k ascending in one lane.
#include <hip/hip_runtime.h>

#include "limiter.h"
#include "launch.h"

namespace elemhip {

namespace {

namespace lm = limiter;

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (uint32_t o = 32u; o > 0u; o >>= 1) v = lm::dmax(v, __shfl_xor(v, (int)o));
    return v;
}

__global__ __launch_bounds__(lm::kTile) void elemhip_limiter_detect(LimiterArgs a) {
    extern __shared__ double lds[];
    const lm::Plan& p = a.plan;
    const uint32_t lane = threadIdx.x, tile = blockIdx.x, g = blockIdx.y, fFirst = tile * lm::kTile, E = lm::ext_frames(p);
    const uint32_t nCh = a.numChannels, width = lm::group_width(p, nCh), groups = lm::group_count(p, nCh), H = lm::hist_frames(p);
    double* from = lds;
    double* to = lds + E;
    float* row = reinterpret_cast<float*>(lds + 2u * E);
    const float* hist = reinterpret_cast<const float*>(a.stateIn + lm::state_off_hist(p, groups));
    for (uint32_t k = 0; k < width; ++k) {
        const uint32_t c = g * width + k;
        if (k) __syncthreads();                                  // (every lane has read the row of the channel before)
        lm::tile_stage(p, a.src, a.blockSize, nCh, c, a.validFrames, hist + (size_t)c * H, fFirst, lane, row);
        __syncthreads();
        lm::tile_detect(a.meter, p, row, k == 0u, lane, from);
    }
    lm::tile_reduce(p, lane, from);
    __syncthreads();
    const uint32_t P = lm::hold_pow2(p);
    for (uint32_t w = 1u; w < P; w *= 2u) {
        lm::tile_double(p, from, to, w, lane);
        __syncthreads();
        double* t = from; from = to; to = t;
    }
    const double dm = lm::tile_hold(p, from, P, lane);
    const uint32_t f = fFirst + lane;
    double v = -INFINITY;
    if (f < a.validFrames) {
        a.frames[(size_t)g * a.frameCap + f] = dm;
        v = dm + lm::ramp(p, a.n0 + f);
    }
    v = wave_max(v);
    if ((lane & 63u) == 0u) to[lane >> 6] = v;                  // (`to` was last read before the loop's last barrier)
    __syncthreads();
    if (lane == 0u) a.tiles[(size_t)g * a.tileCap + tile] = lm::dmax(lm::dmax(to[0], to[1]), lm::dmax(to[2], to[3]));
}

__global__ __launch_bounds__(64) void elemhip_limiter_scan(LimiterArgs a) {
    const uint32_t lane = threadIdx.x, g = blockIdx.x, numTiles = lm::tile_count(a.validFrames);
    double carry = reinterpret_cast<const double*>(a.stateIn)[g];
    double* at = a.tiles + (size_t)g * a.tileCap;
    for (uint32_t t0 = 0; t0 < numTiles; t0 += 64u) {
        const uint32_t t = t0 + lane;
        double v = t < numTiles ? at[t] : -INFINITY;
#pragma unroll
        for (uint32_t o = 1u; o < 64u; o <<= 1) {
            const double up = __shfl_up(v, o);
            if (lane >= o) v = lm::dmax(v, up);
        }
        const double up = __shfl_up(v, 1u);
        const double before = lane == 0u ? carry : lm::dmax(carry, up);     // M in front of tile t
        carry = lm::dmax(carry, __shfl(v, 63));
        if (t < numTiles) at[t] = before;
    }
    if (lane == 0u) reinterpret_cast<double*>(a.stateOut)[g] = carry;
}

__global__ __launch_bounds__(lm::kTile) void elemhip_limiter_release(LimiterArgs a) {
    __shared__ double sc[2][lm::kTile];
    const lm::Plan& p = a.plan;
    const uint32_t lane = threadIdx.x, tile = blockIdx.x, g = blockIdx.y, f = tile * lm::kTile + lane;
    const bool live = f < a.validFrames;
    double* slot = a.frames + (size_t)g * a.frameCap + f;
    const double dm = live ? *slot : 0.0, ns = lm::ramp(p, a.n0 + f);
    sc[0][lane] = live ? dm + ns : -INFINITY;
    __syncthreads();
    double* from = sc[0];
    double* to = sc[1];
    for (uint32_t w = 1u; w < lm::kTile; w *= 2u) {
        lm::scan_step(from, to, w, lane);
        __syncthreads();
        double* t = from; from = to; to = t;
    }
    double d = 0.0;
    if (live) {
        d = lm::release(dm, lm::dmax(a.tiles[(size_t)g * a.tileCap + tile], from[lane]), ns);
        *slot = d;
    }
    d = wave_max(d);
    if ((lane & 63u) == 0u && d > 0.0) atomicMax(&a.stats[g].maxBits, loudness::double_bits(d));
}

__global__ __launch_bounds__(lm::kTile) void elemhip_limiter_apply(LimiterArgs a) {
    extern __shared__ double lds[];
    const lm::Plan& p = a.plan;
    const uint32_t lane = threadIdx.x, g = blockIdx.y, fFirst = blockIdx.x * lm::kTile, f = fFirst + lane, bs = a.blockSize;
    const uint32_t nCh = a.numChannels, width = lm::group_width(p, nCh), groups = lm::group_count(p, nCh), H = lm::hist_frames(p);
    const double* dHist = reinterpret_cast<const double*>(a.stateIn + lm::state_off_d(p, groups)) + (size_t)g * p.D;
    const float* hist = reinterpret_cast<const float*>(a.stateIn + lm::state_off_hist(p, groups));
    lm::tile_window(p, a.frames + (size_t)g * a.frameCap, a.validFrames, dHist, fFirst, lane, lds);
    __syncthreads();
    const bool live = f < a.validFrames, inside = (uint64_t)f < (uint64_t)a.outBlocks * bs;
    const double gn = live ? lm::tile_gain(p, lds, lane) : 1.0;
    if (inside) {
        float* out = a.dst + ((size_t)(f / bs) * nCh + (size_t)g * width) * bs + f % bs;
        for (uint32_t k = 0; k < width; ++k) {
            const uint32_t c = g * width + k;
            out[(size_t)k * bs] = live ? lm::apply(p, gn, lm::input_at(a.src, bs, nCh, c, a.validFrames, hist + (size_t)c * H, H, (int64_t)f - (int64_t)lm::latency(p))) : 0.0f;
        }
    }
    const unsigned long long limited = __ballot(live && gn < 1.0);
    if ((lane & 63u) == 0u && limited) atomicAdd(&a.stats[g].limited, (unsigned long long)__popcll(limited));
}

__global__ __launch_bounds__(256) void elemhip_limiter_history(LimiterArgs a) {
    const lm::Plan& p = a.plan;
    const uint32_t j = blockIdx.x * 256u + threadIdx.x, nCh = a.numChannels, groups = lm::group_count(p, nCh), H = lm::hist_frames(p);
    if (blockIdx.y < nCh) {
        const uint32_t c = blockIdx.y;
        if (j >= H) return;
        const float* old = reinterpret_cast<const float*>(a.stateIn + lm::state_off_hist(p, groups)) + (size_t)c * H;
        reinterpret_cast<float*>(a.stateOut + lm::state_off_hist(p, groups))[(size_t)c * H + j] = lm::history_next(a.src, a.blockSize, nCh, c, old, a.validFrames, H, j);
    } else {
        const uint32_t g = blockIdx.y - nCh;
        if (j >= p.D) return;
        const double* old = reinterpret_cast<const double*>(a.stateIn + lm::state_off_d(p, groups)) + (size_t)g * p.D;
        reinterpret_cast<double*>(a.stateOut + lm::state_off_d(p, groups))[(size_t)g * p.D + j] = lm::d_history_next(a.frames + (size_t)g * a.frameCap, old, a.validFrames, p.D, j);
    }
}

} // namespace

hipError_t launch_limiter(hipStream_t s, const LimiterArgs& a) {
    const lm::Plan& p = a.plan;
    if (a.blockSize == 0u || p.D < 1u || p.D > lm::kMaxD || !lm::channels_ok(p, a.numChannels) || a.numChannels > 32768u) return hipErrorInvalidValue;
    if (a.validFrames == 0u) return hipErrorInvalidValue;          // (nothing to carry forward either: the caller skips an empty set)
    // every index the kernels form follows from these: frames < frameCap, tiles < tileCap, stores inside outBlocks whole blocks
    const uint32_t numTiles = lm::tile_count(a.validFrames);
    if (a.validFrames > a.frameCap || numTiles > a.tileCap) return hipErrorInvalidValue;
    if ((uint64_t)a.outBlocks * a.blockSize < a.validFrames || a.outBlocks > a.outBlocksCap) return hipErrorInvalidValue;
    if ((uint64_t)a.outBlocks * a.blockSize > 0xFFFFFFFFull - lm::kTile) return hipErrorInvalidValue;      // (a lane's frame number is 32 bits)
    const uint32_t groups = lm::group_count(p, a.numChannels), E = lm::ext_frames(p);
    const uint32_t outTiles = (uint32_t)(((uint64_t)a.outBlocks * a.blockSize + lm::kTile - 1u) / lm::kTile);
    const uint32_t detectLds = 2u * E * (uint32_t)sizeof(double) + lm::row_frames(p) * (uint32_t)sizeof(float);
    hipLaunchKernelGGL(elemhip_limiter_detect, dim3(numTiles, groups), dim3(lm::kTile), detectLds, s, a);
    hipLaunchKernelGGL(elemhip_limiter_scan, dim3(groups), dim3(64), 0, s, a);
    hipLaunchKernelGGL(elemhip_limiter_release, dim3(numTiles, groups), dim3(lm::kTile), 0, s, a);
    hipLaunchKernelGGL(elemhip_limiter_apply, dim3(outTiles, groups), dim3(lm::kTile), (lm::kTile + p.D) * (uint32_t)sizeof(double), s, a);
    hipLaunchKernelGGL(elemhip_limiter_history, dim3((lm::hist_frames(p) + 255u) / 256u, a.numChannels + groups), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace elemhip
