// qc.hip — the inspector's kernels (elemhip_qc_set; the definitions and the arithmetic: qc.h), behind a launch set's last level next to
// the meter and the analyser, on the render's stream: they read the delivered block where it lies in HBM, still warm in L2.
//   elemhip_qc_tiles   one workgroup of 128 threads per (tile, channel); a tile is 128 leaves of 64 PROGRAMME frames, so neither depends
//                      on how the render is cut. The tile's part of the set is staged into padded LDS rows with 16-byte loads along the
//                      block rows (a lane walking 64 frames in global memory would stride 256 bytes); lane l then walks leaf l in frame
//                      order: the leaf's float64 sums (begun from the carried partial where the leaf began before the set) and the
//                      exact summary of its stretch. The 128 summaries are combined in an in-order tree in LDS; the overview's pieces
//                      are folded from the leaves' minima and maxima and the odd frames around them.
//   elemhip_qc_pairs   the same staging for the two channels of a pair, 64 leaves per workgroup: the leaf sums of x_a x_b.
//   elemhip_qc_fold    behind them, per channel: one wave adds the leaf sums of x to the total in leaf order, one those of x^2 (64
//                      leaves per coalesced load, handed round the wave), one lane folds the tiles' summaries into the programme's
//                      and merges the overview's pieces; per pair one wave. No atomics: the same bits every run.
#include <hip/hip_runtime.h>

#include <atomic>

#include "launch.h"
#include "qc.h"

namespace elemhip {

namespace {

std::atomic<uint64_t> gLaunches{0};

struct Range { uint64_t base, lo, hi; };      // a tile's first programme frame; the part of it this set holds
__device__ __forceinline__ Range tile_range(const QcArgs& A, uint32_t t, uint32_t frames) {
    Range r;
    r.base = (A.p0 / frames + t) * frames;
    r.lo = r.base > A.p0 ? r.base : A.p0;
    const uint64_t end = A.p0 + A.count;
    r.hi = r.base + frames < end ? r.base + frames : end;
    if (r.hi < r.lo) r.hi = r.lo;
    return r;
}

// programme frames [r.lo, r.hi) of channel c into rows of kRowStride floats, row = (frame - r.base) / kLeaf: 16-byte loads along the
// set's [block][channel][blockSize] rows, aligned in the SOURCE (where blockSize is a multiple of 4; else frame by frame); the frames
// of a group outside the range are dropped
__device__ __forceinline__ void stage(const QcArgs& A, uint32_t c, const Range& r, float* rows) {
    if (r.hi <= r.lo) return;
    const uint32_t qa = A.q0 + (uint32_t)(r.lo - A.p0), qb = A.q0 + (uint32_t)(r.hi - A.p0);
    const uint32_t shift = (uint32_t)(r.lo - r.base);      // frame qa lands at shift
    if (A.blockSize & 3u) {                 // rows that are not 16-byte aligned: frame by frame
        for (uint32_t q = qa + threadIdx.x; q < qb; q += qc::kThreads) {
            const uint32_t blk = q / A.blockSize, f = q - blk * A.blockSize, j = q - qa + shift;
            rows[(j >> 6) * qc::kRowStride + (j & 63u)] = A.src[((size_t)blk * A.numChannels + c) * A.blockSize + f];
        }
        return;
    }
    for (uint32_t g = (qa >> 2) + threadIdx.x; g * 4u < qb; g += qc::kThreads) {
        const uint32_t q4 = g * 4u, blk = q4 / A.blockSize, f = q4 - blk * A.blockSize;
        const float4 v = *reinterpret_cast<const float4*>(A.src + ((size_t)blk * A.numChannels + c) * A.blockSize + f);
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t q = q4 + k;
            if (q >= qa && q < qb) { const uint32_t j = q - qa + shift; rows[(j >> 6) * qc::kRowStride + (j & 63u)] = e[k]; }
        }
    }
}

__global__ __launch_bounds__(qc::kThreads) void elemhip_qc_tiles(const QcArgs A) {
    __shared__ float rows[qc::kTileLeaves * qc::kRowStride];
    __shared__ qc::Stretch<uint32_t> red[qc::kTileLeaves];
    __shared__ float leafMn[qc::kTileLeaves], leafMx[qc::kTileLeaves];
    const uint32_t t = blockIdx.x, c = blockIdx.y, l = threadIdx.x;
    if (t >= A.numTiles || c >= A.numChannels) return;      // (never)
    const Range r = tile_range(A, t, qc::kTileFrames);
    stage(A, c, r, rows);
    __syncthreads();
    // the walk: leaf l in frame order
    const uint64_t leafP = r.base + (uint64_t)l * qc::kLeaf;
    const uint64_t a = leafP > r.lo ? leafP : r.lo, b = leafP + qc::kLeaf < r.hi ? leafP + qc::kLeaf : r.hi;
    qc::Stretch<uint32_t> s = qc::stretch_empty<uint32_t>();
    if (a < b) {
        const bool carried = leafP < A.p0;          // the programme's open leaf goes on: its partial sums are the start
        double sum = carried ? A.state[c].sum.partial : 0.0, sq = carried ? A.state[c].sq.partial : 0.0;
        const float* row = rows + l * qc::kRowStride;
        for (uint64_t P = a; P < b; ++P) {
            const qc::Frame f = qc::classify(row[(uint32_t)(P - leafP)], A.spec);
            qc::stretch_push<uint32_t>(s, f, (uint32_t)(P - A.p0), A.spec);
            const double d = (double)f.x;
            sum += d; sq += d * d;
        }
        const uint32_t leaf = (uint32_t)(leafP / qc::kLeaf - A.p0 / qc::kLeaf);
        if (leaf < A.leafCap) {
            A.leafSums[((size_t)c * 2u) * A.leafCap + leaf] = sum;
            A.leafSums[((size_t)c * 2u + 1u) * A.leafCap + leaf] = sq;
        }
    }
    red[l] = s; leafMn[l] = s.mn; leafMx[l] = s.mx;
    // the in-order tree: lane l takes the stretch of lane l + step behind its own
    for (uint32_t step = 1; step < qc::kTileLeaves; step <<= 1) {
        __syncthreads();
        if ((l & (2u * step - 1u)) == 0u) {
            uint64_t start = r.base + (uint64_t)(l + step) * qc::kLeaf;
            start = start < r.lo ? r.lo : start > r.hi ? r.hi : start;
            red[l] = qc::stretch_combine<uint32_t>(red[l], red[l + step], (uint32_t)(start - A.p0), A.spec);
        }
    }
    __syncthreads();
    if (l == 0u && t < A.tileCap) A.tileStretch[(size_t)c * A.tileCap + t] = red[0];
    // the overview: this tile's pieces, a bucket's part inside [lo, hi); whole buckets leave at once, the others wait for the fold
    const uint32_t B = A.spec.bucket;
    if (B == 0u || r.hi <= r.lo) return;
    const uint64_t gF = r.lo / B, gL = (r.hi - 1u) / B, g0 = A.p0 / B;
    for (uint64_t g = gF + l; g <= gL; g += qc::kThreads) {
        const uint64_t pa = g * B > r.lo ? g * B : r.lo, pb = (g + 1u) * B < r.hi ? (g + 1u) * B : r.hi;
        float mn = INFINITY, mx = -INFINITY;
        for (uint64_t P = pa; P < pb;) {
            const uint32_t j = (uint32_t)(P - r.base);
            if ((j & 63u) == 0u && P + qc::kLeaf <= pb) { qc::minmax_fold(mn, mx, leafMn[j >> 6], leafMx[j >> 6]); P += qc::kLeaf; }
            else { const float x = qc::classify(rows[(j >> 6) * qc::kRowStride + (j & 63u)], A.spec).x; qc::minmax_fold(mn, mx, x, x); P += 1u; }
        }
        if (pb - pa == B) {
            if (g - g0 < A.outCount) { float* o = A.out + ((size_t)c * A.outCount + (size_t)(g - g0)) * 2u; o[0] = mn; o[1] = mx; }
        } else if (t < A.tileCap) {
            float* e = A.tileEdge + ((size_t)c * A.tileCap + t) * 4u + (g == gF ? 0u : 2u);
            e[0] = mn; e[1] = mx;
        }
    }
}

__global__ __launch_bounds__(qc::kThreads) void elemhip_qc_pairs(const QcArgs A) {
    __shared__ float rowsA[qc::kPairLeaves * qc::kRowStride];
    __shared__ float rowsB[qc::kPairLeaves * qc::kRowStride];
    const uint32_t t = blockIdx.x, k = blockIdx.y, l = threadIdx.x;
    if (k >= A.numPairs) return;            // (never)
    const uint32_t ca = A.pairs[2u * k], cb = A.pairs[2u * k + 1u];
    const Range r = tile_range(A, t, qc::kPairLeaves * qc::kLeaf);
    if (ca >= A.numChannels || cb >= A.numChannels || r.hi <= r.lo) return;
    stage(A, ca, r, rowsA);
    stage(A, cb, r, rowsB);
    __syncthreads();
    if (l >= qc::kPairLeaves) return;
    const uint64_t leafP = r.base + (uint64_t)l * qc::kLeaf;
    const uint64_t a = leafP > r.lo ? leafP : r.lo, b = leafP + qc::kLeaf < r.hi ? leafP + qc::kLeaf : r.hi;
    if (a >= b) return;
    double acc = leafP < A.p0 ? A.pairState[k].partial : 0.0;
    const float* ra = rowsA + l * qc::kRowStride; const float* rb = rowsB + l * qc::kRowStride;
    for (uint64_t P = a; P < b; ++P) {
        const uint32_t j = (uint32_t)(P - leafP);
        acc += (double)qc::classify(ra[j], A.spec).x * (double)qc::classify(rb[j], A.spec).x;
    }
    const uint32_t leaf = (uint32_t)(leafP / qc::kLeaf - A.p0 / qc::kLeaf);
    if (leaf < A.leafCap) A.leafSums[((size_t)A.numChannels * 2u + k) * A.leafCap + leaf] = acc;
}

// the leaves of one row into its sums, in leaf order (qc::fold_leaf for every leaf, with its test hoisted: only the last leaf can be
// open): every lane of the wave keeps the same running sums; 64 leaves per load
__device__ __forceinline__ qc::Sums fold_row(qc::Sums s, const double* leaves, uint32_t n, uint64_t p0, uint32_t count, uint32_t lane) {
    if (n == 0u) return s;
    const uint32_t whole = (p0 / qc::kLeaf + n) * qc::kLeaf <= p0 + count ? n : n - 1u;      // the complete leaves
    double total = s.total;
    for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
        const double mine = i0 + lane < n ? leaves[i0 + lane] : 0.0;
        const uint32_t m = whole > i0 ? (whole - i0 < 64u ? whole - i0 : 64u) : 0u;
        for (uint32_t j = 0; j < m; ++j) total += __shfl(mine, (int)j, 64);
        if (whole < n && whole >= i0 && whole < i0 + 64u) s.partial = __shfl(mine, (int)(whole - i0), 64);
    }
    s.total = total;
    if (whole == n) s.partial = 0.0;
    return s;
}

constexpr uint32_t kFoldThreads = 192;
__global__ __launch_bounds__(kFoldThreads) void elemhip_qc_fold(const QcArgs A) {
    const uint32_t row = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t n = qc::leaf_count(A.p0, A.count);
    if (n > A.leafCap || A.numTiles > A.tileCap) return;      // (never: sized by the host for the largest set)
    if (row >= A.numChannels) {
        const uint32_t k = row - A.numChannels;
        if (k >= A.numPairs || wave != 0u) return;
        const qc::Sums s = fold_row(A.pairState[k], A.leafSums + ((size_t)A.numChannels * 2u + k) * A.leafCap, n, A.p0, A.count, lane);
        if (lane == 0u) A.pairState[k] = s;
        return;
    }
    const uint32_t c = row;
    qc::ChannelState* st = A.state + c;
    if (wave < 2u) {
        const qc::Sums s = fold_row(wave ? st->sq : st->sum, A.leafSums + ((size_t)c * 2u + wave) * A.leafCap, n, A.p0, A.count, lane);
        if (lane == 0u) { if (wave) st->sq = s; else st->sum = s; }
        return;
    }
    if (lane != 0u) return;
    // the tiles' summaries behind the programme's, in order; the overview's pieces into the open bucket
    qc::Stretch<uint64_t> S = st->s;
    qc::ChannelState ov = *st;
    const uint32_t B = A.spec.bucket;
    const uint64_t g0 = B ? A.p0 / B : 0u;
    float* out = A.out + (size_t)c * A.outCount * 2u;
    for (uint32_t t = 0; t < A.numTiles; ++t) {
        const Range r = tile_range(A, t, qc::kTileFrames);
        S = qc::stretch_combine<uint64_t>(S, qc::widen(A.tileStretch[(size_t)c * A.tileCap + t], A.p0), r.lo, A.spec);
        if (B == 0u || r.hi <= r.lo) continue;
        const float* e = A.tileEdge + ((size_t)c * A.tileCap + t) * 4u;
        const uint64_t gF = r.lo / B, gL = (r.hi - 1u) / B;
        if (qc::has_lead(r.lo, r.hi, B)) {
            const uint64_t pb = (gF + 1u) * B < r.hi ? (gF + 1u) * B : r.hi;
            if (gF - g0 < A.outCount || ov.bCount + (uint32_t)(pb - r.lo) < B) qc::bucket_merge(ov, e[0], e[1], (uint32_t)(pb - r.lo), B, gF, g0, out, 2u);
        }
        if (qc::has_trail(r.lo, r.hi, B)) qc::bucket_merge(ov, e[2], e[3], (uint32_t)(r.hi - gL * B), B, gL, g0, out, 2u);
    }
    st->s = S; st->bMin = ov.bMin; st->bMax = ov.bMax; st->bCount = ov.bCount;
}

} // namespace

hipError_t launch_qc(hipStream_t s, const QcArgs& a) {
    if (a.count == 0u) return hipSuccess;
    const uint32_t tiles = qc::tile_count(a.p0, a.count), leaves = qc::leaf_count(a.p0, a.count);
    if (a.numChannels == 0u || a.numChannels > 65535u || a.numPairs > qc::kMaxPairs || a.blockSize == 0u) return hipErrorInvalidValue;
    if (a.numTiles != tiles || tiles > a.tileCap || leaves > a.leafCap || a.outCount != qc::buckets_complete(a.p0, a.count, a.spec.bucket)) return hipErrorInvalidValue;
    if ((a.blockSize & 3u) == 0u && (reinterpret_cast<uintptr_t>(a.src) & 15u) != 0u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(elemhip_qc_tiles, dim3(tiles, a.numChannels), dim3(qc::kThreads), 0, s, a);
    gLaunches.fetch_add(1u, std::memory_order_relaxed);
    if (a.numPairs) {
        const uint32_t half = qc::kPairLeaves * qc::kLeaf;
        const uint32_t halves = (uint32_t)((a.p0 + a.count + half - 1u) / half - a.p0 / half);
        hipLaunchKernelGGL(elemhip_qc_pairs, dim3(halves, a.numPairs), dim3(qc::kThreads), 0, s, a);
        gLaunches.fetch_add(1u, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(elemhip_qc_fold, dim3(a.numChannels + a.numPairs), dim3(kFoldThreads), 0, s, a);
    gLaunches.fetch_add(1u, std::memory_order_relaxed);
    return hipGetLastError();
}

uint64_t qc_launches() { return gLaunches.load(std::memory_order_relaxed); }

} // namespace elemhip
