// conv_long.inc — `convolve` inside a launch set, LONG partitions (included by conv.hip; r05, VERDICT r04 "next" #3).
//
// The reference (wasm/Convolve.h:49 -> TwoStageFFTConvolver::init(512, 4096, ir, len)) cuts the impulse response into a head of
// 512-sample partitions and a tail of 4096-sample ones: the small partitions exist so that a block can be answered within a block,
// the large ones so that the bulk of the work costs an eighth of the multiply-adds per output sample. r02-r04 evaluated the whole
// IR with 512-sample partitions, 188 x 513 complex multiply-adds per channel and block: 6.3 GFLOP per 1024-block set of C3,
// half of the set's kernel time even on the matrix cores. In a launch set there is no latency to answer to — every input block
// of the set is known before the convolve level starts — so the head is not needed at all:
//
//     the WHOLE IR in 4096-sample partitions g_q (8192-point spectra G_q), the set's input in 4096-sample chunks (8 blocks each),
//     overlap-save:   U_c = RFFT_8192([chunk c-1 | chunk c]),   Y_C = sum_q G_q U_{C-q},   out chunk C = IRFFT_8192(Y_C)[4096:8192]
//
//   K1  long_fft   (node, chunk row): U_c for the set's chunks and for the Q-1 chunks in front of it — those come from a ring of the
//                  node's last input blocks in the time domain (conv state `hist`, written by every path that consumes input);
//   K2  long_mac   (node, 256 bins, run of 16 chunks): Y_C[k] = sum_q G_q[k] U_{C-q}[k], one thread per bin: the 16 accumulators and
//                  eight taps live in registers, every spectrum value loaded is used for up to eight multiply-adds (0.8 GFLOP per
//                  C3 set instead of 6.3: plain v_fma_f32 — the matrix-core Toeplitz kernel stays with the 512-partition path);
//   K3  long_ifft  (node, chunk): inverse transform, the second half -> the node's output buffers of the chunk's 8 blocks (folded
//                  root gain applied);
//   K4  long_state (node, block): what the block-at-a-time path and the next set need: the input ring, the 1024-point spectra of
//                  the last P blocks (the 512-partition state `X`), then long_tail (node): the overlap the last block leaves.
// Conditions (conv_use_long): whole sets of a multiple of 8 blocks, an IR of at least kLongMinP 512-partitions, every call so far
// whole 512-frame blocks (Engine::convAligned, as for the 512-partition set path). Anything else renders through the kernels
// above this file; both leave the same state, so calls of either kind interleave freely.
// Arithmetic: float FFTs (fft4096.h: Stockham radix-16 in LDS, tables rounded from double), IR spectra computed in double on the
// host; the result differs from the reference's (and from the 512-partition path's) by float rounding only — the bar is 1e-6 on
// |y| <~ 1 (SURVEY 8(d) C3 note), tests/test_gpu_convolve.py + the wasm recordings.
#include "fft4096.h"

namespace {

using lfft::kRow;
__device__ c2 kTw8192[lfft::N];        // exp(-2 pi i j / 8192), rounded from double on the host (upload_convolve_tables)

constexpr uint32_t kLongTaps = 8;       // taps per register group of the MAC (G rows are allocated in multiples of this, zero rows behind the IR)
constexpr uint32_t kLongRun = 16;       // chunks per thread of the MAC

struct LongState { gcf2p G; gfp hist; uint32_t Q, Qp, R; };
__device__ __forceinline__ LongState long_state_of(const State& st) {
    LongState ls;
    ls.Q = st.hdr[conv::H_Q]; ls.Qp = (ls.Q + kLongTaps - 1u) / kLongTaps * kLongTaps; ls.R = st.hdr[conv::H_HISTBLKS];
    ls.hist = st.overlap + 512u;
    ls.G = (gcf2p)(ls.hist + (size_t)ls.R * 512u);
    return ls;
}
// per-node scratch of the long path, behind the 512-partition path's: U rows [histRows + maxChunks][kRow], Y rows [maxChunks][kRow]
__host__ __device__ __forceinline__ size_t long_scratch_floats(uint32_t maxBatch, uint32_t histRows) {
    const size_t maxChunks = (maxBatch + 7u) / 8u;
    return ((size_t)histRows + 2u * maxChunks) * kRow * 2u;
}
// The U rows are a RING of Ru = histRows + maxChunks rows (r06): a set's chunks go where the previous set's left off, so the Q - 1
// spectra in front of a set are the previous set's last rows and are NOT transformed again (15 % of long_fft's workgroups at C3's
// geometry — and the difference between 1208 workgroups and 1024, i.e. between two rounds on the chip and one). Logical row l of a
// set (l = histRows + chunk, chunk in [-histRows, chunks)) lives at physical row (l0 + l) mod Ru.
// Scratch header words (uint32 view of the node's first kBatchHdr floats):
//   per SET, written by long_fft's chunk-0 workgroup, read by long_mac / long_ifft:  [0] the node's block counter at the start of the
//   set, [1] l0, [2] 1: the history rows were carried over (not transformed by this set);
//   PERSISTENT, written by long_ifft's last-chunk workgroup only, read by long_fft only:  [8] uid of the convolver state the ring
//   belongs to (conv::H_UID: a new IR is a new state), [9] the block counter the ring is current for, [10] physical row of the next
//   set's chunk 0, [11] Ru (a tag of the layout the row numbers were written for).
// Any path that moves the block counter without going through long_ifft (single blocks, 512-partition sets) leaves [9] behind: the
// next long set transforms its history from the time-domain ring `hist`, as every set did in r05.
enum : uint32_t { LH_BLK0 = 0, LH_L0 = 1, LH_CARRIED = 2, LH_UID = 8, LH_BLKEND = 9, LH_ROWNEXT = 10, LH_RU = 11 };
struct LongCtx { gf2p U, Y; uint32_t histRows, Ru; };
__device__ __forceinline__ LongCtx long_ctx(const BatchCtx& c, uint32_t maxBatch, uint32_t histRows) {
    LongCtx l;
    l.histRows = histRows;
    l.Ru = histRows + (maxBatch + 7u) / 8u;
    l.U = (gf2p)(c.scratch + batch_scratch_floats_512(maxBatch));
    l.Y = l.U + (size_t)l.Ru * kRow;
    return l;
}
__device__ __forceinline__ uint32_t long_phys(uint32_t l0, uint32_t logical, uint32_t Ru) { const uint32_t r = l0 + logical; return r >= Ru ? r - Ru : r; }

// (tab: the kTabSize twiddle factors of fft4096.h in LDS, filled by long_fill_tab before the first barrier of the kernel)
__device__ __forceinline__ void long_fill_tab(c2* tab, uint32_t tid) {
    for (uint32_t i = tid; i < lfft::kTabSize; i += 256u) tab[i] = kTw8192[lfft::tab_source(i)];
}
template <uint32_t S>
__device__ __forceinline__ void fft4096_pass(c2* buf, const c2* tab, uint32_t tid) {
    c2 v[16];
    lfft::pass_read(buf, tid, v);
    lfft::pass_twiddle_s<S>(v, tid, tab);
    lfft::dft16(v);
    __syncthreads();
    lfft::pass_write_s<S>(buf, tid, v);
    __syncthreads();
}
__device__ __forceinline__ void fft4096_lds(c2* buf, const c2* tab, uint32_t tid) {
    fft4096_pass<0u>(buf, tab, tid); fft4096_pass<1u>(buf, tab, tid); fft4096_pass<2u>(buf, tab, tid);
}

} // namespace

// K1 (node, row): row = c + histRows, chunk c in [-histRows, chunks): U_c = 2 RFFT_8192([chunk c-1 | chunk c])
// (four workgroups per CU: 128 VGPRs, 38 KB of LDS — the r05 build held 158 and ran three, i.e. 1208 workgroups in two rounds)
__global__ __launch_bounds__(256, 4)
void elemhip_convolve_long_fft(PlanView pv, uint32_t* recs, float* hbm, const Globals* g, uint32_t workBegin,
                               uint32_t arenaFloats, float* scratchAll, uint32_t maxBatch, uint32_t batch, uint32_t histRows, uint32_t longMode, size_t perNode,
                               const float* inDirect, uint32_t numInCh) {
    __shared__ c2 buf[lfft::kBuf], tab[lfft::kTabSize];
    const uint32_t convIdx = pv.convWork[workBegin + blockIdx.x] & 0xFFFFu, row = blockIdx.y, tid = threadIdx.x;
    const ConvDesc d = pv.convs[convIdx];
    if (!root_running((gcup)recs, d.rootRec, g->numOut)) return;
    BatchCtx c;
    if (!batch_ctx(d, (gup)recs, g, scratchAll, convIdx, maxBatch, c, perNode) || !conv_use_long(c.st, batch, longMode)) return;
    const LongState ls = long_state_of(c.st);
    const int cc = (int)row - (int)histRows;                       // chunk of the SECOND half of the transform's input
    if (cc < -(int)(ls.Qp - 1u)) return;                            // older than any tap of this node reaches
    const LongCtx l = long_ctx(c, maxBatch, histRows);
    const uint32_t stride = g->blockStride;
    const uint32_t blk0u = c.st.hdr[conv::H_BLK];                   // the node's block counter at the start of the set
    gup sh = (gup)c.scratch;
    const uint32_t uid = c.st.hdr[conv::H_UID];
    const bool carried = uid != 0u && sh[LH_UID] == uid && sh[LH_BLKEND] == blk0u && sh[LH_RU] == l.Ru && sh[LH_ROWNEXT] < l.Ru;
    const uint32_t rowNext = carried ? sh[LH_ROWNEXT] : histRows;   // physical row of this set's chunk 0
    const uint32_t l0 = rowNext >= histRows ? rowNext - histRows : rowNext + l.Ru - histRows;
    if (row == histRows && tid == 0u) { sh[LH_BLK0] = blk0u; sh[LH_L0] = l0; sh[LH_CARRIED] = carried ? 1u : 0u; }   // (chunk 0's workgroup)
    if (carried && cc < 0) return;                                  // the previous set left this spectrum in the ring
    const long long blk0 = (long long)blk0u;
    // z[n] = x[2n] + i x[2n+1], x = [chunk cc - 1 | chunk cc]: element n = tid + 256 r is frames 2 tid, 2 tid + 1 of block (r & 7) of
    // chunk cc - 1 (r < 8) or cc (r >= 8). chunk >= 0: the set's arena (block 8 chunk + i), chunk < 0: the time-domain input ring
    const uint32_t frame = 2u * tid;
#pragma unroll
    for (uint32_t half = 0; half < 2; ++half) {
        const int chunk = half == 0u ? cc - 1 : cc;
        if (chunk >= 0) {
            // (inDirect: a plan of convolvers only reads the caller's [block][channel][frame] input where it lies — no copy into the arenas)
            gcfp base; size_t step;
            if (c.inKind == 1u && inDirect && c.inBuf < kMaxHostIn) { step = (size_t)numInCh * stride; base = (gcfp)inDirect + (size_t)(8u * (uint32_t)chunk) * step + (size_t)c.inBuf * stride + frame; }
            else { step = arenaFloats; base = (gcfp)hbm + (size_t)(8u * (uint32_t)chunk) * step + (size_t)c.inBuf * stride + frame; }
            if (c.inKind == 1u) {
#pragma unroll
                for (uint32_t i = 0; i < 8; ++i) buf[lfft::pad(tid + 256u * (8u * half + i))] = *(gcf2p)(base + (size_t)i * step);
            } else {
#pragma unroll
                for (uint32_t i = 0; i < 8; ++i) buf[lfft::pad(tid + 256u * (8u * half + i))] = mk(c.cval, c.cval);   // a constant input (inKind 4: cval == 0)
            }
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 8; ++i) {
                const long long hb = blk0 + 8ll * chunk + (long long)i;          // (uniform over the workgroup)
                c2 v = mk(0.0f, 0.0f);
                if (hb >= 0) v = *(gcf2p)(ls.hist + (size_t)((uint32_t)hb % ls.R) * 512u + frame);
                buf[lfft::pad(tid + 256u * (8u * half + i))] = v;
            }
        }
    }
    long_fill_tab(tab, tid);
    __syncthreads();
    fft4096_lds(buf, tab, tid);
    gf2p Urow = l.U + (size_t)long_phys(l0, row, l.Ru) * kRow;
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) {
        const uint32_t k = tid + 256u * r;                          // 0 .. 2047 (+ 2048 below)
        c2 a, b;
        lfft::split_forward(buf, k, (const c2*)kTw8192, a, b);
        Urow[k] = a; Urow[lfft::M - k] = b;
    }
    if (tid == 0u) { c2 a, b; lfft::split_forward(buf, 2048u, (const c2*)kTw8192, a, b); Urow[2048] = a; }
}

// K2 (node, 256 bins, run of kLongRun chunks): Y_C[k] = sum_q G_q[k] U_{C-q}[k]. A thread owns one bin and kLongRun consecutive chunks;
// the taps go by in groups of kLongTaps (their G values in registers), and within a group the kLongRun + kLongTaps - 1 spectrum rows
// the group touches are loaded once each and fed to every (chunk, tap) pair on their diagonal — fully unrolled, so that accumulators,
// taps and the row in flight are compile-time registers.
// The grid covers bins 0 .. 4095 in 16 slabs; bin 4096 (the Nyquist bin) is summed by the first kLongRun threads of slab 0, one chunk
// each, behind the main loop (r06: as a 17th slab of one live thread it made C3's grid 1088 workgroups for 1024 places on the chip —
// a second round for 64 workgroups that took as long as a full one).
template <uint32_t RUN>
__global__ __launch_bounds__(256, RUN <= 16u ? 4 : 2)
void elemhip_convolve_long_mac(PlanView pv, uint32_t* recs, float* hbm, const Globals* g, uint32_t workBegin,
                               uint32_t arenaFloats, float* scratchAll, uint32_t maxBatch, uint32_t batch, uint32_t histRows, uint32_t longMode, size_t perNode) {
    const uint32_t convIdx = pv.convWork[workBegin + blockIdx.x] & 0xFFFFu, tid = threadIdx.x;
    const uint32_t k = blockIdx.y * 256u + tid, C0 = blockIdx.z * RUN, chunks = batch / 8u;
    const ConvDesc d = pv.convs[convIdx];
    if (!root_running((gcup)recs, d.rootRec, g->numOut)) return;
    BatchCtx c;
    if (!batch_ctx(d, (gup)recs, g, scratchAll, convIdx, maxBatch, c, perNode) || !conv_use_long(c.st, batch, longMode)) return;
    if (C0 >= chunks) return;
    const LongState ls = long_state_of(c.st);
    const LongCtx l = long_ctx(c, maxBatch, histRows);
    const uint32_t l0 = ((gcup)c.scratch)[LH_L0];
    gcf2p Uk = (gcf2p)l.U + k, Gk = ls.G + k;
    c2 acc[RUN];
#pragma unroll
    for (uint32_t i = 0; i < RUN; ++i) acc[i] = mk(0.0f, 0.0f);
    // The two empty asm statements keep the schedule the loop had when its tap order was a run-time choice: l0 in an SGPR before
    // the loop (else a wait for its scalar load sits in front of every conditional row load) and q0 opaque per group (else the
    // strength-reduced addresses cost more registers). Without them C3's long MAC took 26.9 us per launch instead of 26.5.
    asm volatile("" :: "s"(l0));
    for (uint32_t qi = 0; qi < ls.Qp; qi += kLongTaps) {
        uint32_t q0 = qi;
        asm volatile("" : "+s"(q0));
        c2 gq[kLongTaps];
#pragma unroll
        for (uint32_t t = 0; t < kLongTaps; ++t) gq[t] = Gk[(size_t)(q0 + t) * kRow];
        // rows C0 + dd - q0 - (kLongTaps - 1), dd = 0 .. RUN + kLongTaps - 2; row (chunk i, tap t): dd = i - t + kLongTaps - 1
        const int rowBase = (int)histRows + (int)C0 - (int)q0 - (int)(kLongTaps - 1u);      // >= 0: histRows >= Qp - 1
        c2 u[RUN + kLongTaps - 1u];
#pragma unroll
        for (uint32_t dd = 0; dd < RUN + kLongTaps - 1u; ++dd) {
            const int rr = rowBase + (int)dd;                     // rows behind the set's last chunk feed accumulators that are never stored: not read
            u[dd] = rr < (int)(histRows + chunks) ? Uk[(size_t)long_phys(l0, (uint32_t)rr, l.Ru) * kRow] : mk(0.0f, 0.0f);
        }
#pragma unroll
        for (uint32_t dd = 0; dd < RUN + kLongTaps - 1u; ++dd) {
#pragma unroll
            for (uint32_t t = 0; t < kLongTaps; ++t) {
                const int i = (int)dd + (int)t - (int)(kLongTaps - 1u);
                if (i >= 0 && i < (int)RUN) {
                    const c2 h = gq[t], x = u[dd];
                    acc[i].x = fmaf(h.x, x.x, acc[i].x); acc[i].x = fmaf(-h.y, x.y, acc[i].x);
                    acc[i].y = fmaf(h.x, x.y, acc[i].y); acc[i].y = fmaf(h.y, x.x, acc[i].y);
                }
            }
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < RUN; ++i) if (C0 + i < chunks) l.Y[(size_t)(C0 + i) * kRow + k] = acc[i];
    // bin 4096: thread i of slab 0 sums chunk C0 + i over all taps (both operands are real there; kept as the complex product of the rows)
    if (blockIdx.y == 0u && tid < RUN && C0 + tid < chunks) {
        gcf2p Un = (gcf2p)l.U + lfft::M, Gn = ls.G + lfft::M;
        const uint32_t top = histRows + C0 + tid;                   // logical row of (chunk C0 + tid, tap 0)
        c2 a0 = mk(0.0f, 0.0f), a1 = mk(0.0f, 0.0f);
        for (uint32_t q = 0; q < ls.Qp; q += 2u) {                  // (Qp is a multiple of kLongTaps; rows top - q >= 0: histRows >= Qp - 1)
            const c2 h0 = Gn[(size_t)q * kRow], h1 = Gn[(size_t)(q + 1u) * kRow];
            const c2 x0 = Un[(size_t)long_phys(l0, top - q, l.Ru) * kRow], x1 = Un[(size_t)long_phys(l0, top - q - 1u, l.Ru) * kRow];
            a0.x = fmaf(h0.x, x0.x, a0.x); a0.x = fmaf(-h0.y, x0.y, a0.x); a0.y = fmaf(h0.x, x0.y, a0.y); a0.y = fmaf(h0.y, x0.x, a0.y);
            a1.x = fmaf(h1.x, x1.x, a1.x); a1.x = fmaf(-h1.y, x1.y, a1.x); a1.y = fmaf(h1.x, x1.y, a1.y); a1.y = fmaf(h1.y, x1.x, a1.y);
        }
        l.Y[(size_t)(C0 + tid) * kRow + lfft::M] = mk(a0.x + a1.x, a0.y + a1.y);
    }
}

// K3 (node, chunk C): out chunk C = IRFFT_8192(Y_C)[4096:8192] -> the node's output buffer in the arenas of blocks 8C .. 8C + 7
__global__ __launch_bounds__(256, 4)
void elemhip_convolve_long_ifft(PlanView pv, uint32_t* recs, float* hbm, const Globals* g, uint32_t workBegin,
                                uint32_t arenaFloats, float* scratchAll, uint32_t maxBatch, uint32_t batch, uint32_t histRows, uint32_t longMode, size_t perNode,
                                const float* inDirect, uint32_t numInCh, float* outDirect, uint32_t numOutCh) {
    __shared__ c2 buf[lfft::kBuf], tab[lfft::kTabSize];
    const uint32_t convIdx = pv.convWork[workBegin + blockIdx.x] & 0xFFFFu, C = blockIdx.y, tid = threadIdx.x;
    const ConvDesc d = pv.convs[convIdx];
    if (!root_running((gcup)recs, d.rootRec, g->numOut)) return;
    BatchCtx c;
    if (!batch_ctx(d, (gup)recs, g, scratchAll, convIdx, maxBatch, c, perNode) || !conv_use_long(c.st, batch, longMode)) return;
    const LongCtx l = long_ctx(c, maxBatch, histRows);
    gcf2p Yrow = (gcf2p)l.Y + (size_t)C * kRow;
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) {
        const uint32_t k = tid + 256u * r;
        c2 a, b;
        lfft::split_inverse(Yrow[k], Yrow[lfft::M - k], k, (const c2*)kTw8192, a, b);
        buf[lfft::pad(k)] = a;
        if (k) buf[lfft::pad(lfft::M - k)] = b;
    }
    if (tid == 0u) { c2 a, b; lfft::split_inverse(Yrow[2048], Yrow[2048], 2048u, (const c2*)kTw8192, a, b); buf[lfft::pad(2048u)] = a; }
    long_fill_tab(tab, tid);
    __syncthreads();
    fft4096_lds(buf, tab, tid);
    const uint32_t stride = g->blockStride;
    const float gain = d.fuseRootRec == kNone ? 1.0f : c.gain;
    // (outDirect: every output channel of the call is the folded root of one convolver — the host checked — so the chunk goes straight
    //  into the caller's [block][channel][frame] buffer and the set has no bus-sum epilogue)
    const bool direct = outDirect != nullptr && d.fuseRootRec != kNone;
    const uint32_t outCh = direct ? ((gcup)recs)[d.fuseRootRec * kRecDwords + rec::ROOT_CHANNEL] : 0u;
    // element n = tid + 256 r, r = 8 + i, holds samples 4096 + 512 i + 2 tid (+ 1): frames 2 tid, 2 tid + 1 of the chunk's block i
    {
        const size_t step = direct ? (size_t)numOutCh * stride : (size_t)arenaFloats;
        gfp base = direct ? (gfp)outDirect + (size_t)(8u * C) * step + (size_t)outCh * stride + 2u * tid
                          : (gfp)hbm + (size_t)(8u * C) * step + (size_t)d.outHbm * stride + 2u * tid;
        const uint32_t p8 = lfft::pad(tid + 2048u);                 // pad(tid + 256 (8 + i)) = p8 + 272 i
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i) {
            const c2 f = buf[p8 + 272u * i];
            c2 y = mk(f.x, -f.y);
            if (d.fuseRootRec != kNone) { y.x *= gain; y.y *= gain; }
            *(gf2p)(base + (size_t)i * step) = y;
        }
    }
    // the node's time-domain input ring: this chunk's blocks, where they are among the set's last R (every long_fft workgroup has read
    // its history by now: the ring slots of blocks in front of the set may be reused)
    const LongState ls = long_state_of(c.st);
    const uint32_t b0 = ((gcup)c.scratch)[LH_BLK0];
    if (8u * C + 7u + ls.R >= batch) {                              // (uniform: only the last R / 8 chunks of a set have anything to keep)
#pragma unroll 1
        for (uint32_t i = 0; i < 8; ++i) {
            const uint32_t j = 8u * C + i;
            if (j + ls.R < batch) continue;
            gfp h = ls.hist + (size_t)((b0 + j) % ls.R) * 512u;
            c2 v = mk(c.cval, c.cval);
            if (c.inKind == 1u && inDirect && c.inBuf < kMaxHostIn) v = *(gcf2p)((gcfp)inDirect + ((size_t)j * numInCh + c.inBuf) * stride + 2u * tid);
            else if (c.inKind == 1u) v = *(gcf2p)((gcfp)hbm + (size_t)j * arenaFloats + (size_t)c.inBuf * stride + 2u * tid);
            *(gf2p)(h + 2u * tid) = v;
        }
    }
    // the set's last chunk moves the block counter on; the 512-partition state (spectra ring, overlap) is now behind — made on demand
    // before the next evaluation that reads it (launch_convolve_fix_overlap), never between two long-partition sets
    if (C + 1u == batch / 8u && tid == 0u) {
        c.st.hdr[conv::H_BLK] = b0 + batch; c.st.hdr[conv::H_BLK_NEXT] = b0 + batch;
        c.st.hdr[conv::H_FILL] = 0u; c.st.hdr[conv::H_FILL_NEXT] = 0u;
        c.st.hdr[conv::H_OVL_STALE] = 1u;
        // the spectra ring is current for block b0 + batch of THIS convolver state: the next long set starts behind this one's last chunk
        gup sh = (gup)c.scratch;
        sh[LH_UID] = c.st.hdr[conv::H_UID]; sh[LH_BLKEND] = b0 + batch; sh[LH_RU] = l.Ru;
        sh[LH_ROWNEXT] = long_phys(sh[LH_L0], histRows + batch / 8u, l.Ru);
    }
}

// ---- on demand (launch_convolve_fix_overlap): the 512-partition state of a node a long-partition set rendered last ---------------
// Launched by the host before the next evaluation that reads it — a block-at-a-time call, a set that is no multiple of 8 blocks.
// Between two long-partition sets nobody reads it (overlap-save starts from the input ring), so the steady state of an offline
// render never pays for it (first build: per set, 188 dependent rounds of loads for the overlap alone — 100+ us of a 174 us set).
// (entry, jj): the 1024-point spectrum of the node's jj-th newest block, from the time-domain input ring, into the spectra ring `X`
__global__ __launch_bounds__(256)
void elemhip_convolve_long_state(PlanView pv, uint32_t* recs, float* hbm, const Globals* g, uint32_t workBegin,
                                 float* scratchAll, uint32_t maxBatch, size_t perNode) {
    __shared__ c2 A[conv::kFft], B[conv::kFft], W[conv::kFft];
    const uint32_t entry = pv.convWork[workBegin + blockIdx.x], convIdx = entry & 0xFFFFu, jj = blockIdx.y, tid = threadIdx.x;
    if ((entry >> 16) != 0u) return;                                    // (the fix-up walks the whole work list: helper entries are not nodes)
    const ConvDesc d = pv.convs[convIdx];
    BatchCtx c;
    if (!batch_ctx(d, (gup)recs, g, scratchAll, convIdx, maxBatch, c, perNode)) return;
    if (c.st.hdr[conv::H_OVL_STALE] == 0u) return;
    const LongState ls = long_state_of(c.st);
    const uint32_t blk = c.st.hdr[conv::H_BLK];
    if (jj >= c.st.P || jj >= blk || jj >= ls.R) return;
    const uint32_t b = blk - 1u - jj;
    gcfp h = (gcfp)(ls.hist + (size_t)(b % ls.R) * 512u);
    for (uint32_t i = tid; i < conv::kFft; i += 256u) W[i] = kTwiddle[i];
    A[tid] = mk(h[tid], 0.0f); A[tid + 256u] = mk(h[tid + 256u], 0.0f); A[tid + 512u] = mk(0.0f, 0.0f); A[tid + 768u] = mk(0.0f, 0.0f);
    __syncthreads();
    fft1024(A, B, W, tid);
#pragma unroll
    for (uint32_t q = 0; q < 2; ++q) {
        const uint32_t k = tid + 256u * q;
        c.st.X[(size_t)(b % c.st.P) * 512u + k] = k == 0u ? mk(B[0].x, B[512].x) : B[k];
    }
}

// (entry): the overlap the node's last block leaves behind — the second half of IFFT_1024(sum_p H_p X_{last - p}), exactly what the
// block-at-a-time path would hold after that block
__global__ __launch_bounds__(256)
void elemhip_convolve_long_tail(PlanView pv, uint32_t* recs, float* hbm, const Globals* g, uint32_t workBegin,
                                float* scratchAll, uint32_t maxBatch, size_t perNode) {
    __shared__ c2 A[conv::kFft], B[conv::kFft], W[conv::kFft];
    const uint32_t entry = pv.convWork[workBegin + blockIdx.x], convIdx = entry & 0xFFFFu, tid = threadIdx.x;
    if ((entry >> 16) != 0u) return;
    const ConvDesc d = pv.convs[convIdx];
    BatchCtx c;
    if (!batch_ctx(d, (gup)recs, g, scratchAll, convIdx, maxBatch, c, perNode)) return;
    if (c.st.hdr[conv::H_OVL_STALE] == 0u) return;
    const uint32_t P = c.st.P, blk = c.st.hdr[conv::H_BLK];
    if (blk == 0u) { if (tid == 0u) c.st.hdr[conv::H_OVL_STALE] = 0u; return; }
    const uint32_t last = blk - 1u, lm = last % P;
    for (uint32_t i = tid; i < conv::kFft; i += 256u) W[i] = kTwiddle[i];
    c2 acc[2] = {mk(0.0f, 0.0f), mk(0.0f, 0.0f)};
    for (uint32_t p = 0; p < P; ++p) {
        if (p > last) break;                                           // blocks before the convolver existed: silence
        const uint32_t slot = lm >= p ? lm - p : lm + P - p;
#pragma unroll
        for (uint32_t q = 0; q < 2; ++q) {
            const uint32_t k = tid + 256u * q;
            acc[q] = cadd(acc[q], smul(c.st.H[(size_t)p * 512u + k], c.st.X[(size_t)slot * 512u + k], k == 0u));
        }
    }
#pragma unroll
    for (uint32_t q = 0; q < 2; ++q) {
        const uint32_t k = tid + 256u * q;
        if (k == 0u) { A[0] = mk(acc[q].x, 0.0f); A[512] = mk(acc[q].y, 0.0f); }
        else { A[k] = mk(acc[q].x, -acc[q].y); A[1024u - k] = acc[q]; }
    }
    __syncthreads();
    fft1024(A, B, W, tid);
    for (uint32_t i = tid; i < 512u; i += 256u) c.st.overlap[i] = B[512u + i].x;
    if (tid == 0u) c.st.hdr[conv::H_OVL_STALE] = 0u;
}
