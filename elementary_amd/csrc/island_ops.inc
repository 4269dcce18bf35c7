// island_ops.inc — the node library of the block-render path as hand-written HIP for gfx950 (CDNA4): every op body the
// island kernels run. Shared by the interpreter kernels (island.inc, built ahead of time) and the per-island-shape
// specialised kernels (island_spec.inc, compiled at run time by jit.cpp).
//
// One launch renders one *island level*: every workgroup (4 wavefronts) interprets the program
// of one island with that island's block buffers AND its program resident in LDS.  Stateless node
// loops (runtime/elem/builtins/Math.h etc.) run sample-parallel, 64 lanes x (samples/64);
// stateful recurrences (phasor, polyBLEP phase, one-pole, biquad, SVF, ...) run one node per lane
// with only the loop-carried state update on the serial chain, everything else hoisted into
// sample-parallel pre/post passes, and the chain's operands streamed from LDS with 16-byte reads
// one chunk ahead of the dependent arithmetic.  An epilogue workgroup then sums root buffers into
// the output bus, advances root fades and promotes feedback taps (GraphRenderSequence.h:268-309).
//
// PARITY RULES (SURVEY.md §7): compiled with -ffp-contract=off; float-state recurrences are
// op-for-op the reference's expressions, in the reference's order; nodes that compute in double
// in the reference (SVF, shelf, mm1p, prewarp) compute in double here.
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include "device.h"
#include "launch.h"
#else   // run-time compilation (jit.cpp): device.h is prepended to the program text, no host headers
#ifndef FLT_MAX
#define FLT_MAX 3.402823466e+38F
#endif
#ifndef FLT_EPSILON
#define FLT_EPSILON 1.192092896e-07F
#endif
#endif

using namespace elemhip;

#ifdef ELEMHIP_SPEC
// a specialised kernel knows its island's LDS footprint: one static array, the only LDS object of the image (byte 0)
__shared__ __attribute__((aligned(16))) float lds[ELEMHIP_SPEC_LDS_WORDS];
#else
extern __shared__ __attribute__((aligned(16))) float lds[];
#endif

namespace {

// Global-memory pointers carry an explicit address space. With plain (generic) pointers the
// optimiser merges `cond ? hbm[i] : lds[j]` into one FLAT load of a selected generic pointer,
// and a flat access to LDS costs ~700 cycles instead of ~100.
typedef float __attribute__((address_space(1)))*          gfp;
typedef const float __attribute__((address_space(1)))*    gcfp;
typedef uint32_t __attribute__((address_space(1)))*       gup;
typedef const uint32_t __attribute__((address_space(1)))* gcup;
// node records staged in LDS (see rec_ld_f64 below)
typedef uint32_t __attribute__((address_space(3)))*       rup;
typedef const uint32_t __attribute__((address_space(3)))* rcup;

struct Ctx {
    rup             recs;     // the island's node records, staged in LDS (Member.rec indexes this table)
    gfp             hbm;      // arena slice of the block being rendered (host inputs + exports)
    gfp             hbmS;     // stream-ring slice of the block being rendered (specialised kernels; device.h kOpStream)
    gfp             hbm0;     // base of the whole arena allocation: recurrence streams address it through ONE buffer descriptor
    uint32_t        offE, offS;   // byte offsets of `hbm` / `hbmS` from `hbm0`
    const Globals*  g;
    gcup            lcg;      // [2*(kMaxBlock+1)] jump-ahead table for `rand`
    uint32_t        members;  // LDS word offsets of the staged program tables
    uint32_t        operands;
    uint32_t        n;        // frames this block
    uint32_t        stride;   // floats per arena buffer
    uint32_t        numIn;    // host input channels
    uint32_t        lane;
    float           srF;
    double          sr;
    int64_t         sampleTime;   // of the block being rendered (a multi-block launch advances it per block)
    uint32_t        bset;         // index of that block inside its launch set (0: the realtime path, or the set's first block)
    uint32_t        lo, hi;       // specialised kernels of split islands: the frames [lo, hi) this workgroup renders
    struct Persist* ps;       // set while a kTaskOwnsWave task runs (pipelined launches)
    struct Deferred* defer;   // specialised kernels: a completion-counter update waiting for the previous block's arena stores
};

// A recurrence wave of a specialised kernel does not sit out the L2 round trip of its last stores at the end of a block:
// the counter update that publishes the block is handed to the wave's NEXT piece of work, which performs it as soon as
// its own first loads are issued (vector memory operations complete in issue order, so `vmcnt(those loads)` is exactly
// "the earlier stores have reached L2"), or to the slot walk when there is nothing to run next.
struct Deferred { uint32_t addrBytes, add, pending; };

// Walk state handed to a recurrence task that owns its wave (device.h kTaskOwnsWave): what it needs to publish a block and
// wait for the next one without going back through the walk.
struct Persist {
    uint32_t on;          // the running task has the flag
    uint32_t b, batch;    // block being rendered / blocks in this launch
    uint32_t D;           // buffer sets (Island::copies)
    uint32_t ctr;         // LDS word of the completion counters [stage][D]
    uint32_t s, prev, prevT, lastStage, lastT;   // this slot's stage, the stage it waits on (kNone: none) and its task count, ditto the last stage
    uint32_t slotArea;    // LDS words between the block buffers of consecutive sets
    uint32_t done;        // out: every block rendered and published
    // (unused since the specialised kernels' wave-owning loop was retired; kept: the 512-thread kernel holds this struct in scratch)
    uint32_t arenaBytes, streamBase, streamSlice, ntasks;
};

#define WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
#define UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
// NO s_wakeup ANYWHERE in these kernels. On gfx950 an s_wakeup executed by one wave ends an `s_nop N` (N > 0) that ANOTHER wave of
// the workgroup is sitting in — and `s_nop N` is what the compiler inserts for the wait states the ISA wants between, e.g., a
// v_readfirstlane that writes an SGPR and the VMEM instruction that uses it as its base: the store then goes out with the STALE
// pair. tools/micro/wakeup_nop.hip measures it in isolation (profiles/r04/micro_s_wakeup_truncates_s_nop.txt: 50 010 of 300 000
// stores misplaced next to waves that ping, none without the pings, none when the wait states are five `s_nop 0`). It is what
// made the specialised kernels of tap islands fault and mis-render one block in ~150 in r03 (a tapOut stores through such a pair;
// profiles/r04/tap_spec_bisect_matrix.txt). Waiting waves therefore poll with a short s_sleep and are never pinged.

__device__ __forceinline__ float    u2f(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ uint32_t f2u(float f)    { return __float_as_uint(f); }
__device__ __forceinline__ uint32_t ldsu(uint32_t w) { return __float_as_uint(lds[w]); }
// The island kernel is one huge loop (walk -> task switch -> publish). Anything loop-invariant that lives in a VGPR (the
// lane id and what derives from it, LDS addresses of the walk's own tables) gets hoisted by the compiler and then, under
// the register pressure of the biggest task bodies, spilled to scratch — and reloaded on the hand-over path between two
// tasks with a full memory round trip each. These two make such values opaque per iteration, so they are recomputed
// (one or two ALU instructions) instead of kept.
__device__ __forceinline__ uint32_t opaque_zero() { uint32_t z; asm volatile("s_mov_b32 %0, 0" : "=s"(z)); return z; }
// A wave-uniform POD that was fetched with vector loads (the compiler cannot prove the plan tables read-only, so it does
// not use scalar loads): move every dword to an SGPR. Left in VGPRs, such values are the loop-carried registers the
// allocator spills to scratch.
template <typename T>
__device__ __forceinline__ T uni_pod(const T& x) {
    static_assert(sizeof(T) % 4 == 0, "dword-sized POD");
    uint32_t d[sizeof(T) / 4];
    __builtin_memcpy(d, &x, sizeof(T));
#pragma unroll
    for (uint32_t i = 0; i < sizeof(T) / 4; ++i) d[i] = UNI(d[i]);
    T r;
    __builtin_memcpy(&r, d, sizeof(T));
    return r;
}
__device__ __forceinline__ uint32_t opaque_lane() {
    uint32_t l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

__device__ __forceinline__ void deferred_publish_now(Deferred& d) {   // the caller has waited for the stores
    uint32_t t0_, t1_;
    if (opaque_lane() == 0)
        asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3\n\tds_add_u32 %0, %1" : "=&v"(t0_), "=&v"(t1_) : "s"(d.addrBytes), "s"(d.add) : "memory");
    WAVE_SYNC();
    d.pending = 0u;
}
// KEEP = vector memory operations issued after the stores in question that may stay in flight
template <int KEEP>
__device__ __forceinline__ void take_deferred(Deferred* d) {
    if (d == nullptr || d->pending == 0u) return;
    static_assert(KEEP >= 0 && KEEP < 64, "vmcnt is a 6-bit counter");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt((uint32_t)(((KEEP >> 4) & 3) << 14 | (KEEP & 15) | 0x0070));   // vmcnt(KEEP) lgkmcnt(0)
    deferred_publish_now(*d);
}

// Node records are staged in LDS for the duration of a launch (the island kernel copies the island's records in at the
// start and back at the end), so the render code reads and writes node state through LDS pointers: a task's state round
// trip through global memory cost ~3 k cycles on a lone wave. Global record pointers remain for the epilogue kernels.
template <typename P>
__device__ __forceinline__ double rec_ld_f64(P r, uint32_t d) {
    return __hiloint2double((int)r[d + 1], (int)r[d]);
}
template <typename P>
__device__ __forceinline__ void rec_st_f64(P r, uint32_t d, double v) {
    r[d] = (uint32_t)__double2loint(v); r[d + 1] = (uint32_t)__double2hiint(v);
}
template <typename P>
__device__ __forceinline__ gfp rec_ptr(P r, uint32_t d) {
    uint64_t p = (uint64_t)r[d] | ((uint64_t)r[d + 1] << 32);
    return (gfp)reinterpret_cast<float*>(p);
}

// the same through wave-uniform (scalar) values: the record word is read once and broadcast
template <typename P>
__device__ __forceinline__ gfp rec_ptr_uni(P r, uint32_t d) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)r[d]), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)r[d + 1]);
    return (gfp)reinterpret_cast<float*>((uint64_t)lo | ((uint64_t)hi << 32));
}

__device__ __forceinline__ float clampf(float v, float lo, float hi) {   // std::clamp
    return (v < lo) ? lo : ((hi < v) ? hi : v);
}
__device__ __forceinline__ double clampd(double v, double lo, double hi) {
    return (v < lo) ? lo : ((hi < v) ? hi : v);
}

// arena buffer `v` (an operand value or Member::outHbm; never kNone) of the block being rendered
__device__ __forceinline__ gfp hbm_buf(const Ctx& c, uint32_t v) {
#ifdef ELEMHIP_SPEC
    return (v & kOpStream) ? c.hbmS + (size_t)(v & ~(uint32_t)kOpStream) * c.stride : c.hbm + (size_t)v * c.stride;
#else
    return c.hbm + (size_t)v * c.stride;
#endif
}
// ... and its byte offset from the arena base (recurrence streams: buffer loads / stores over the whole arena)
__device__ __forceinline__ uint32_t hbm_off(const Ctx& c, uint32_t v) {
#ifdef ELEMHIP_SPEC
    return (v & kOpStream) ? c.offS + (v & ~(uint32_t)kOpStream) * c.stride * 4u : c.offE + v * c.stride * 4u;
#else
    return c.offE + v * c.stride * 4u;
#endif
}

// ---- program access (staged in LDS) ------------------------------------------------------------
typedef float    v4f __attribute__((ext_vector_type(4)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef double   v2d __attribute__((ext_vector_type(2)));

// 16-byte LDS accesses: the compiler only emits ds_read_b128 / ds_write_b128 when told the
// address is aligned (every slot, scratch array and program table is laid out on 16 bytes)
__device__ __forceinline__ v4u lds4u(uint32_t w) { return *reinterpret_cast<const v4u*>(__builtin_assume_aligned(&lds[w], 16)); }
// Walk-only LDS accessors (uniform word index in, SGPR-addressed): the byte address is moved from a scalar into a
// scratch VGPR right at the access, so the walk keeps no loop-carried VGPR address (see opaque_zero above). The dynamic
// LDS segment of the island kernels starts at LDS byte 0 (they have no static __shared__; checked at kernel entry).
__device__ __forceinline__ void wlds_ld8(uint32_t w, v4u& a, v4u& b) {
    uint32_t t;
    asm volatile("v_mov_b32 %2, %3\n\tds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:16\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(a), "=&v"(b), "=&v"(t) : "s"(w << 2) : "memory");
}
__device__ __forceinline__ void wlds_ld8_1(uint32_t w, uint32_t w1, v4u& a, v4u& b, uint32_t& x) {
    uint32_t t0, t1;
    asm volatile("v_mov_b32 %3, %5\n\tv_mov_b32 %4, %6\n\tds_read_b128 %0, %3\n\tds_read_b128 %1, %3 offset:16\n\t"
                 "ds_read_b32 %2, %4\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(a), "=&v"(b), "=&v"(x), "=&v"(t0), "=&v"(t1) : "s"(w << 2), "s"(w1 << 2) : "memory");
}
__device__ __forceinline__ void wlds_ld2(uint32_t w0, uint32_t w1, uint32_t& x0, uint32_t& x1) {
    asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3\n\tds_read_b32 %0, %0\n\tds_read_b32 %1, %1\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(x0), "=&v"(x1) : "s"(w0 << 2), "s"(w1 << 2) : "memory");
}
// executed by ONE lane: completion counter += add, then the slot's next-block word
__device__ __forceinline__ void wlds_publish(uint32_t ctrW, uint32_t add, uint32_t nbW, uint32_t nb) {
    uint32_t t0, t1;
    asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3\n\tds_add_u32 %0, %1\n\tv_mov_b32 %0, %4\n\tv_mov_b32 %1, %5\n\tds_write_b32 %0, %1"
                 : "=&v"(t0), "=&v"(t1) : "s"(ctrW << 2), "s"(add), "s"(nbW << 2), "s"(nb) : "memory");
}
__device__ __forceinline__ v4f ld4(uint32_t w) { return *reinterpret_cast<const v4f*>(__builtin_assume_aligned(&lds[w], 16)); }
__device__ __forceinline__ void st4(uint32_t w, v4f v) { *reinterpret_cast<v4f*>(__builtin_assume_aligned(&lds[w], 16)) = v; }
__device__ __forceinline__ v2d ld2d(const double* p) { return *reinterpret_cast<const v2d*>(__builtin_assume_aligned(p, 16)); }

__device__ __forceinline__ Member member_uniform(const Ctx& c, uint32_t k) {   // same k on every lane
    const uint32_t w = c.members + k * 8u;
    const v4u a = lds4u(w);
    Member m;
    m.rec = UNI(a.x); m.opnd = UNI(a.y); m.nin = UNI(a.z); m.outLds = UNI(a.w);
    m.outHbm = UNI(ldsu(w + 4)); m.scratch = UNI(ldsu(w + 5));
    // pad0_/pad1_ carry the first two operand codes on the device
    m.pad0_ = UNI(ldsu(c.operands + m.opnd)); m.pad1_ = UNI(ldsu(c.operands + m.opnd + 1));
    return m;
}
__device__ __forceinline__ Member member_lane(const Ctx& c, uint32_t k) {      // per-lane k
    const uint32_t w = c.members + k * 8u;
    const v4u a = lds4u(w);
    Member m;
    m.rec = a.x; m.opnd = a.y; m.nin = a.z; m.outLds = a.w;
    m.outHbm = ldsu(w + 4); m.scratch = ldsu(w + 5);
    return m;
}
__device__ __forceinline__ uint32_t member_nin(const Ctx& c, const Member& m) {
    return m.nin == kNone ? c.numIn : m.nin;
}
#ifdef ELEMHIP_SPEC
// operand codes of a specialised kernel: LDS-buffer operands of the staged table (buffer set 0) move to the member's set
__device__ __forceinline__ uint32_t spec_adj(uint32_t o, uint32_t off) { return (o & kOpKindMask) == kOpLds ? o + off : o; }
// (a k the compiler cannot fold — `in` picks its channel from the node record — goes to the staged operand table: indexing
//  m.sops[] with a run-time k put the member in scratch memory, 72 bytes per lane and a scratch round trip per `in` task)
__device__ __forceinline__ uint32_t opnd_uniform(const Ctx& c, const Member& m, uint32_t k) {
    if (__builtin_constant_p(k) && k < 6u) return m.sops[k];    // folds to the constant the generator wrote
    return spec_adj(UNI(ldsu(c.operands + m.opnd + k)), m.off);
}
__device__ __forceinline__ uint32_t opnd_lane(const Ctx& c, const Member& m, uint32_t k) {
    if (__builtin_constant_p(k) && k < 6u) return m.sops[k];
    return spec_adj(ldsu(c.operands + m.opnd + k), m.off);
}
__device__ __forceinline__ uint32_t opnd_tab(const Ctx& c, const Member& m, uint32_t idx) { return spec_adj(ldsu(c.operands + m.opnd + idx), m.off); }
#else
__device__ __forceinline__ uint32_t opnd_uniform(const Ctx& c, const Member& m, uint32_t k) {
    if (k == 0) return m.pad0_;      // decoded with the task header / member
    if (k == 1) return m.pad1_;
    return UNI(ldsu(c.operands + m.opnd + k));
}
__device__ __forceinline__ uint32_t opnd_lane(const Ctx& c, const Member& m, uint32_t k) {
    return ldsu(c.operands + m.opnd + k);
}
__device__ __forceinline__ uint32_t opnd_tab(const Ctx& c, const Member& m, uint32_t idx) { return ldsu(c.operands + m.opnd + idx); }
#endif

// Sample-parallel operand: LDS buffer (step 1) / broadcast cell (step 0) share one addressing
// form, HBM buffers are the other; both are wave-uniform so the choice is a scalar branch made
// once per operand, outside the sample loop.
struct PIn { uint32_t base, step; gcfp g; bool isG; };   // isG: an HBM arena buffer (a flag, not g != nullptr: see SIn)
__device__ __forceinline__ PIn pin_of(const Ctx& c, uint32_t o) {
    // arithmetic selects only: an if/else ladder here compiled to ~30 scalar instructions of control flow
    const uint32_t kind = o >> 30, v = o & kOpValMask;
    PIn p;
    p.step = (kind == 0u) ? 1u : 0u;                     // LDS buffer
    p.base = (kind <= 1u) ? v : 0u;                      // buffer / broadcast cell; otherwise LDS word 0 (= 0.0f)
    const uint64_t ga = (uint64_t)(uintptr_t)(float*)hbm_buf(c, v);
    p.g = (gcfp)(float*)(uintptr_t)((kind == 2u) ? ga : 0ull);
    p.isG = kind == 2u;
    return p;
}
__device__ __forceinline__ float pget(const PIn& p, uint32_t i) { return p.isG ? p.g[i] : lds[p.base + i * p.step]; }
__device__ __forceinline__ float fetch(const Ctx& c, uint32_t o, uint32_t i) {
    const uint32_t kind = o & kOpKindMask, v = o & kOpValMask;
    if (kind == kOpLds)   return lds[v + i];
    if (kind == kOpConst) return lds[v];
    if (kind == kOpHbm)   return hbm_buf(c, v)[i];
    return 0.0f;
}
__device__ __forceinline__ void put(const Ctx& c, const Member& m, uint32_t i, float y) {
    if (m.outLds != kNone) lds[m.outLds + i] = y;
    if (m.outHbm != kNone) hbm_buf(c, m.outHbm)[i] = y;
}
__device__ __forceinline__ void zero_fill(const Ctx& c, const Member& m, uint32_t s0, uint32_t s1) {
    for (uint32_t i = s0 + c.lane; i < s1; i += 64) put(c, m, i, 0.0f);
}

// Canonical frame mapping of sample-parallel tasks: a task covers 64*V frames, V in {1,2,4,8}
// (the planner only emits such ranges), and lane l owns the V CONSECUTIVE frames i .. i+V-1 with
// i = s0 + l*V: one vector LDS/global access per operand, no per-frame control flow. Every
// sample-parallel op uses this mapping, which is what lets dependent ops of one stage run back
// to back on a wave without a barrier (each lane only re-reads what it wrote itself).
typedef float v2f __attribute__((ext_vector_type(2)));
typedef const v2f __attribute__((address_space(1)))* gcv2;
typedef const v4f __attribute__((address_space(1)))* gcv4;
typedef v2f __attribute__((address_space(1)))* gv2;
typedef v4f __attribute__((address_space(1)))* gv4;

template <int V>
__device__ __forceinline__ void vload(const PIn& p, uint32_t i, float (&x)[V]) {
    if (p.isG) {
        if constexpr (V == 1) x[0] = p.g[i];
        else if constexpr (V == 2) { const v2f a = *(gcv2)(p.g + i); x[0] = a.x; x[1] = a.y; }
        else {
#pragma unroll
            for (int q = 0; q < V; q += 4) { const v4f a = *(gcv4)(p.g + i + q); x[q] = a.x; x[q + 1] = a.y; x[q + 2] = a.z; x[q + 3] = a.w; }
        }
    } else if (p.step) {
        const uint32_t w = p.base + i;
        if constexpr (V == 1) x[0] = lds[w];
        else if constexpr (V == 2) { const v2f a = *reinterpret_cast<const v2f*>(__builtin_assume_aligned(&lds[w], 8)); x[0] = a.x; x[1] = a.y; }
        else {
#pragma unroll
            for (int q = 0; q < V; q += 4) { const v4f a = ld4(w + q); x[q] = a.x; x[q + 1] = a.y; x[q + 2] = a.z; x[q + 3] = a.w; }
        }
    } else {
        const float v = lds[p.base];
#pragma unroll
        for (int q = 0; q < V; ++q) x[q] = v;
    }
}

// nlim = first frame that must NOT be written (block shorter than the task range => per-frame tail)
template <int V>
__device__ __forceinline__ void vstore(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim, const float (&y)[V]) {
    if (i + V <= nlim) {
        if (m.outLds != kNone) {
            const uint32_t w = m.outLds + i;
            if constexpr (V == 1) lds[w] = y[0];
            else if constexpr (V == 2) { v2f a; a.x = y[0]; a.y = y[1]; *reinterpret_cast<v2f*>(__builtin_assume_aligned(&lds[w], 8)) = a; }
            else {
#pragma unroll
                for (int q = 0; q < V; q += 4) { v4f a; a.x = y[q]; a.y = y[q + 1]; a.z = y[q + 2]; a.w = y[q + 3]; st4(w + q, a); }
            }
        }
        if (m.outHbm != kNone) {
            gfp g = hbm_buf(c, m.outHbm) + i;
            if constexpr (V == 1) g[0] = y[0];
            else if constexpr (V == 2) { v2f a; a.x = y[0]; a.y = y[1]; *(gv2)g = a; }
            else {
#pragma unroll
                for (int q = 0; q < V; q += 4) { v4f a; a.x = y[q]; a.y = y[q + 1]; a.z = y[q + 2]; a.w = y[q + 3]; *(gv4)(g + q) = a; }
            }
        }
    } else {
#pragma unroll
        for (int q = 0; q < V; ++q) if (i + q < nlim) put(c, m, i + q, y[q]);
    }
}

template <int V>
__device__ __forceinline__ void vzero(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim) {
    float z[V];
#pragma unroll
    for (int q = 0; q < V; ++q) z[q] = 0.0f;
    vstore<V>(c, m, i, nlim, z);
}

// ---- stateless math (Math.h) -------------------------------------------------------------
__device__ __forceinline__ float unary_eval(uint16_t op, float x) {
    switch (op) {
        case OP_SIN:   return sinf(x);
        case OP_COS:   return cosf(x);
        case OP_TAN:   return tanf(x);
        case OP_TANH:  return tanhf(x);
        case OP_ASINH: return asinhf(x);
        case OP_LN:    return logf(x);
        case OP_LOG:   return log10f(x);
        case OP_LOG2:  return log2f(x);
        case OP_CEIL:  return ceilf(x);
        case OP_FLOOR: return floorf(x);
        case OP_ROUND: return roundf(x);
        case OP_SQRT:  return sqrtf(x);
        case OP_EXP:   return expf(x);
        default:       return fabsf(x);   // OP_ABS
    }
}

__device__ __forceinline__ float binary_eval(uint16_t op, float x, float y) {
    switch (op) {
        case OP_LE:  return (x < y)  ? 1.0f : 0.0f;
        case OP_LEQ: return (x <= y) ? 1.0f : 0.0f;
        case OP_GE:  return (x > y)  ? 1.0f : 0.0f;
        case OP_GEQ: return (x >= y) ? 1.0f : 0.0f;
        case OP_POW: // SafePow, Math.h:179-188
            if (x < 0.0f && y != floorf(y)) return 0.0f;
            return powf(x, y);
        case OP_EQ:  return (fabsf(x - y) <= FLT_EPSILON) ? 1.0f : 0.0f;
        case OP_AND: return (fabsf(1.0f - x) <= FLT_EPSILON && fabsf(1.0f - y) <= FLT_EPSILON) ? 1.0f : 0.0f;
        default:     return (fabsf(1.0f - x) <= FLT_EPSILON || fabsf(1.0f - y) <= FLT_EPSILON) ? 1.0f : 0.0f; // OP_OR
    }
}

__device__ __forceinline__ float reduce_eval(uint16_t op, float a, float b) {
    switch (op) {
        case OP_ADD: return a + b;
        case OP_SUB: return a - b;
        case OP_MUL: return a * b;
        case OP_DIV: return (b == 0.0f) ? 0.0f : a / b;   // SafeDivides, Math.h:135-140
        case OP_MOD: return fmodf(a, b);
        case OP_MIN: return (b < a) ? b : a;               // std::min
        default:     return (a < b) ? b : a;               // std::max
    }
}

template <uint16_t OPC, int V>
__device__ __forceinline__ void run_unary(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim) {
    if (member_nin(c, m) < 1) return vzero<V>(c, m, i, nlim);
    float x[V];
    vload<V>(pin_of(c, opnd_uniform(c, m, 0)), i, x);
#pragma unroll
    for (int q = 0; q < V; ++q) x[q] = unary_eval(OPC, x[q]);
    vstore<V>(c, m, i, nlim, x);
}

template <uint16_t OPC, int V>
__device__ __forceinline__ void run_binary(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim) {
    if (member_nin(c, m) < 2) return vzero<V>(c, m, i, nlim);
    float x[V], y[V];
    vload<V>(pin_of(c, opnd_uniform(c, m, 0)), i, x);
    vload<V>(pin_of(c, opnd_uniform(c, m, 1)), i, y);
#pragma unroll
    for (int q = 0; q < V; ++q) x[q] = binary_eval(OPC, x[q], y[q]);
    vstore<V>(c, m, i, nlim, x);
}

// BinaryReducingNode (Math.h:59-89): strict left fold over the children, any fan-in. Operand
// codes are fetched 64 at a time (lane b reads code k+b with one LDS access, v_readlane
// broadcasts them) and the loads of a batch of children are all in flight before the ordered fold.
template <uint16_t OPC, int V>
__device__ __forceinline__ void run_reduce(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim) {
    uint32_t nin = member_nin(c, m);
    if (nin < 1) return vzero<V>(c, m, i, nlim);
    if (m.nin == kNone && nin > kMaxHostIn) nin = kMaxHostIn;
    float acc[V];
    vload<V>(pin_of(c, opnd_uniform(c, m, 0)), i, acc);
    if (nin == 2) {
        float y[V];
        vload<V>(pin_of(c, opnd_uniform(c, m, 1)), i, y);
#pragma unroll
        for (int q = 0; q < V; ++q) acc[q] = reduce_eval(OPC, acc[q], y[q]);
        return vstore<V>(c, m, i, nlim, acc);
    }
    constexpr int KB = (V <= 2) ? 16 : (V == 4 ? 8 : 4);   // children in flight (KB * V registers)
    uint32_t k = 1;
    // all HBM children (a mixer): one buffer descriptor over the arena, child offset in an SGPR —
    // 4 instructions per child (v_readlane, s_and, s_mul, buffer_load) instead of a generic decode
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((float*)c.hbm, 0, 0x7FFFFFFF, 0x00020000);
    const uint32_t strideBytes = c.stride * 4u;
    while (k < nin) {
        const uint32_t left = min(nin - k, 64u);
        const uint32_t mine = (c.lane < left) ? opnd_tab(c, m, k + c.lane) : (uint32_t)kOpZero;
        const bool allHbm = (V <= 2) && __all(c.lane >= left || ((mine >> 30) == 2u && (mine & kOpValMask) < (0x7FFFFFFFu / strideBytes)));
        if (allHbm) {
            constexpr int KH = (V == 1) ? 64 : 32;   // one memory round trip per 64 children
            for (uint32_t b0 = 0; b0 < left; b0 += KH) {
                float v[KH][V];
#pragma unroll
                for (int b = 0; b < KH; ++b) {
                    if (b0 + b < left) {
                        const uint32_t code = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)(b0 + b));
                        const uint32_t soff = (code & kOpValMask) * strideBytes;
                        if constexpr (V == 1) v[b][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, i * 4u, soff, 0));
                        else { const v2f t2 = __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(rsrc, i * 4u, soff, 0)); v[b][0] = t2.x; v[b][V - 1] = t2.y; }
                    }
                }
#pragma unroll
                for (int b = 0; b < KH; ++b)
                    if (b0 + b < left) {
#pragma unroll
                        for (int q = 0; q < V; ++q) acc[q] = reduce_eval(OPC, acc[q], v[b][q]);
                    }
            }
        } else {
            for (uint32_t b0 = 0; b0 < left; b0 += KB) {
                float v[KB][V];
#pragma unroll
                for (int b = 0; b < KB; ++b)
                    if (b0 + b < left) vload<V>(pin_of(c, (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)(b0 + b))), i, v[b]);
#pragma unroll
                for (int b = 0; b < KB; ++b)
                    if (b0 + b < left) {
#pragma unroll
                        for (int q = 0; q < V; ++q) acc[q] = reduce_eval(OPC, acc[q], v[b][q]);
                    }
            }
        }
        k += left;
    }
    vstore<V>(c, m, i, nlim, acc);
}

// Per-frame form for the less common sample-parallel nodes: f(frame) -> value, same mapping.
template <int V, typename F>
__device__ __forceinline__ void vmap(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim, F&& f) {
    float y[V];
#pragma unroll
    for (int q = 0; q < V; ++q) y[q] = f(i + q);
    vstore<V>(c, m, i, nlim, y);
}

// IdentityNode `in` (Math.h:92-126): out = inputData[channel]; leaf => host input channel.
template <int V>
__device__ __forceinline__ void run_in(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim) {
    const uint32_t ch = UNI(c.recs[m.rec * kRecDwords + rec::P0]);
    const uint32_t nin = member_nin(c, m);
    const bool neg = (int32_t)ch < 0;   // static_cast<size_t>(negative int) is huge: zero-fill
    if (neg || ch >= nin || (m.nin == kNone && ch >= kMaxHostIn)) return vzero<V>(c, m, i, nlim);
    float x[V];
    vload<V>(pin_of(c, opnd_uniform(c, m, ch)), i, x);
    vstore<V>(c, m, i, nlim, x);
}

template <int V>
__device__ __forceinline__ void run_copy(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim) {
    float x[V];
    vload<V>(pin_of(c, opnd_uniform(c, m, 0)), i, x);
    vstore<V>(c, m, i, nlim, x);
}

// RootNode (Core.h:66-78) + GainFade::process (helpers/GainFade.h:56-72). The gain itself is
// advanced once per block by the epilogue, after every island has read it.
template <int V>
__device__ __forceinline__ void run_root(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim) {
    if (member_nin(c, m) < 1) return vzero<V>(c, m, i, nlim);
    rcup r = c.recs + m.rec * kRecDwords;
    const float g = u2f(UNI(r[rec::ROOT_GAIN])), tg = u2f(UNI(r[rec::ROOT_TARGET])), step = u2f(UNI(r[rec::ROOT_STEP]));
    float x[V];
    vload<V>(pin_of(c, opnd_uniform(c, m, 0)), i, x);
    if (g == tg) {
#pragma unroll
        for (int q = 0; q < V; ++q) x[q] = x[q] * tg;
    } else {
#pragma unroll
        for (int q = 0; q < V; ++q) x[q] = x[q] * clampf(g + step * (float)(int)(i + q), 0.0f, 1.0f);
    }
    vstore<V>(c, m, i, nlim, x);
}

// CutoffPrewarpNode (filters/MultiMode1p.h:9-36): double internals.
template <int V>
__device__ __forceinline__ void run_prewarp(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim) {
    if (member_nin(c, m) < 1) return vzero<V>(c, m, i, nlim);
    const double T = 1.0 / c.sr;
    float x[V];
    vload<V>(pin_of(c, opnd_uniform(c, m, 0)), i, x);
#pragma unroll
    for (int q = 0; q < V; ++q) {
        const double twoPi = 2.0 * 3.141592653589793238;
        const double wd = twoPi * (double)x[q];
        x[q] = (float)tan(wd * T / 2.0);
    }
    vstore<V>(c, m, i, nlim, x);
}

// SampleTimeNode (wasm/SampleTime.h:11-24), MetronomeNode (wasm/Metro.h:40-55)
template <int V>
__device__ __forceinline__ void run_time(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim) {
    const int64_t st = c.sampleTime;
    vmap<V>(c, m, i, nlim, [&](uint32_t t) { return (float)(double)((uint64_t)st + (uint64_t)t); });
}
template <int V>
__device__ __forceinline__ void run_metro(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim) {
    rcup r = c.recs + m.rec * kRecDwords;
    const int64_t is64 = (int64_t)((uint64_t)r[rec::P0] | ((uint64_t)r[rec::P1] << 32));
    const double is = (double)is64;
    const int64_t st = c.sampleTime;
    vmap<V>(c, m, i, nlim, [&](uint32_t t) {
        const double tt = (double)((uint64_t)st + (uint64_t)t) / is;
        return ((tt - floor(tt)) < 0.5) ? 1.0f : 0.0f;
    });
}

// TableNode (Table.h:35-71): clamp, scale, linear interpolation with wrapping neighbours
template <int V>
__device__ __forceinline__ void run_table(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim) {
    rcup r = c.recs + m.rec * kRecDwords;
    gcfp buf = rec_ptr(r, rec::TBL_BUF);
    const int size = (int)UNI(r[rec::TBL_LEN]);
    if (member_nin(c, m) < 1 || !buf || size == 0) return vzero<V>(c, m, i, nlim);
    float x[V];
    vload<V>(pin_of(c, opnd_uniform(c, m, 0)), i, x);
#pragma unroll
    for (int q = 0; q < V; ++q) {
        const float readPos = clampf(x[q], 0.0f, 1.0f) * (float)(size - 1);
        const int readLeft = (int)readPos, readRight = readLeft + 1;
        const float frac = readPos - floorf(readPos);
        const float left = buf[readLeft % size], right = buf[readRight % size];
        x[q] = left + frac * (right - left);
    }
    vstore<V>(c, m, i, nlim, x);
}

// SparSeq2Node (SparSeq2.h:68-127). The event bounds the reference carries from sample to sample are, after
// each update, always (prev(upper_bound(t)), upper_bound(t)) — the 1e-9 tolerances only decide WHEN it looks
// them up again — so the output is a pure function of t: a binary search per frame, no serial state.
template <int V>
__device__ __forceinline__ void run_sparseq2(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim) {
    rcup r = c.recs + m.rec * kRecDwords;
    gcup seq = (gcup)rec_ptr(r, rec::SPS_SEQ);
    const uint32_t len = UNI(r[rec::SPS_LEN]);
    if (member_nin(c, m) < 1 || !seq || len == 0u) return vzero<V>(c, m, i, nlim);
    const bool interp = (int)UNI(r[rec::SPS_INTERP]) == 1;
    gcfp values = (gcfp)(seq + 2u * len);
    float x[V];
    vload<V>(pin_of(c, opnd_uniform(c, m, 0)), i, x);
#pragma unroll
    for (int q = 0; q < V; ++q) {
        const double t = (double)x[q];
        uint32_t lo = 0, hi = len;                                  // upper_bound(t)
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (rec_ld_f64(seq, 2u * mid) > t) hi = mid; else lo = mid + 1u; }
        float y;
        if (lo == 0u) y = 0.0f;                                      // before the first event
        else if (lo == len) y = values[len - 1u];                    // after the last one
        else {
            const double tp = rec_ld_f64(seq, 2u * (lo - 1u)), tn = rec_ld_f64(seq, 2u * lo);
            const double alpha = interp ? ((t - tp) / (tn - tp)) : 0.0;
            const float vp = values[lo - 1u], vn = values[lo];
            y = vp + (float)alpha * (vn - vp);
        }
        x[q] = y;
    }
    vstore<V>(c, m, i, nlim, x);
}

// TapInNode / TapOutNode (Feedback.h:40-53, 111-126); buffers are always float.
// Inside a launch set the end-of-block promotion (GraphRenderSequence.h:297-308) does not happen between two blocks. A tapIn
// whose tapOut sits in the same island (plan.cpp "taps inside launch sets": one block in flight, the tapOut at least a stage
// behind) is handed the tapOut's LDS slot in Member::scratch: from the set's second block on that slot still holds what the
// promotion would have copied, and the island's completion counters order the hand-over like every other LDS buffer — no
// global memory between two waves of the workgroup. The set's first block (and the block-at-a-time path) reads the shared
// buffer the last promotion left; the tapOut keeps writing its private buffer for the set's one promotion.
template <int V>
__device__ __forceinline__ void run_tapin(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim) {
    if (c.bset > 0u && m.scratch != kNone) {
        float x[V];
        vload<V>(PIn{m.scratch, 1u, (gcfp)nullptr, false}, i, x);
        return vstore<V>(c, m, i, nlim, x);
    }
    rcup r = c.recs + m.rec * kRecDwords;
    gcfp shared = rec_ptr_uni(r, rec::TAP_SHARED);   // (wave-uniform: one record read, broadcast)
    if (!shared) return vzero<V>(c, m, i, nlim);
    vmap<V>(c, m, i, nlim, [&](uint32_t t) { return shared[t]; });
}
template <int V>
__device__ __forceinline__ void run_tapout(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim) {
    rcup r = c.recs + m.rec * kRecDwords;
    if (member_nin(c, m) < 1) return vzero<V>(c, m, i, nlim);
    gfp priv = rec_ptr_uni(r, rec::TAP_PRIVATE);
    float x[V];
    vload<V>(pin_of(c, opnd_uniform(c, m, 0)), i, x);
#pragma unroll
    for (int q = 0; q < V; ++q) if (i + q < nlim) priv[i + q] = x[q];
    vstore<V>(c, m, i, nlim, x);
}

template <int V>
__device__ __forceinline__ void run_fill(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim) {
    const float v = u2f(UNI(c.recs[m.rec * kRecDwords + rec::P0]));
    vmap<V>(c, m, i, nlim, [&](uint32_t) { return v; });
}

// UniformRandomNoiseNode (Noise.h:9-43): the LCG is affine mod 2^32, so sample i is an exact
// jump-ahead  s_{i+1} = A[i+1]*s_0 + C[i+1]  from a precomputed table — bit-identical, no chain.
__device__ __forceinline__ void run_rand(const Ctx& c, const Member& m, uint32_t s0, uint32_t s1) {
    rup r = c.recs + m.rec * kRecDwords;
    const uint32_t seed = r[rec::S0];
    for (uint32_t i = s0 + c.lane; i < s1; i += 64) {
        const uint32_t s = c.lcg[2 * (i + 1)] * seed + c.lcg[2 * (i + 1) + 1];
        put(c, m, i, (float)(int)((s >> 16) & 0x7FFF) / 32767.0f);
    }
    WAVE_SYNC();
    if (c.lane == 0) r[rec::S0] = c.lcg[2 * c.n] * seed + c.lcg[2 * c.n + 1];
}

// SingleSampleDelayNode (Delays.h:15-39): out[i] = (i ? in[i-1] : z); z = in[n-1]
__device__ __forceinline__ void run_z(const Ctx& c, const Member& m, uint32_t s0, uint32_t s1) {
    if (member_nin(c, m) < 1) return zero_fill(c, m, s0, s1);
    rup r = c.recs + m.rec * kRecDwords;
    const uint32_t o = opnd_uniform(c, m, 0);
    const float z = u2f(r[rec::S0]);
    const float last = (c.n > 0) ? fetch(c, o, c.n - 1) : z;
    for (uint32_t i = s0 + c.lane; i < s1; i += 64) put(c, m, i, i ? fetch(c, o, i - 1) : z);
    WAVE_SYNC();
    if (c.lane == 0) r[rec::S0] = f2u(last);
}

// SampleDelayNode (Delays.h:177-272). The reference writes the block into the ring and then
// reads ring[(size + w0 - len + i) & mask]; for i >= len that is this block's in[i-len], for
// i < len it is older ring data the block's own writes cannot touch (size >= len + blockSize).
__device__ __forceinline__ void run_sdelay(const Ctx& c, const Member& m, uint32_t s0, uint32_t s1) {
    rup r = c.recs + m.rec * kRecDwords;
    gfp ring = rec_ptr(r, rec::RING_PTR);
    const int size = (int)r[rec::RING_SIZE];
    const int len  = (int)r[rec::RING_LEN];
    int w0 = (int)r[rec::RING_WRITE];
    if (r[rec::RING_RESET]) w0 = 0;
    if (member_nin(c, m) < 1 || size == 0 || ring == nullptr) {
        WAVE_SYNC();
        if (c.lane == 0) { r[rec::RING_RESET] = 0; r[rec::RING_WRITE] = (uint32_t)w0; }
        return zero_fill(c, m, s0, s1);
    }
    const int mask = size - 1;
    const uint32_t o = opnd_uniform(c, m, 0);
    const int readStart = w0 - len;
    for (uint32_t i = s0 + c.lane; i < s1; i += 64) {
        float y;
        if (len >= 0 && (int)i >= len) y = fetch(c, o, i - (uint32_t)len);
        else                           y = ring[(size + readStart + (int)i) & mask];
        put(c, m, i, y);
    }
    WAVE_SYNC();
    for (uint32_t i = s0 + c.lane; i < s1; i += 64) ring[(w0 + (int)i) & mask] = fetch(c, o, i);
    WAVE_SYNC();
    if (c.lane == 0) { r[rec::RING_RESET] = 0; r[rec::RING_WRITE] = (uint32_t)((w0 + (int)c.n) & mask); }
}

// VariableDelayNode (Delays.h:51-169). When the smallest read offset in the block exceeds the
// block length no read can observe a write of this block, so reads then writes are
// sample-parallel; otherwise lane 0 walks the block serially.
__device__ __forceinline__ void run_delay(const Ctx& c, const Member& m, uint32_t s0, uint32_t s1) {
    rup r = c.recs + m.rec * kRecDwords;
    gfp ring = rec_ptr(r, rec::RING_PTR);
    const int size = (int)r[rec::RING_SIZE];
    int w0 = (int)r[rec::RING_WRITE];
    if (r[rec::RING_RESET]) w0 = 0;
    const uint32_t nin = member_nin(c, m);
    if (nin < 3) {
        WAVE_SYNC();
        if (c.lane == 0) { r[rec::RING_RESET] = 0; r[rec::RING_WRITE] = (uint32_t)w0; }
        return zero_fill(c, m, s0, s1);
    }
    const uint32_t oLen = opnd_uniform(c, m, 0), oFb = opnd_uniform(c, m, 1), oX = opnd_uniform(c, m, 2);
    if (size == 0 || ring == nullptr) {   // Delays.h:106-107 copies input 0
        for (uint32_t i = s0 + c.lane; i < s1; i += 64) put(c, m, i, fetch(c, oLen, i));
        WAVE_SYNC();
        if (c.lane == 0) { r[rec::RING_RESET] = 0; r[rec::RING_WRITE] = (uint32_t)w0; }
        return;
    }
    const float fsize = (float)size;
    float mn = FLT_MAX;
    for (uint32_t i = s0 + c.lane; i < s1; i += 64) mn = fminf(mn, clampf(fetch(c, oLen, i), 0.0f, fsize));
    for (int d = 32; d >= 1; d >>= 1) mn = fminf(mn, __shfl_xor(mn, d));
    const bool parallel = (mn >= (float)(c.n + 2)) && ((uint32_t)size >= c.n);
    if (parallel) {
        for (uint32_t i = s0 + c.lane; i < s1; i += 64) {
            int w = w0 + (int)i; if (w >= size) w -= size;       // size >= n: at most one wrap
            const float offset = clampf(fetch(c, oLen, i), 0.0f, fsize);
            const float readFrac = (float)(size + w) - offset;
            const int readLeft = (int)readFrac;
            const int readRight = readLeft + 1;
            const float frac = readFrac - floorf(readFrac);
            const float left = ring[readLeft % size];
            const float right = ring[readRight % size];
            const float out = left + frac * (right - left);
            const float fb = clampf(fetch(c, oFb, i), -1.0f, 1.0f);
            const float in = fetch(c, oX, i) + fb * out;
            put(c, m, i, out);
            lds[m.scratch + i] = in;   // every read of the block precedes every write
        }
        WAVE_SYNC();
        for (uint32_t i = s0 + c.lane; i < s1; i += 64) {
            int w = w0 + (int)i; if (w >= size) w -= size;
            ring[w] = lds[m.scratch + i];
        }
        WAVE_SYNC();
        if (c.lane == 0) {
            int w = w0 + (int)c.n; if (w >= size) w -= size;
            r[rec::RING_RESET] = 0; r[rec::RING_WRITE] = (uint32_t)w;
        }
        return;
    }
    if (c.lane == 0) {
        int w = w0;
        for (uint32_t i = s0; i < s1; ++i) {
            const float offset = clampf(fetch(c, oLen, i), 0.0f, fsize);
            if (offset <= FLT_EPSILON) {
                const float in = fetch(c, oX, i);
                ring[w] = in;
                put(c, m, i, in);
                if (++w >= size) w -= size;
                continue;
            }
            const float readFrac = (float)(size + w) - offset;
            const int readLeft = (int)readFrac;
            const int readRight = readLeft + 1;
            const float frac = readFrac - floorf(readFrac);
            const float left = __builtin_nontemporal_load(&ring[readLeft % size]);
            const float right = __builtin_nontemporal_load(&ring[readRight % size]);
            const float out = left + frac * (right - left);
            const float fb = clampf(fetch(c, oFb, i), -1.0f, 1.0f);
            const float in = fetch(c, oX, i) + fb * out;
            __builtin_nontemporal_store(in, &ring[w]);
            put(c, m, i, out);
            if (++w >= size) w -= size;
        }
        r[rec::RING_RESET] = 0; r[rec::RING_WRITE] = (uint32_t)w;
    }
    WAVE_SYNC();
}

// SampleSeqNode<F,false> (builtins/SampleSeq.h:169-404): k-rate control from in[0][0], two
// cross-fading BufferReader<float>s (detail::GainFade step 0.02/sample) added into a zeroed output.
// Every lane replays the (tiny, uniform) control logic; the fade ramps are produced serially only
// while a reader is still moving (<= 50 frames), the sample reads and the mix are frame-parallel.
__device__ __forceinline__ void run_sampleseq(const Ctx& c, const Member& m, uint32_t s0, uint32_t s1) {
    rup r = c.recs + m.rec * kRecDwords;
    const uint32_t n = c.n;
    const double dur = rec_ld_f64(r, rec::SSQ_DUR);
    double rtDur = rec_ld_f64(r, rec::SSQ_RTDUR);
    float gain[2], target[2], step[2]; uint32_t pos[2], bsz[2]; double start[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        rcup rr = r + rec::SSQ_READER0 + q * rec::SSQ_READER_DWORDS;
        gain[q] = u2f(rr[0]); target[q] = u2f(rr[1]); step[q] = u2f(rr[2]); pos[q] = rr[3];
        start[q] = rec_ld_f64(rr, 4); bsz[q] = rr[6];
    }
    int prev = (int)r[rec::SSQ_PREV], next = (int)r[rec::SSQ_NEXT];
    uint32_t active = r[rec::SSQ_ACTIVE], flags = r[rec::SSQ_FLAGS];
    // mc.sampleseq (mc/SampleSeq.h): same control logic, readers fade with elem::GainFade (8 ms in, 8 ms out)
    const bool mcf = (flags & 4u) != 0u;
    const float inStep = u2f(r[rec::SSQ_READER0 + 7]), outStep = u2f(r[rec::SSQ_READER0 + rec::SSQ_READER_DWORDS + 7]);
    auto resetReaders = [&]() {   // BufferReader::reset (:149-155)
        gain[0] = gain[1] = 0.0f; target[0] = target[1] = 0.0f; start[0] = start[1] = 0.0;
    };
    if (dur != rtDur) { resetReaders(); rtDur = dur; }                                       // :289-296
    const bool bufPending = r[rec::SSQ_BUFPENDING] != 0, seqPending = r[rec::SSQ_SEQPENDING] != 0;
    if (bufPending) { resetReaders(); flags |= 2u; }                                         // :298-304
    if (seqPending) { prev = -1; next = -1; flags |= 1u; }                                   // :306-316
    gcfp buf = rec_ptr(r, rec::SSQ_BUF);
    const uint32_t bufLen = r[rec::SSQ_BUFLEN], seqLen = r[rec::SSQ_SEQLEN];
    gcfp values = rec_ptr(r, rec::SSQ_SEQ) + 2u * seqLen;
    auto evTime = [&](uint32_t k) { gcup p = (gcup)(rec_ptr(r, rec::SSQ_SEQ)) + 2u * k; return rec_ld_f64(p, 0); };
    const bool ok = member_nin(c, m) >= 1 && (flags & 1u) && seqLen > 0 && (flags & 2u) && buf != nullptr && dur > 0.0;
    uint32_t avail[2] = {0u, 0u};
    float g0[2] = {0.0f, 0.0f};
    if (ok) {
        auto setTarget = [&](int q, float g) {
            target[q] = g;
            if (mcf) step[q] = (gain[q] > target[q]) ? outStep : inStep;             // GainFade::fadeIn / fadeOut + updateCurrentStep (GainFade.h:88-118)
            else     step[q] = (g < gain[q]) ? -fabsf(step[q]) : fabsf(step[q]);   // :33-41
        };
        auto toPos = [&](double p, uint32_t outOfRange) { return (p >= 0.0 && p < 4.0e9) ? (uint32_t)p : outOfRange; };
        const double t = (double)fetch(c, opnd_uniform(c, m, 0), 0);                         // :332
        const bool update = (prev < 0 && next < 0) || (prev >= 0 && t <= evTime((uint32_t)prev) + 1e-6)
                         || (next >= 0 && t >= evTime((uint32_t)next) - 1e-6);               // :337-339
        bool aligned = true;                                                                  // :94-103
        if (mcf ? (target[active] > 0.5f) : (fabsf(target[active] - 1.0f) <= 1e-6f)) {        // fade.on(): GainFade.h:102 / SampleSeq.h:53
            const double p = ((t - start[active]) / rtDur) * (double)(bsz[active] - 1u);
            const int np = (fabs(p) < 9.2e18) ? (int)(long long)p : 0;
            const int delta = (int)pos[active] - np;
            aligned = abs(delta) < 16;
        }
        if (update || !aligned) {                                                             // updateEventBoundaries :257-281
            uint32_t lo = 0, hi = seqLen;                                                     // upper_bound(t)
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (evTime(mid) > t) hi = mid; else lo = mid + 1; }
            next = lo < seqLen ? (int)lo : -1;
            if (lo == 0) { prev = -1; setTarget(0, 0.0f); setTarget(1, 0.0f); }
            else {
                prev = (int)lo - 1;
                if (active == 0) setTarget(0, 0.0f); else setTarget(1, 0.0f);
                active = (active + 1u) & 1u;
                if (fabsf(values[prev] - 1.0f) <= 1e-6f) {                                    // engage :75-83
                    const int q = (int)active;
                    const double st = evTime((uint32_t)prev);
                    if (q == 0) { start[0] = st; bsz[0] = bufLen; setTarget(0, 1.0f); } else { start[1] = st; bsz[1] = bufLen; setTarget(1, 1.0f); }
                    const double p = ((t - st) / rtDur) * (double)(bufLen - 1u);
                    const uint32_t np = min(toPos(p, bufLen), bufLen);
                    if (q == 0) pos[0] = np; else pos[1] = np;
                }
            }
        }
        // fade ramps: gains used at frame i, serial only while moving (detail::GainFade::operator() :43-51)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            avail[q] = (pos[q] < bsz[q]) ? min(n, bsz[q] - pos[q]) : 0u;
            float g = gain[q];
            uint32_t k = 0;
            // mono: moves until gain == target; mc: until fpEqual(gain, target), and from then on the sample is scaled by the
            // TARGET while the gain itself stays where it stopped (GainFade::operator(), GainFade.h:43-54)
            for (; k < avail[q] && (mcf ? !(fabsf(g - target[q]) <= 1e-6f) : g != target[q]); ++k) {
                if (c.lane == 0) lds[m.scratch + q * kSlotWords + k] = g;
                g = clampf(g + step[q], 0.0f, 1.0f);
            }
            g0[q] = mcf ? target[q] : g;     // constant from frame k on
            for (uint32_t i = k + c.lane; i < avail[q]; i += 64) lds[m.scratch + q * kSlotWords + i] = g0[q];
            gain[q] = g;
        }
    }
    (void)g0;
    WAVE_SYNC();
    for (uint32_t i = s0 + c.lane; i < s1; i += 64) {
        float acc = 0.0f;                                                                     // :374-377
        if (ok) {
            if (i < avail[0]) acc += buf[pos[0] + i] * lds[m.scratch + i] ;
            if (i < avail[1]) acc += buf[pos[1] + i] * lds[m.scratch + kSlotWords + i];
        }
        put(c, m, i, acc);
    }
    WAVE_SYNC();
    if (c.lane == 0) {
        rec_st_f64(r, rec::SSQ_RTDUR, rtDur);
        r[rec::SSQ_PREV] = (uint32_t)prev; r[rec::SSQ_NEXT] = (uint32_t)next; r[rec::SSQ_ACTIVE] = active; r[rec::SSQ_FLAGS] = flags;
        r[rec::SSQ_BUFPENDING] = 0; r[rec::SSQ_SEQPENDING] = 0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            rup rr = r + rec::SSQ_READER0 + q * rec::SSQ_READER_DWORDS;
            rr[0] = f2u(gain[q]); rr[1] = f2u(target[q]); rr[2] = f2u(step[q]);
            rr[3] = pos[q] + ((mcf && ok) ? n : avail[q]);      // mc: position += numSamples whatever was read (mc/SampleSeq.h:71)
            rec_st_f64(rr, 4, start[q]); rr[6] = bsz[q];
        }
    }
}

// MeterNode (Analyzers.h:23-41): pass-through + block min/max left in the record for Runtime::processQueuedEvents
__device__ __forceinline__ void run_meter(const Ctx& c, const Member& m, uint32_t s0, uint32_t s1) {
    if (member_nin(c, m) < 1) return zero_fill(c, m, s0, s1);
    rup r = c.recs + m.rec * kRecDwords;
    const uint32_t o = opnd_uniform(c, m, 0);
    float mn = FLT_MAX, mx = -FLT_MAX;
    for (uint32_t i = s0 + c.lane; i < s1; i += 64) { const float x = fetch(c, o, i); put(c, m, i, x); mn = fminf(mn, x); mx = fmaxf(mx, x); }
    for (int d = 32; d >= 1; d >>= 1) { mn = fminf(mn, __shfl_xor(mn, d)); mx = fmaxf(mx, __shfl_xor(mx, d)); }
    if (c.lane == 0 && s1 > s0) {
        const uint32_t k = r[rec::EVT_COUNT];
        gup log = (gup)rec_ptr(r, rec::EVT_LOG);
        if (log) { gup e = log + (size_t)(k & r[rec::EVT_LOGMASK]) * 4u; e[0] = k; e[1] = f2u(mn); e[2] = f2u(mx); }
        r[rec::EVT_A] = f2u(mn); r[rec::EVT_B] = f2u(mx); r[rec::EVT_COUNT] = k + 1u;
    }
}

// SnapshotNode (Analyzers.h:83-110): out = x; the value at the last zero -> non-zero transition of the trigger is kept
__device__ __forceinline__ void run_snapshot(const Ctx& c, const Member& m, uint32_t s0, uint32_t s1) {
    if (member_nin(c, m) < 2) return zero_fill(c, m, s0, s1);
    rup r = c.recs + m.rec * kRecDwords;
    const uint32_t oL = opnd_uniform(c, m, 0), oX = opnd_uniform(c, m, 1);
    const float z = u2f(r[rec::EVT_A]);
    int last = -1; uint32_t cnt = 0;
    for (uint32_t i = s0 + c.lane; i < s1; i += 64) {
        const float l = fetch(c, oL, i), prev = i == 0u ? z : fetch(c, oL, i - 1u);
        put(c, m, i, fetch(c, oX, i));
        if (fabsf(prev) <= FLT_EPSILON && l > FLT_EPSILON) { last = (int)i; ++cnt; }
    }
    for (int d = 32; d >= 1; d >>= 1) { last = max(last, __shfl_xor(last, d)); cnt += __shfl_xor(cnt, d); }
    if (c.lane == 0 && s1 > s0) {
        const uint32_t blk = r[rec::EVT_BLK];
        if (last >= 0) {
            const float v = fetch(c, oX, (uint32_t)last);
            gup log = (gup)rec_ptr(r, rec::EVT_LOG);
            const uint32_t k = r[rec::EVT_LOGN];
            if (log) { gup e = log + (size_t)(k & r[rec::EVT_LOGMASK]) * 4u; e[0] = blk; e[1] = f2u(v); e[2] = cnt; }
            r[rec::EVT_LOGN] = k + 1u;
            r[rec::EVT_B] = f2u(v); r[rec::EVT_COUNT] = r[rec::EVT_COUNT] + cnt;
        }
        r[rec::EVT_BLK] = blk + 1u;
        r[rec::EVT_A] = f2u(fetch(c, oL, s1 - 1u));
    }
}

// ScopeNode (Analyzers.h:175-190) + MultiChannelRingBuffer::write (:34-59): pass-through of input 0, up to four
// inputs appended to the node's device ring; an overrun nudges the read position past the write position.
template <uint32_t MaxCh = 4u>
__device__ __forceinline__ void run_scope(const Ctx& c, const Member& m, uint32_t s0, uint32_t s1) {
    const uint32_t nin = member_nin(c, m);
    if (nin < 1) return zero_fill(c, m, s0, s1);
    rup r = c.recs + m.rec * kRecDwords;
    gfp ring = rec_ptr(r, rec::SCP_RING);
    // the reference's ring positions (mod 8192); the device ring holds SCP_MASK + 1 frames per channel — the same 8192, or a whole
    // relay window's history (engine.cpp, event_replay.h) — and is addressed by the count of frames written so far
    const uint32_t cap = 8192u, mask = cap - 1u, n = s1 - s0;
    const uint32_t w = r[rec::SCP_WRITE], rd = r[rec::SCP_READ];
    const uint32_t hmask = UNI(r[rec::SCP_MASK]), abs0 = UNI(r[rec::SCP_ABS]);
    const size_t hcap = (size_t)hmask + 1u;
    const uint32_t chans = min(nin, MaxCh);
    for (uint32_t ch = 0; ch < chans; ++ch) {
        const uint32_t o = opnd_uniform(c, m, ch);
        for (uint32_t i = s0 + c.lane; i < s1; i += 64) {
            const float x = fetch(c, o, i);
            if (ch == 0u) put(c, m, i, x);
            if (ring) ring[ch * hcap + ((abs0 + i - s0) & hmask)] = x;
        }
    }
    if (c.lane == 0 && n > 0) {
        const uint32_t freeSlots = rd > w ? rd - w : cap - (w - rd);
        const uint32_t nw = (w + n) & mask;
        r[rec::SCP_WRITE] = nw;
        r[rec::SCP_READ] = n >= freeSlots ? ((nw + 1u) & mask) : rd;
        r[rec::SCP_ABS] = abs0 + n;
    }
}

// FFTNode::process (wasm/FFT.h:74-90): pass-through of input 0, which is also appended to the node's ONE-channel ring — the scope's
// ring write at one channel (no input: zeros out, nothing written). The transform happens at the relay (fft_frames.hip).
__device__ __forceinline__ void run_fft(const Ctx& c, const Member& m, uint32_t s0, uint32_t s1) { run_scope<1u>(c, m, s0, s1); }

// The block's entry of a capture ring's per-block log (device.h CAP_LOGMASK; `behind` = floats of the ring's channels, the log sits
// after them): entered by ONE lane at the end of every block the node renders.
__device__ __forceinline__ void capture_log(rup r, gfp ring, size_t behind, uint32_t abs0, uint32_t fell) {
    const uint32_t blk = r[rec::CAP_BLK], lm = r[rec::CAP_LOGMASK];
    if (lm && ring) { gup e = (gup)(ring + behind) + (size_t)(blk & lm) * 4u; e[0] = blk; e[1] = abs0; e[2] = fell; e[3] = 0u; }
    r[rec::CAP_BLK] = blk + 1u;
}

// CaptureNode (Capture.h:21-58): pass-through of input 1; while the gate (input 0) is non-zero its samples are recorded. The
// reference collects them in a 128-frame scratch it appends to its ring when full or when the gate falls (MultiChannelRingBuffer
// ::write, an overrun nudging the read position); here the scratch IS the ring ahead of the write position — the k-th recorded
// sample lands at (write + scratch + k), written frame-parallel — and the wave replays the flushes on the two ballot masks so
// that the positions the host relay sees (engine.cpp, processQueuedEvents) move exactly when the reference's do.
// MCCaptureNode (builtins/mc/Capture.h:39-105): output channel ch passes input ch + 1 through; the record of channel 0 also does
// the recording for ALL capture channels. The reference walks the block sample by sample with two markers — writeStop = the last
// gated sample + 1, writeStart = the last sample where the gate ROSE while on — and hands [writeStart, writeStop) of every input
// to the multi-channel ring at each FALLING gate (Change.h: any decrease) and at the end of the block. Here the gate's 64-frame
// ballots give the same markers segment by segment (a segment = the frames between two falling edges): highest set bit of
// (rising & gated), highest set bit of gated.
__device__ __forceinline__ void run_mccapture(const Ctx& c, const Member& m, uint32_t s0, uint32_t s1) {
    const uint32_t nin = member_nin(c, m);
    if (nin < 2) return zero_fill(c, m, s0, s1);                          // Capture.h:48-54 (no recording either)
    rup r = c.recs + m.rec * kRecDwords;
    const uint32_t ch = UNI(r[rec::CAP_CH]);
    if (ch + 1u < nin) { const uint32_t oX = opnd_uniform(c, m, ch + 1u); for (uint32_t i = s0 + c.lane; i < s1; i += 64u) put(c, m, i, fetch(c, oX, i)); }
    else zero_fill(c, m, s0, s1);
    if (ch != 0u || s1 <= s0) return;
    gfp ring = rec_ptr(r, rec::CAP_RING);
    // the reference's ring positions (mod cap = bitceil(sr)); the device ring holds CAP_MASK + 1 frames per channel — the same, or a
    // whole relay window's takes (device.h CAP_ABS) — and is addressed by the count of frames handed over so far
    const uint32_t hmask = UNI(r[rec::CAP_MASK]), mask = UNI(r[rec::CAP_REFMASK]), cap = mask + 1u, ringChans = UNI(r[rec::CAP_CHANS]), chans = min(ringChans, nin - 1u);
    const size_t hcap = (size_t)hmask + 1u;
    const uint32_t oG = opnd_uniform(c, m, 0);
    uint32_t w = UNI(r[rec::CAP_WRITE]), rd = UNI(r[rec::CAP_READ]), ready = UNI(r[rec::CAP_READY]), abs0 = UNI(r[rec::CAP_ABS]), fell = 0u;
    float last = u2f(UNI(r[rec::CAP_CHANGE]));
    uint32_t wStart = 0u, wStop = 0u;
    auto flush = [&](uint32_t a, uint32_t b) {                            // MultiChannelRingBuffer::write(inputData + 1, numIns - 1, b - a, a)
        const uint32_t ns = b - a;
        const uint32_t freeSlots = rd > w ? rd - w : cap - (w - rd);
        const uint32_t nw = (w + ns) & mask;
        if (ns >= freeSlots) rd = (nw + 1u) & mask;
        if (ring)
            for (uint32_t k = 0; k < chans; ++k) {
                const uint32_t oK = opnd_uniform(c, m, k + 1u);
                for (uint32_t j = c.lane; j < ns; j += 64u) ring[(size_t)k * hcap + ((abs0 + j) & hmask)] = fetch(c, oK, a + j);
            }
        w = nw; abs0 += ns;
    };
    for (uint32_t base = s0; base < s1; base += 64u) {
        const uint32_t i = base + c.lane;
        const bool on = i < s1;
        const float g = on ? fetch(c, oG, i) : 0.0f, prev = !on ? 0.0f : (i == s0 ? last : fetch(c, oG, i - 1u));
        const unsigned long long valid = __ballot(on);
        const unsigned long long gm = __ballot(on && g != 0.0f), rm = __ballot(on && (g - prev) > 0.0f);
        unsigned long long fm = __ballot(on && (g - prev) < 0.0f);
        uint32_t pos = 0u;
        for (;;) {
            const unsigned long long fe = pos < 64u ? (fm >> pos) << pos : 0ull;           // falling edges at or after `pos`
            const uint32_t end = fe ? (uint32_t)__builtin_ctzll(fe) : 64u;
            const unsigned long long lowEnd = end >= 64u ? ~0ull : ((1ull << end) - 1ull), lowPos = pos >= 64u ? ~0ull : ((1ull << pos) - 1ull);
            const unsigned long long seg = lowEnd & ~lowPos & valid;                         // frames [pos, end) of this chunk
            const unsigned long long gs = gm & seg, rs = rm & gm & seg;
            if (rs) wStart = base + 63u - (uint32_t)__builtin_clzll(rs);
            if (gs) wStop = base + 64u - (uint32_t)__builtin_clzll(gs);
            if (!fe) break;
            flush(wStart, wStop);                                                            // the gate fell at frame `end`: hand over, then that frame's own gate counts again
            ready = 1u; fell = 1u; wStart = 0u; wStop = 0u;
            fm &= ~(1ull << end);
            pos = end;
        }
    }
    if (wStop > wStart) flush(wStart, wStop);
    WAVE_SYNC();
    if (c.lane == 0) {
        r[rec::CAP_WRITE] = w; r[rec::CAP_READ] = rd; r[rec::CAP_READY] = ready; r[rec::CAP_ABS] = abs0;
        r[rec::CAP_CHANGE] = f2u(fetch(c, oG, s1 - 1u));
        capture_log(r, ring, (size_t)ringChans * hcap, abs0, fell);
    }
}

__device__ __forceinline__ void run_capture(const Ctx& c, const Member& m, uint32_t s0, uint32_t s1) {
    if (UNI(c.recs[m.rec * kRecDwords + rec::CAP_CHANS]) != 0u) return run_mccapture(c, m, s0, s1);
    if (member_nin(c, m) < 2) return zero_fill(c, m, s0, s1);
    rup r = c.recs + m.rec * kRecDwords;
    gfp ring = rec_ptr(r, rec::CAP_RING);
    // (positions mod cap = bitceil(sr) as the reference keeps them; the device ring of CAP_MASK + 1 frames is addressed by CAP_ABS)
    const uint32_t hmask = r[rec::CAP_MASK], mask = r[rec::CAP_REFMASK], cap = mask + 1u;
    const uint32_t oG = opnd_uniform(c, m, 0), oX = opnd_uniform(c, m, 1);
    uint32_t w = r[rec::CAP_WRITE], rd = r[rec::CAP_READ], s = r[rec::CAP_SCRATCH], ready = r[rec::CAP_READY], abs0 = r[rec::CAP_ABS], fell = 0u;
    const float z = u2f(r[rec::CAP_CHANGE]);
    uint32_t head = abs0 + s;                                         // where the next recorded sample goes
    for (uint32_t base = s0; base < s1; base += 64u) {
        const uint32_t i = base + c.lane;
        const bool on = i < s1;
        const float g = on ? fetch(c, oG, i) : 0.0f, prev = !on ? 0.0f : (i == 0u ? z : fetch(c, oG, i - 1u));
        const float x = on ? fetch(c, oX, i) : 0.0f;
        if (on) put(c, m, i, x);
        const bool rec_ = on && g != 0.0f;                            // static_cast<bool>(gate)
        const uint64_t gm = __ballot(rec_), fm = __ballot(on && (g - prev) < 0.0f);   // Change.h: sign of the difference < -0.5
        if (rec_ && ring) ring[(head + (uint32_t)__popcll(gm & ((1ull << c.lane) - 1ull))) & hmask] = x;
        const uint32_t cnt = (uint32_t)__popcll(gm);
        head += cnt;
        if (fm != 0ull) fell = 1u;
        if (fm == 0ull && s + cnt < 128u) { s += cnt; continue; }   // no flush inside these 64 frames
        const uint32_t nf = min(64u, s1 - base);
        for (uint32_t j = 0; j < nf; ++j) {
            const bool falling = (fm >> j) & 1ull;
            if (falling || s >= 128u) {
                const uint32_t freeSlots = rd > w ? rd - w : cap - (w - rd);
                const uint32_t nw = (w + s) & mask;
                if (s >= freeSlots) rd = (nw + 1u) & mask;
                w = nw; abs0 += s; s = 0u;
                if (falling) ready = 1u;
            }
            if ((gm >> j) & 1ull) ++s;
        }
    }
    if (c.lane == 0 && s1 > s0) {
        r[rec::CAP_WRITE] = w; r[rec::CAP_READ] = rd; r[rec::CAP_SCRATCH] = s; r[rec::CAP_READY] = ready; r[rec::CAP_ABS] = abs0;
        r[rec::CAP_CHANGE] = f2u(fetch(c, oG, s1 - 1u));
        capture_log(r, ring, (size_t)hmask + 1u, abs0, fell);
    }
}

// ---- lane-per-node recurrences ---------------------------------------------------------------
// Entered by lanes [0, count) of the task's wave; `m` is that lane's node. Every operand of a
// chain lives in LDS (the planner imports HBM operands first): a block buffer (16-byte aligned,
// streamed 8 samples at a time with two ds_read_b128) or a broadcast cell (read once). Which
// operands are cells is a property of the TASK (the planner groups chain members by that mask),
// so the choice is a scalar branch.
constexpr int CH = 8;

// A streamed operand / output of a specialised kernel is named by its BYTE OFFSET from the arena base (Ctx::hbm0): the loops
// below reach it through one buffer descriptor over the whole arena, `goff` in the VGPR offset (each lane its own node's
// buffer), the position inside the block in the scalar offset and the instruction's immediate — no address arithmetic per
// access, none per group of frames (r02's loops formed a 64-bit pointer per 16-byte access: ~100 of their 420 instructions
// per 128 frames).
struct SIn { uint32_t base; float cval; gfp arena; uint32_t goff; bool isG; uint32_t boff; bool isS; };   // isG: the operand streams from the HBM arena (specialised kernels only);
                                                               // boff / isS: the buffer's byte offset inside its slice, slice of the stream ring (else of the block's arena)
struct SOut { uint32_t lds; gfp arena; uint32_t goff; bool isG; uint32_t cnt; Deferred* defer; uint32_t boff; bool isS; bool quad; };   // isG: the recurrence writes its block straight to the arena;
                                                               // cnt: members of the task (specialised kernels; 64 = every lane stores); defer: Ctx::defer
                                                               // quad: member m of the task sits in lanes 4m .. 4m+3 (chain_skew.h), not in lane m
constexpr uint32_t kCntQuad = 0x80000000u;                     // Member::cnt of a task laid out in quads (set by spec_stateful, read by sout_of)
// (isG is a separate flag, not a null test: the compiler cannot prove arena base + offset non-null, the flag folds)

__device__ __forceinline__ SIn sin_const(float v) { SIn s; s.base = 0u; s.cval = v; s.arena = (gfp)nullptr; s.goff = 0u; s.isG = false; s.boff = 0u; s.isS = false; return s; }
__device__ __forceinline__ SIn sin_lds(uint32_t w) { SIn s; s.base = w; s.cval = 0.0f; s.arena = (gfp)nullptr; s.goff = 0u; s.isG = false; s.boff = 0u; s.isS = false; return s; }
__device__ __forceinline__ float sin_at(const SIn& s, uint32_t t) {   // per-frame access (tails, rare shapes)
    return s.isG ? ((gcfp)((const char __attribute__((address_space(1)))*)s.arena + s.goff))[t] : lds[s.base + t];
}
__device__ __forceinline__ SIn sin_of(const Ctx& c, uint32_t o) {
    const uint32_t kind = o & kOpKindMask, v = o & kOpValMask;
    SIn s;
    s.arena = (gfp)nullptr; s.goff = 0u; s.isG = false; s.boff = 0u; s.isS = false;
    if (kind == kOpLds)        { s.base = v; s.cval = 0.0f; }
    else if (kind == kOpConst) { s.base = v; s.cval = lds[v]; }
#ifdef ELEMHIP_SPEC
    else if (kind == kOpHbm)   { s.base = 0u; s.cval = 0.0f; s.arena = c.hbm0; s.goff = hbm_off(c, v); s.isG = true;
                                 s.boff = (v & ~(uint32_t)kOpStream) * c.stride * 4u; s.isS = (v & kOpStream) != 0u; }
#endif
    else                       { s.base = 0u; s.cval = 0.0f; }   // zero operand (mask bit set by the planner)
    return s;
}
__device__ __forceinline__ SOut sout_of(const Ctx& c, const Member& m) {
    SOut o;
    o.lds = m.outLds; o.arena = c.hbm0; o.goff = 0u; o.isG = false; o.cnt = 64u; o.defer = c.defer; o.boff = 0u; o.isS = false; o.quad = false;
#ifdef ELEMHIP_SPEC
    if (m.gdirect) { o.isG = true; o.goff = hbm_off(c, m.outHbm); o.boff = (m.outHbm & ~(uint32_t)kOpStream) * c.stride * 4u; o.isS = (m.outHbm & kOpStream) != 0u; }
    o.cnt = m.cnt & ~kCntQuad; o.quad = (m.cnt & kCntQuad) != 0u;
#endif
    return o;
}
__device__ __forceinline__ SOut sout_lds(uint32_t w) { SOut o; o.lds = w; o.arena = (gfp)nullptr; o.goff = 0u; o.isG = false; o.cnt = 64u; o.defer = nullptr; o.boff = 0u; o.isS = false; o.quad = false; return o; }
__device__ __forceinline__ void sout_put(const SOut& o, uint32_t t, float y) {   // per-frame store (tails, rare shapes)
    if (o.isG) ((gfp)((char __attribute__((address_space(1)))*)o.arena + o.goff))[t] = y; else lds[o.lds + t] = y;
}

// A recurrence's step together with the registers it carries from frame to frame. The step lambda captures them by reference;
// `each(g)` calls g(reg) for every one of them, so that a loop can move the state between lanes (chain_loop_q does, behind the
// last group of a block). The other loops only call the step. SHORT marks a step of a couple of VALU ops and no streamed operand:
// chain_loop_q writes such a loop out span by span (a few KB of code) and so spares it the counter and back edge, one scalar
// instruction per 16-frame group of a loop that has 34.
template <typename F, typename E, bool SHORT = false>
struct ChainStep {
    F f; E each;
    static constexpr bool kShort = SHORT;
    template <int N> __device__ __forceinline__ float operator()(const float (&x)[N]) { return f(x); }
};
template <bool SHORT = false, typename F, typename E>
__device__ __forceinline__ ChainStep<F, E, SHORT> chain_step(F f, E each) { return ChainStep<F, E, SHORT>{f, each}; }
template <typename T> struct IsChainStep { static constexpr bool value = false, kShort = false; };
template <typename F, typename E, bool SHORT> struct IsChainStep<ChainStep<F, E, SHORT>> { static constexpr bool value = true, kShort = SHORT; };
template <typename T> struct IsChainStep<T&> : IsChainStep<T> {};
template <typename T> struct IsChainStep<const T> : IsChainStep<T> {};

// Chunked chain with the broadcast-cell mask CM known at compile time: cell operands are plain
// loop-invariant scalars (no loads, no register copies), buffer operands are streamed with two
// ds_read_b128 per 8 frames, one chunk ahead of the dependent arithmetic (ping-pong registers).
// `step(x[NIN]) -> y` carries the node state by reference.
#ifdef ELEMHIP_SPEC
// Specialised kernels: 16 frames per group, written to the instruction count (a lone wavefront issues one instruction
// every ~4 cycles whatever it is, an LDS access costs it 12-50 and suffers from the island's other LDS traffic). Per frame
// only the recurrence's own VALU ops; per 16 frames four 16-byte loads per streamed operand — from the HBM arena
// (global_load_dwordx4, L2-resident, DEPTH groups ahead: vector loads return in order, so vmcnt(N) waits for exactly the
// group that is due) or from LDS — and four 16-byte stores of the results. Every lane runs the whole chain with its own
// member's addresses (lanes beyond the task's member count repeat the last member): a partial EXEC mask costs ~1 cycle
// per VALU op on a lone wave, and the per-lane form needs no uniformity argument when a task carries several nodes.
constexpr int CHG = 16;
template <int I> struct IntC { static constexpr int value = I; };
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) { f(IntC<I>{}); static_for<I + 1, N>(f); }
}
// The four 16-byte stores of a 16-frame group, with EXEC cut down to the task's member lanes for just these instructions (one
// asm statement: no branch, no compiler-visible EXEC change). A store instruction moves its active lanes' data through the
// CU's shared vector-memory data path: with all 64 lanes enabled (r02: the extra lanes' offsets out of range, dropped at the
// far end) a lone recurrence wave paid ~0.5 k cycles per block for its stores when alone on the CU and ~2.2 k beside the
// island's seven other waves (profiles/r03/ab_chain_loops.txt). The compiler does not count these stores: its own vmcnt
// waits (for the operand loads) only become more conservative by them; the publishing code waits with explicit counts.
// chain_store_group_lds: the same for an output block that lives in LDS (ds_write_b128, byte address per lane).
// OFF: byte offset of the group inside the span (immediate); voff: the lane's buffer offset; soff: the span's offset.
typedef float v4f_ __attribute__((ext_vector_type(4)));
template <int OFF>
__device__ __forceinline__ void chain_store_group(const v4f_& a0, const v4f_& a1, const v4f_& a2, const v4f_& a3, uint32_t voff,
                                                  __amdgpu_buffer_rsrc_t rsrc, uint32_t soff, unsigned long long mask) {
    static_assert(OFF >= 0 && OFF + 48 < 4096, "12-bit immediate");
    unsigned long long saved;
    asm volatile("s_mov_b64 %0, exec\n\t"
                 "s_mov_b64 exec, %8\n\t"
                 "buffer_store_dwordx4 %1, %5, %6, %7 offen offset:%c9\n\t"
                 "buffer_store_dwordx4 %2, %5, %6, %7 offen offset:%c10\n\t"
                 "buffer_store_dwordx4 %3, %5, %6, %7 offen offset:%c11\n\t"
                 "buffer_store_dwordx4 %4, %5, %6, %7 offen offset:%c12\n\t"
                 "s_mov_b64 exec, %0\n\t"
                 "s_nop 0"
                 : "=&s"(saved)
                 : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(voff), "s"(rsrc), "s"(soff), "s"(mask),
                   "i"(OFF), "i"(OFF + 16), "i"(OFF + 32), "i"(OFF + 48)
                 : "memory");
}
// ---- the quad-skewed form of the loop (chain_skew.h): one 16-byte store per lane and group ---------------------------------
// chain_store_window / chain_store_window_lds: the stores of a window of W groups (chain_skew.h) — every lane of a quad its own four
// frames of each — with EXEC cut to the task's 4 * count member lanes exactly as chain_store_group does it, ONE switch for the W of
// them. EXEC is saved and restored, not assumed to be all ones. voff already carries the lane's place inside a group; OFF is the
// byte offset of the window's first group inside the span, group i of the window lies 64 * i bytes behind it.
// Operands of the one asm statement: %0 the saved EXEC, %1 the mask, then the W pieces, their W immediates, and the address operands.
#define CHAIN_WST_G(D, I, V, R, S) "buffer_store_dwordx4 %" #D ", %" #V ", %" #R ", %" #S " offen offset:%c" #I "\n\t"
#define CHAIN_WST_L(D, I, V) "ds_write_b128 %" #V ", %" #D " offset:%c" #I "\n\t"
#define CHAIN_W1(X, ...) X(2, 3, __VA_ARGS__)
#define CHAIN_W2(X, ...) X(2, 4, __VA_ARGS__) X(3, 5, __VA_ARGS__)
#define CHAIN_W4(X, ...) X(2, 6, __VA_ARGS__) X(3, 7, __VA_ARGS__) X(4, 8, __VA_ARGS__) X(5, 9, __VA_ARGS__)
#define CHAIN_W8(X, ...) X(2, 10, __VA_ARGS__) X(3, 11, __VA_ARGS__) X(4, 12, __VA_ARGS__) X(5, 13, __VA_ARGS__) \
                         X(6, 14, __VA_ARGS__) X(7, 15, __VA_ARGS__) X(8, 16, __VA_ARGS__) X(9, 17, __VA_ARGS__)
#define CHAIN_A1 "v"(a[0]), "i"(OFF)
#define CHAIN_A2 "v"(a[0]), "v"(a[1]), "i"(OFF), "i"(OFF + 64)
#define CHAIN_A4 "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "i"(OFF), "i"(OFF + 64), "i"(OFF + 128), "i"(OFF + 192)
#define CHAIN_A8 "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]), \
                 "i"(OFF), "i"(OFF + 64), "i"(OFF + 128), "i"(OFF + 192), "i"(OFF + 256), "i"(OFF + 320), "i"(OFF + 384), "i"(OFF + 448)
#define CHAIN_WSTORE(STORES, PIECES, ...) \
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %1\n\t" STORES "s_mov_b64 exec, %0\n\ts_nop 0" \
                 : "=&s"(saved) : "s"(mask), PIECES, __VA_ARGS__ : "memory")
template <int OFF, int W>
__device__ __forceinline__ void chain_store_window(const v4f_ (&a)[W], uint32_t voff, __amdgpu_buffer_rsrc_t rsrc, uint32_t soff, unsigned long long mask) {
    static_assert(W == 1 || W == 2 || W == 4 || W == 8, "the window sizes that are written out");
    static_assert(OFF >= 0 && OFF + 64 * (W - 1) < 4096, "12-bit immediate");
    unsigned long long saved;
    if constexpr (W == 1) CHAIN_WSTORE(CHAIN_W1(CHAIN_WST_G, 4, 5, 6), CHAIN_A1, "v"(voff), "s"(rsrc), "s"(soff));
    else if constexpr (W == 2) CHAIN_WSTORE(CHAIN_W2(CHAIN_WST_G, 6, 7, 8), CHAIN_A2, "v"(voff), "s"(rsrc), "s"(soff));
    else if constexpr (W == 4) CHAIN_WSTORE(CHAIN_W4(CHAIN_WST_G, 10, 11, 12), CHAIN_A4, "v"(voff), "s"(rsrc), "s"(soff));
    else CHAIN_WSTORE(CHAIN_W8(CHAIN_WST_G, 18, 19, 20), CHAIN_A8, "v"(voff), "s"(rsrc), "s"(soff));
}
template <int OFF, int W>
__device__ __forceinline__ void chain_store_window_lds(const v4f_ (&a)[W], uint32_t addr, unsigned long long mask) {
    static_assert(W == 1 || W == 2 || W == 4 || W == 8, "the window sizes that are written out");
    static_assert(OFF >= 0 && OFF + 64 * (W - 1) < 65536, "16-bit immediate");
    unsigned long long saved;
    if constexpr (W == 1) CHAIN_WSTORE(CHAIN_W1(CHAIN_WST_L, 4), CHAIN_A1, "v"(addr));
    else if constexpr (W == 2) CHAIN_WSTORE(CHAIN_W2(CHAIN_WST_L, 6), CHAIN_A2, "v"(addr));
    else if constexpr (W == 4) CHAIN_WSTORE(CHAIN_W4(CHAIN_WST_L, 10), CHAIN_A4, "v"(addr));
    else CHAIN_WSTORE(CHAIN_W8(CHAIN_WST_L, 18), CHAIN_A8, "v"(addr));
}
#undef CHAIN_WSTORE
#undef CHAIN_A8
#undef CHAIN_A4
#undef CHAIN_A2
#undef CHAIN_A1
#undef CHAIN_W8
#undef CHAIN_W4
#undef CHAIN_W2
#undef CHAIN_W1
#undef CHAIN_WST_L
#undef CHAIN_WST_G
// every lane takes the register of chain_skew::state_lane(lane), its quad's first lane (one v_mov_b32 with a DPP quad permute; all
// 64 lanes are enabled)
__device__ __forceinline__ void quad_first(uint32_t& v) { v = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, chain_skew::kStateQuadPerm, 0xF, 0xF, false); }
__device__ __forceinline__ void quad_first(float& v) { uint32_t u = f2u(v); quad_first(u); v = u2f(u); }

// Taken by chain_loop_d when the task is laid out in quads, every streamed operand comes from the arena and the block is the
// kernel's own (a multiple of the span). Per lane the instruction stream of a steady group is the unskewed loop's minus three of
// its four stores; the lane's skew lives in its VGPR offsets alone. Group 0 of a block (the head) is peeled: its steps are
// predicated per lane, its loads clamped into the operand's block buffer — global loads are not range-checked by anything. Behind
// the last group every frame of the block is stored and the lane of skew 0 holds the member's final state; the three lagging lanes
// of its quad take that state from it (quad_first) where they used to run up to 12 more predicated steps on three more clamped
// loads per operand (~50 issue slots and 3 memory instructions per block of the lone wave, for bits the quad already held). The
// last span issues no loads at all.
// A steady group is written to the instruction count: the chain's own VALU ops, four loads per streamed operand, ONE wait, ONE
// store, and the EXEC switch of the stores shared by the W groups of a window (chain_skew.h) — for a one-pole 32 + 4 + 1 + 1 + 4 / W.
// tools/chain_loop_census.py counts it in the code object; tests/test_chain_loop_census.py holds it there.
template <int NIN, uint32_t CM, int DEPTH, typename Step>
__device__ __forceinline__ void chain_loop_q(const SIn (&in)[NIN], const SOut out, Step&& step) {
    constexpr int NS0 = NIN - __builtin_popcount(CM & ((1u << NIN) - 1u));
    constexpr int NS = NS0 > 0 ? NS0 : 1;
    constexpr uint32_t n = ELEMHIP_SPEC_BLOCK, span = (uint32_t)(DEPTH * CHG);
    static_assert(n % span == 0u && n >= span, "whole spans only");
    static_assert(CHG == (int)chain_skew::kGroup, "chain_skew.h is written for 16-frame groups");
    constexpr int W = (int)chain_skew::window(NS0 > 0, (uint32_t)DEPTH);   // groups per store window
    static_assert(chain_skew::window_fits((uint32_t)W, (uint32_t)DEPTH), "a window never leaves its span");
    const uint32_t skew = chain_skew::lane_skew(opaque_lane(), out.cnt);
    gfp arena = out.arena;
#pragma unroll
    for (int k = 0; k < NIN; ++k) if (in[k].isG) arena = in[k].arena;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((float*)arena, 0, 0x7FFFFFFF, 0x00020000);
    uint32_t ooff = (out.isG ? out.goff : (out.lds << 2)) + chain_skew::store_bias(skew);
    uint32_t ioff[NIN];
#pragma unroll
    for (int k = 0; k < NIN; ++k) ioff[k] = in[k].goff + chain_skew::load_bias(skew);
#define CHAIN_OPAQUE_OFFSETS() do { asm volatile("" : "+v"(ooff)); _Pragma("unroll") for (int k_ = 0; k_ < NIN; ++k_) asm volatile("" : "+v"(ioff[k_])); } while (0)
    const unsigned long long smask = chain_skew::store_mask(out.cnt);
    typedef const char __attribute__((address_space(1)))* gccp;
    // a steady group: D-th of the span at byte offset soff of the block (never group 0)
    auto load = [&](uint32_t soff, auto Dc, v4f (&x)[NS][CHG / 4]) {
        constexpr int D = decltype(Dc)::value;
        int s_ = 0;
#pragma unroll
        for (int k = 0; k < NIN; ++k) {
            if (!((CM >> k) & 1u)) {
#pragma unroll
                for (int q = 0; q < CHG / 4; ++q) {
                    x[s_][q] = *(gcv4)((gccp)arena + ioff[k] + soff + (D * CHG * 4 + 16 * q + chain_skew::kLoadImmBias));
                }
                ++s_;
            }
        }
    };
    // group G (0: the head's), pieces [0, NQ): every piece at its own clamped offset
    auto load_edge = [&](uint32_t G, auto NQc, v4f (&x)[NS][CHG / 4]) {
        constexpr int NQ = decltype(NQc)::value;
        int s_ = 0;
#pragma unroll
        for (int k = 0; k < NIN; ++k) {
            if (!((CM >> k) & 1u)) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    x[s_][q] = *(gcv4)((gccp)arena + (in[k].goff + chain_skew::load_offset(G, (uint32_t)q, skew, n)));
                }
                ++s_;
            }
        }
    };
    // One wait per group, for whichever of its loads was issued last (vector loads return in order; the compiler orders the four
    // loads of a group as it likes): an empty statement that READS every piece of the group, and a scheduling barrier behind it so
    // that no step of the group moves above it. (Until r09 the statement made the last piece opaque and nothing more: the chain's
    // first steps, which read the first piece, were scheduled in front of it and the loop waited piece by piece, three times per
    // group. The statement has no outputs: the compiler pads an asm output that the next VALU instruction touches with a wait state.)
    auto wait_group = [&](const v4f (&x)[NS][CHG / 4]) {
        static_assert(CHG == 16 && NS <= 3, "four pieces per stream, at most three streams in one statement");
        if constexpr (NS0 == 1) asm volatile("" : : "v"(x[0][0]), "v"(x[0][1]), "v"(x[0][2]), "v"(x[0][3]));
        else if constexpr (NS0 == 2) asm volatile("" : : "v"(x[0][0]), "v"(x[0][1]), "v"(x[0][2]), "v"(x[0][3]), "v"(x[1][0]), "v"(x[1][1]), "v"(x[1][2]), "v"(x[1][3]));
        else if constexpr (NS0 == 3) asm volatile("" : : "v"(x[0][0]), "v"(x[0][1]), "v"(x[0][2]), "v"(x[0][3]), "v"(x[1][0]), "v"(x[1][1]), "v"(x[1][2]), "v"(x[1][3]),
                                                         "v"(x[2][0]), "v"(x[2][1]), "v"(x[2][2]), "v"(x[2][3]));
        if constexpr (NS0 > 0) __builtin_amdgcn_sched_barrier(0);
    };
    auto operands = [&](const v4f (&x)[NS][CHG / 4], int j, float (&xs)[NIN]) {
        int s_ = 0;
#pragma unroll
        for (int k = 0; k < NIN; ++k) {
            if ((CM >> k) & 1u) xs[k] = in[k].cval;
            else xs[k] = x[s_++][j / 4][j % 4];
        }
    };
    // The 16 steps of a group; returns the lane's piece of it, its last four results. HEAD: group 0 of the block — a lane of skew k
    // holds for its first 4k steps
    auto run = [&](v4f (&x)[NS][CHG / 4], auto Hc) {
        constexpr bool HEAD = decltype(Hc)::value != 0;
        float y[CHG];
        wait_group(x);
#pragma unroll
        for (int j = 0; j < CHG; ++j) {
            float xs[NIN];
            operands(x, j, xs);
            if constexpr (HEAD) { y[j] = 0.0f; if (chain_skew::head_active(skew, (uint32_t)j)) y[j] = step(xs); }
            else y[j] = step(xs);
        }
        v4f a;
        a.x = y[CHG - 4]; a.y = y[CHG - 3]; a.z = y[CHG - 2]; a.w = y[CHG - 1];
        return a;
    };
    v4f X[DEPTH][NS][CHG / 4];
    CHAIN_OPAQUE_OFFSETS();
    if constexpr (NS0 > 0) {
        load_edge(0u, IntC<CHG / 4>{}, X[0]);
        static_for<1, DEPTH>([&](auto Dc) { load(0u, Dc, X[decltype(Dc)::value]); });
        take_deferred<DEPTH * NS0 * (CHG / 4)>(out.defer);   // the previous block is published under this block's first loads
    } else take_deferred<0>(out.defer);
    auto span_body = [&](uint32_t soff, auto Hc, auto Lc) {
        constexpr bool HEAD = decltype(Hc)::value != 0, LAST = decltype(Lc)::value != 0;
        // (without loads there is no offset arithmetic to keep in the immediates, and an empty statement that DEFINES ooff right in
        //  front of the store statement that reads it draws a wait-state pad from the compiler)
        if constexpr (NS0 > 0) CHAIN_OPAQUE_OFFSETS();
        v4f A[W];                                            // the pieces of the open window
        static_for<0, DEPTH>([&](auto Dc) {
            constexpr int D = decltype(Dc)::value;
            A[D % W] = run(X[D], IntC<(HEAD && D == 0) ? 1 : 0>{});
            if constexpr (chain_skew::window_closes((uint32_t)D, (uint32_t)W)) {
                constexpr int OFF = (int)chain_skew::window_first((uint32_t)D, (uint32_t)W) * CHG * 4;
                if (out.isG) chain_store_window<OFF, W>(A, ooff, rsrc, soff, smask);
                else chain_store_window_lds<OFF, W>(A, ooff + soff, smask);
            }
            if constexpr (NS0 > 0 && !LAST) load(soff + span * 4u, Dc, X[D]);
        });
    };
    constexpr int NSPAN = (int)(n / span);
    if constexpr (NS0 > 0 || IsChainStep<Step>::kShort) {
        // Streamed operands: the spans are written out one after the other. As a loop around a peeled head and last span the
        // prefetched registers were carried through phi copies at every span end, each behind a wait for ITS load — the whole
        // next span drained there (vmcnt 24, 20 .. 2 in a row) instead of one group at a time.
        // A short step without operands (ChainStep::kShort) is written out too: 0.6 KB per span, and no counter or back edge.
        static_for<0, NSPAN>([&](auto Sc) {
            constexpr int S = decltype(Sc)::value;
            span_body((uint32_t)S * span * 4u, IntC<S == 0 ? 1 : 0>{}, IntC<S == NSPAN - 1 ? 1 : 0>{});
        });
    } else if constexpr (n == span) span_body(0u, IntC<1>{}, IntC<1>{});
    else {
        // No streamed operand, a step of some length: a loop around the inner spans (counter and back edge: ~1 instruction per
        // group). With EVERY such loop written out the C2 voice kernel grew from 48 to 65 KB of code and its block period went UP,
        // 7.12 k -> 7.17 k cycles (profiles/r09/spec_island_wave_busy_c2_chain_window.txt): only the short steps are.
        span_body(0u, IntC<1>{}, IntC<0>{});
        for (uint32_t t0 = span; t0 + span < n; t0 += span) span_body(t0 * 4u, IntC<0>{}, IntC<0>{});
        span_body((n - span) * 4u, IntC<0>{}, IntC<1>{});
    }
    // No tail: the lane of skew 0 has none to run (it stepped frame n - 1 in the last group), so it holds the member's final state,
    // and the lanes of skew k take it from there where they would step their last 4k frames to the same bits. A mirror lane's quad
    // is four unskewed copies of the last member: it reads its own value back.
    static_assert(!chain_skew::tail_active(0u, 0u), "skew 0 ends the last group with the final state");
    step.each([](auto& s) { quad_first(s); });
#undef CHAIN_OPAQUE_OFFSETS
}
// DEPTH = groups in flight per streamed operand (16 VGPRs each).
template <int NIN, uint32_t CM, int DEPTH, typename Step>
__device__ __forceinline__ void chain_loop_d(const SIn (&in)[NIN], const SOut out, uint32_t n, Step&& step) {
    constexpr int NS0 = NIN - __builtin_popcount(CM & ((1u << NIN) - 1u));
    constexpr int NS = NS0 > 0 ? NS0 : 1;
    // Lanes beyond the task's members repeat the last member's loads and ARITHMETIC (full EXEC is the cheap VALU mode, and
    // their state must stay a copy of the member's: every lane writes it back to the node record) but not its STORES:
    // 64 lanes x 16 bytes at one address is 1 KB through the CU's texture-address / LDS data path per instruction
    // (measured on the C2 voice: the phasor wave 11.3 k -> 9.1 k cycles per block). Masking the loads as well, with the
    // extra lanes running on stale operands, was measured too: slower (pole wave 12.9 k -> 14.1 k).
    // Arena accesses are buffer loads / stores over the WHOLE arena (one descriptor, < 2 GB): the lane's buffer offset in the
    // VGPR offset — for a store the extra lanes' offset is out of range and the hardware drops it: no EXEC change, no branch,
    // straight-line code in which the compiler's wait counts for the prefetched loads stay exact — the span's position in
    // the scalar offset, the frame inside the span in the 12-bit immediate.
    // (every recurrence that spec_stateful lays out in quads names its carried registers: a plain lambda stays on the loop below)
    if constexpr (ELEMHIP_SPEC_BLOCK % (DEPTH * CHG) == 0 && NIN <= 3 && IsChainStep<Step>::value) {
        if (out.quad && n == (uint32_t)ELEMHIP_SPEC_BLOCK) {
            bool allG = true;                                // (folds: the operand kinds are compile-time facts of the task)
#pragma unroll
            for (int k = 0; k < NIN; ++k) if (!((CM >> k) & 1u)) allG = allG && in[k].isG;
            if (__builtin_amdgcn_ballot_w64(!allG) == 0ull) return chain_loop_q<NIN, CM, DEPTH>(in, out, step);
        }
    }
    // (a quad task that stays on this loop — an LDS operand, the wide biquad — stores from the first lane of each quad)
    unsigned long long smask = out.quad ? (chain_skew::store_mask(out.cnt) & 0x1111111111111111ull)
                                        : (out.cnt >= 64u ? ~0ull : ((1ull << out.cnt) - 1ull));   // the task's member lanes
    const bool io = ((smask >> opaque_lane()) & 1ull) != 0ull;
    gfp arena = out.arena;
#pragma unroll
    for (int k = 0; k < NIN; ++k) if (in[k].isG) arena = in[k].arena;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((float*)arena, 0, 0x7FFFFFFF, 0x00020000);
    uint32_t ooff = out.goff;
    uint32_t ioff[NIN];
#pragma unroll
    for (int k = 0; k < NIN; ++k) ioff[k] = in[k].goff;
    // The offsets are made opaque once per span: left visible, `offset + constant` is loop-invariant, gets hoisted as one
    // register PER ACCESS (31 VGPRs and, for a wave-uniform offset, a v_mov in front of every load) instead of being folded
    // into the instruction's immediate at selection time.
#define CHAIN_OPAQUE_OFFSETS() do { asm volatile("" : "+v"(ooff)); _Pragma("unroll") for (int k_ = 0; k_ < NIN; ++k_) asm volatile("" : "+v"(ioff[k_])); } while (0)
    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
    // soff: byte offset of the span inside the block (wave-uniform); D: group of the span (compile-time: folds into the immediate)
    auto load = [&](uint32_t soff, auto Dc, float (&x)[NS][CHG]) {
        constexpr int D = decltype(Dc)::value;
        int s_ = 0;
#pragma unroll
        for (int k = 0; k < NIN; ++k) {
            if (!((CM >> k) & 1u)) {
#pragma unroll
                for (int q = 0; q < CHG / 4; ++q) {
                    v4f a;
                    // (global loads: the same broadcast access as a buffer load over the arena descriptor came back ~800 cycles
                    //  per block later on the C2 voice's envelope pole, profiles/r03/ab_chain_loops.txt)
                    if (in[k].isG) a = *(gcv4)((gcfp)((const char __attribute__((address_space(1)))*)arena + ioff[k] + soff) + (D * CHG + 4 * q));
                    else a = ld4(in[k].base + (soff >> 2) + (uint32_t)(D * CHG + 4 * q));
                    x[s_][4 * q] = a.x; x[s_][4 * q + 1] = a.y; x[s_][4 * q + 2] = a.z; x[s_][4 * q + 3] = a.w;
                }
                ++s_;
            }
        }
    };
    auto run = [&](float (&x)[NS][CHG], uint32_t soff, auto Dc) {
        constexpr int D = decltype(Dc)::value;
        float y[CHG];
        // one wait per 16-frame group (for its LAST load: vector loads return in order) instead of one per 16-byte load
        if (NS0 > 0 && NIN <= 3) {   // (the 6-operand biquad sits at the register limit of its kernels: the extra liveness spills)
#pragma unroll
            for (int k_ = 0; k_ < NS; ++k_) asm volatile("" : "+v"(x[k_][CHG - 4]), "+v"(x[k_][CHG - 3]), "+v"(x[k_][CHG - 2]), "+v"(x[k_][CHG - 1]));
        }
#pragma unroll
        for (int j = 0; j < CHG; ++j) {
            float xs[NIN];
            int s_ = 0;
#pragma unroll
            for (int k = 0; k < NIN; ++k) {
                if ((CM >> k) & 1u) xs[k] = in[k].cval;
                else xs[k] = x[s_++][j];
            }
            y[j] = step(xs);
        }
        if (out.isG) {
            v4f a[CHG / 4];
#pragma unroll
            for (int q = 0; q < CHG / 4; ++q) { a[q].x = y[4 * q]; a[q].y = y[4 * q + 1]; a[q].z = y[4 * q + 2]; a[q].w = y[4 * q + 3]; }
            static_assert(CHG == 16, "chain_store_group writes four 16-byte pieces");
            chain_store_group<D * CHG * 4>(a[0], a[1], a[2], a[3], ooff, rsrc, soff, smask);
        } else {
            // LDS output: EXEC cut to the member lanes inside one asm statement as well (a branch around the stores would make
            // the compiler's wait counts for the prefetched loads conservative)
            v4f a[CHG / 4];
#pragma unroll
            for (int q = 0; q < CHG / 4; ++q) { a[q].x = y[4 * q]; a[q].y = y[4 * q + 1]; a[q].z = y[4 * q + 2]; a[q].w = y[4 * q + 3]; }
            const uint32_t addr = (out.lds << 2) + soff;
            const unsigned long long sm_ = smask;      // (an asm operand alone does not make a generic lambda capture the variable)
            unsigned long long saved;
            asm volatile("s_mov_b64 %0, exec\n\t"
                         "s_mov_b64 exec, %6\n\t"
                         "ds_write_b128 %5, %1 offset:%c7\n\t"
                         "ds_write_b128 %5, %2 offset:%c8\n\t"
                         "ds_write_b128 %5, %3 offset:%c9\n\t"
                         "ds_write_b128 %5, %4 offset:%c10\n\t"
                         "s_mov_b64 exec, %0"
                         : "=&s"(saved)
                         : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(addr), "s"(sm_),
                           "i"(D * CHG * 4), "i"(D * CHG * 4 + 16), "i"(D * CHG * 4 + 32), "i"(D * CHG * 4 + 48)
                         : "memory");
        }
    };
    constexpr uint32_t span = (uint32_t)(DEPTH * CHG);
    const uint32_t nFull = n - n % span;
    float X[DEPTH][NS][CHG];
    CHAIN_OPAQUE_OFFSETS();
    if (nFull && NS0 > 0) {
        static_for<0, DEPTH>([&](auto Dc) { load(0u, Dc, X[decltype(Dc)::value]); });
        take_deferred<DEPTH * NS0 * (CHG / 4)>(out.defer);   // the previous block is published under this block's first loads
    } else take_deferred<0>(out.defer);
    for (uint32_t t0 = 0; t0 < nFull; t0 += span) {
        const uint32_t soff = t0 * 4u;
        const uint32_t nxt = (t0 + span < nFull) ? soff + span * 4u : soff;   // nothing left: harmless re-read (never past the block)
        CHAIN_OPAQUE_OFFSETS();
        static_for<0, DEPTH>([&](auto Dc) {
            run(X[decltype(Dc)::value], soff, Dc);
            if (NS0 > 0) load(nxt, Dc, X[decltype(Dc)::value]);
        });
    }
    for (uint32_t t = nFull; t < n; ++t) {
        float xs[NIN];
#pragma unroll
        for (int k = 0; k < NIN; ++k) xs[k] = ((CM >> k) & 1u) ? in[k].cval : sin_at(in[k], t);
        const float y = step(xs);
        if (io) sout_put(out, t, y);
    }
#undef CHAIN_OPAQUE_OFFSETS
}
// The arena loads of a recurrence come back from L2 after 1-2 k cycles when the whole chip is streaming; with one
// streamed operand 8 groups (128 frames, 128 VGPRs) are kept in flight — measured on the C2 voice's envelope pole:
// 15.7 k cycles per block at depth 2, 12.9 k at 4, 12.0 k at 8 — as long as the block is a multiple of that span.
// A specialised kernel is compiled for ONE engine block size (ELEMHIP_SPEC_BLOCK, jit.cpp): only the prefetch depth that block
// size uses is instantiated (r04 carried both and chose by `n` at run time — twice the loops for the optimizer to chew through).
// A block size that is a multiple of 128 frames gets depth 8; a call that asks for fewer frames than the block (n not a
// multiple of 128) renders its remainder frame by frame here.
// One-stream recurrences with more than three operands keep depth 4 (C4 biquad: 27.9 k cycles per block at 8, 24.7 k at 4).
template <int NIN, uint32_t CM, typename Step>
__device__ __forceinline__ void chain_loop_m(const SIn (&in)[NIN], const SOut out, uint32_t n, Step&& step) {
    constexpr int NS0 = NIN - __builtin_popcount(CM & ((1u << NIN) - 1u));
    if constexpr (NS0 == 1 && NIN > 3) {
        chain_loop_d<NIN, CM, 4>(in, out, n, step);
    } else if constexpr (NS0 == 1) {
        chain_loop_d<NIN, CM, ELEMHIP_SPEC_BLOCK % 128 == 0 ? 8 : 4>(in, out, n, step);
    } else if constexpr (NS0 == 0) chain_loop_d<NIN, CM, 4>(in, out, n, step);   // nothing to load: the depth only shapes the unrolling
    else if constexpr (NS0 == 2) chain_loop_d<NIN, CM, 4>(in, out, n, step);
    else chain_loop_d<NIN, CM, 2>(in, out, n, step);
}
#else
template <int NIN, uint32_t CM, typename Step>
__device__ __forceinline__ void chain_loop_m(const SIn (&in)[NIN], const SOut out, uint32_t n, Step&& step) {
    const uint32_t outBase = out.lds;
    constexpr int NS0 = NIN - __builtin_popcount(CM & ((1u << NIN) - 1u));
    constexpr int NS = NS0 > 0 ? NS0 : 1;
    const uint32_t nFull = n & ~(uint32_t)(CH - 1);
    auto load = [&](uint32_t t0, float (&x)[NS][CH]) {
        int s_ = 0;
#pragma unroll
        for (int k = 0; k < NIN; ++k) {
            if (!((CM >> k) & 1u)) {
                const v4f a = ld4(in[k].base + t0), b = ld4(in[k].base + t0 + 4);
                x[s_][0] = a.x; x[s_][1] = a.y; x[s_][2] = a.z; x[s_][3] = a.w;
                x[s_][4] = b.x; x[s_][5] = b.y; x[s_][6] = b.z; x[s_][7] = b.w;
                ++s_;
            }
        }
    };
    auto run8 = [&](const float (&x)[NS][CH], uint32_t t0) {
        float y[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            float xs[NIN];
            int s_ = 0;
#pragma unroll
            for (int k = 0; k < NIN; ++k) {
                if ((CM >> k) & 1u) xs[k] = in[k].cval;
                else xs[k] = x[s_++][j];
            }
            y[j] = step(xs);
        }
        v4f a, b;
        a.x = y[0]; a.y = y[1]; a.z = y[2]; a.w = y[3]; b.x = y[4]; b.y = y[5]; b.z = y[6]; b.w = y[7];
        st4(outBase + t0, a);
        st4(outBase + t0 + 4, b);
    };
    float A[NS][CH], B[NS][CH];
    uint32_t t0 = 0;
    if (nFull && NS0 > 0) load(0, A);
    while (t0 + 2 * CH <= nFull) {
        if (NS0 > 0) load(t0 + CH, B);
        run8(A, t0);
        if (NS0 > 0) load((t0 + 2 * CH < nFull) ? t0 + 2 * CH : t0, A);   // nothing left: harmless re-read
        run8(B, t0 + CH);
        t0 += 2 * CH;
    }
    if (t0 < nFull) { run8(A, t0); t0 += CH; }
    for (uint32_t t = nFull; t < n; ++t) {
        float xs[NIN];
#pragma unroll
        for (int k = 0; k < NIN; ++k) xs[k] = ((CM >> k) & 1u) ? in[k].cval : lds[in[k].base + t];
        lds[outBase + t] = step(xs);
    }
}

#endif   // ELEMHIP_SPEC chain_loop_m

// Dispatch on the task's cell mask (wave-uniform): every combination for up to 3 operands; for the
// 6-operand biquad the two shapes that occur (coefficients constant / everything a signal).
template <int NIN, typename Step>
__device__ __forceinline__ void chain_loop(const SIn (&in)[NIN], uint32_t cmask, const SOut outBase, uint32_t n, Step&& step) {
    cmask &= (1u << NIN) - 1u;
    if constexpr (NIN == 1) {
        if (cmask) chain_loop_m<1, 1u>(in, outBase, n, step); else chain_loop_m<1, 0u>(in, outBase, n, step);
    } else if constexpr (NIN == 2) {
        switch (cmask) {
            case 0: chain_loop_m<2, 0u>(in, outBase, n, step); break;
            case 1: chain_loop_m<2, 1u>(in, outBase, n, step); break;
            case 2: chain_loop_m<2, 2u>(in, outBase, n, step); break;
            default: chain_loop_m<2, 3u>(in, outBase, n, step); break;
        }
    } else if constexpr (NIN == 3) {
        switch (cmask) {
            case 0: chain_loop_m<3, 0u>(in, outBase, n, step); break;
            case 1: chain_loop_m<3, 1u>(in, outBase, n, step); break;
            case 2: chain_loop_m<3, 2u>(in, outBase, n, step); break;
            case 3: chain_loop_m<3, 3u>(in, outBase, n, step); break;
            case 4: chain_loop_m<3, 4u>(in, outBase, n, step); break;
            case 5: chain_loop_m<3, 5u>(in, outBase, n, step); break;
            case 6: chain_loop_m<3, 6u>(in, outBase, n, step); break;
            default: chain_loop_m<3, 7u>(in, outBase, n, step); break;
        }
    } else {
        static_assert(NIN == 6, "chain arity");
        if (cmask == 0x1Fu) chain_loop_m<6, 0x1Fu>(in, outBase, n, step);
        else {
            // mixed shapes: materialise the cells of constant operands as (degenerate) buffers is not
            // possible, so fall back to per-frame reads — correct for any mask, just slower
            for (uint32_t t = 0; t < n; ++t) {
                float xs[NIN];
#pragma unroll
                for (int k = 0; k < NIN; ++k) xs[k] = ((cmask >> k) & 1u) ? in[k].cval : sin_at(in[k], t);
                const float y = step(xs);
                sout_put(outBase, t, y);
            }
        }
    }
}

// Publish / wait of a task that owns its wave (see Persist). Runs in the lanes of the task's members only; every value is
// wave-uniform. Same protocol as the walk: LDS operations of a wave complete in order, so the counter update is ordered
// behind the block's samples; the poll is followed by an acquire fence before the next block's inputs are read.
__device__ __forceinline__ void persist_publish(const Persist& ps, uint32_t copy) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt(0xC07F);
    if (opaque_lane() == 0) {
        uint32_t t0, t1;
        asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, 1\n\tds_add_u32 %0, %1" : "=&v"(t0), "=&v"(t1) : "s"((ps.ctr + ps.s * ps.D + copy) << 2) : "memory");
    }
}
__device__ __forceinline__ void persist_wait(const Persist& ps, uint32_t use, uint32_t copy) {
    const uint32_t wLast = ps.ctr + ps.lastStage * ps.D + copy;
    const uint32_t wPrev = ps.prev == kNone ? wLast : ps.ctr + ps.prev * ps.D + copy;
    for (;;) {
        uint32_t cPrev, cLast;
        wlds_ld2(wPrev, wLast, cPrev, cLast);
        if ((ps.prev == kNone || UNI(cPrev) >= (use + 1u) * ps.prevT) && (use == 0u || UNI(cLast) >= use * ps.lastT)) break;
        __builtin_amdgcn_s_sleep(2);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}


// chain_loop for the recurrence nodes whose whole state lives in the registers `step` captures: when the task owns its wave
// it goes on with the following blocks of the launch right here — the operands that are block buffers and the output move
// to the next buffer set, cells stay — so a block costs the recurrence plus one counter round trip instead of a trip
// through the walk (publish, poll, header, dispatch, member and record decode: ~3 k cycles on the C2 voice).
template <int NIN, typename Run>
__device__ __forceinline__ void persist_blocks(const Ctx& c, const SIn (&in)[NIN], uint32_t cmask, const SOut outBase, Run&& run) {
    Persist* ps = c.ps;
#ifdef ELEMHIP_SPEC
    const bool own = false;      // (a specialised kernel's recurrences never take this LDS protocol)
#else
    const bool own = ps != nullptr && ps->on != 0u;
#endif
    const uint32_t D = own ? ps->D : 1u, copy0 = own ? ps->b % D : 0u;
    uint32_t b = own ? ps->b : 0u, copy = copy0, use = b / D, off = 0u;
    for (;;) {
        SIn inB[NIN];
#pragma unroll
        for (int k = 0; k < NIN; ++k) { inB[k] = in[k]; if (!((cmask >> k) & 1u)) inB[k].base += off; }
        SOut outB = outBase; outB.lds += off;
        run(inB, outB);   // (raising the wave priority around the recurrence was measured: 6 % slower overall)
        if (!own) return;
        persist_publish(*ps, copy);
        if (++b == ps->batch) break;
        if (++copy == D) { copy = 0u; ++use; }
        persist_wait(*ps, use, copy);
        off = copy * ps->slotArea - copy0 * ps->slotArea;   // may wrap: unsigned arithmetic
    }
    ps->done = 1u;
}
template <int NIN, typename Step>
__device__ __forceinline__ void chain_blocks(const Ctx& c, const SIn (&in)[NIN], uint32_t cmask, const SOut outBase, Step&& step) {
    persist_blocks<NIN>(c, in, cmask, outBase, [&](const SIn (&inB)[NIN], const SOut out) { chain_loop<NIN>(inB, cmask, out, c.n, step); });
}
template <int NIN, uint32_t CM, typename Step>
__device__ __forceinline__ void chain_blocks_m(const Ctx& c, const SIn (&in)[NIN], const SOut outBase, Step&& step) {
    persist_blocks<NIN>(c, in, CM, outBase, [&](const SIn (&inB)[NIN], const SOut out) { chain_loop_m<NIN, CM>(inB, out, c.n, step); });
}
// CMT >= 0: the task's cell mask is a compile-time constant (a specialised kernel's task descriptor): only that variant of the
// loops is instantiated — the run-time switch of chain_blocks made every specialised kernel carry (and the optimizer chew through)
// all 2^NIN mask variants of its recurrences, 70 % of a synth voice's IR, until inlining finally proved the mask constant.
template <int CMT, int NIN, typename Step>
__device__ __forceinline__ void chain_blocks_c(const Ctx& c, const SIn (&in)[NIN], uint32_t cmask, const SOut outBase, Step&& step) {
    if constexpr (CMT >= 0 && (NIN <= 3 || ((uint32_t)CMT & ((1u << NIN) - 1u)) == 0x1Fu))
        chain_blocks_m<NIN, (uint32_t)CMT & ((1u << NIN) - 1u)>(c, in, outBase, step);
    else chain_blocks<NIN>(c, in, cmask, outBase, step);
}

__device__ __forceinline__ void szero(const Member& m, uint32_t n) {
    for (uint32_t t = 0; t < n; ++t) lds[m.outLds + t] = 0.0f;
}

__device__ __forceinline__ float change_tick(float& lastIn, float xn) {   // helpers/Change.h:20-31
    const float dt = xn - lastIn;
    lastIn = xn;
    return (dt > 0.0f) ? 1.0f : ((dt < 0.0f) ? -1.0f : 0.0f);
}

// PhasorNode (Core.h:85-136): step = f * (1/sr) in float; phase = next - floor(next)
template <int CMT = -1>
__device__ __forceinline__ void ser_phasor(const Ctx& c, const Member& m, uint32_t cm) {
    rup r = c.recs + m.rec * kRecDwords;
    if (member_nin(c, m) < 1) return szero(m, c.n);
    const SIn in[1] = {sin_of(c, opnd_lane(c, m, 0))};
    float phase = u2f(r[rec::S0]);
    const float rsr = 1.0f / c.srF;
    if ((cm & 1u) && in[0].cval * rsr >= 0.0f && phase >= 0.0f) {
        // constant non-negative step: next >= 0, so next - floor(next) is exactly v_fract_f32(next)
        const SIn st[1] = {sin_const(in[0].cval * rsr)};
        chain_blocks_m<1, 1u>(c, st, sout_of(c, m), chain_step<true>([&](const float (&x)[1]) {   // (two VALU ops per frame: written out)
            const float y = phase;
            phase = __builtin_amdgcn_fractf(phase + x[0]);
            return y;
        }, [&](auto&& g) { g(phase); }));
    } else {
        chain_blocks_c<CMT, 1>(c, in, cm, sout_of(c, m), chain_step([&](const float (&x)[1]) {
            const float stepv = x[0] * rsr;
            const float y = phase;
            const float next = phase + stepv;
            phase = next - floorf(next);
            return y;
        }, [&](auto&& g) { g(phase); }));
    }
    r[rec::S0] = f2u(phase);
}

template <int CMT = -1>
__device__ __forceinline__ void ser_sphasor(const Ctx& c, const Member& m, uint32_t cm) {
    rup r = c.recs + m.rec * kRecDwords;
    if (member_nin(c, m) < 2) return szero(m, c.n);
    const SIn in[2] = {sin_of(c, opnd_lane(c, m, 0)), sin_of(c, opnd_lane(c, m, 1))};
    float phase = u2f(r[rec::S0]), lastIn = u2f(r[rec::S1]);
    const float rsr = 1.0f / c.srF;
    chain_blocks_c<CMT, 2>(c, in, cm, sout_of(c, m), chain_step([&](const float (&x)[2]) {
        if (change_tick(lastIn, x[1]) > 0.5f) phase = 0.0f;
        const float stepv = x[0] * rsr;
        const float y = phase;
        const float next = phase + stepv;
        phase = next - floorf(next);
        return y;
    }, [&](auto&& g) { g(phase); g(lastIn); }));
    r[rec::S0] = f2u(phase); r[rec::S1] = f2u(lastIn);
}

// OnePoleNode (Filters.h:13-39): z = x + p*z
template <int CMT = -1>
__device__ __forceinline__ void ser_pole(const Ctx& c, const Member& m, uint32_t cm) {
    rup r = c.recs + m.rec * kRecDwords;
    if (member_nin(c, m) < 2) return szero(m, c.n);
    const SIn in[2] = {sin_of(c, opnd_lane(c, m, 0)), sin_of(c, opnd_lane(c, m, 1))};
    float z = u2f(r[rec::S0]);
    chain_blocks_c<CMT, 2>(c, in, cm, sout_of(c, m), chain_step([&](const float (&x)[2]) { z = x[1] + x[0] * z; return z; },
                                                                [&](auto&& g) { g(z); }));
    r[rec::S0] = f2u(z);
}

// EnvelopeNode (Filters.h:46-79)
template <int CMT = -1>
__device__ __forceinline__ void ser_env(const Ctx& c, const Member& m, uint32_t cm) {
    rup r = c.recs + m.rec * kRecDwords;
    if (member_nin(c, m) < 3) return szero(m, c.n);
    const SIn in[3] = {sin_of(c, opnd_lane(c, m, 0)), sin_of(c, opnd_lane(c, m, 1)), sin_of(c, opnd_lane(c, m, 2))};
    float z = u2f(r[rec::S0]);
    chain_blocks_c<CMT, 3>(c, in, cm, sout_of(c, m), chain_step([&](const float (&x)[3]) {
        const float vn = fabsf(x[2]);
        if (fabsf(vn) > z) z = x[0] * (z - vn) + vn;
        else               z = x[1] * (z - vn) + vn;
        return z;
    }, [&](auto&& g) { g(z); }));
    r[rec::S0] = f2u(z);
}

// BiquadFilterNode (Filters.h:87-120), TDF-II with coefficient signals
template <int CMT = -1>
__device__ __forceinline__ void ser_biquad(const Ctx& c, const Member& m, uint32_t cm) {
    rup r = c.recs + m.rec * kRecDwords;
    if (member_nin(c, m) < 6) return szero(m, c.n);
    SIn in[6];
    in[0] = sin_of(c, opnd_lane(c, m, 0)); in[1] = sin_of(c, opnd_lane(c, m, 1)); in[2] = sin_of(c, opnd_lane(c, m, 2));
    in[3] = sin_of(c, opnd_lane(c, m, 3)); in[4] = sin_of(c, opnd_lane(c, m, 4)); in[5] = sin_of(c, opnd_lane(c, m, 5));
    float z1 = u2f(r[rec::S0]), z2 = u2f(r[rec::S1]);
    // The nine scalar operations of Filters.h:103-105 (no contraction) with the compiler's pairing switched off (an empty asm on
    // one twin of each pair): left alone, its SLP pass packs (b1 x, b2 x), (a1 y, a2 y) and the two differences with a v_mov_b32
    // per broadcast ON the loop-carried path (y -> (y, y) -> product), five dependent operations per frame instead of four.
    // Packed forms were measured slower or no faster (profiles/r06/c4_biquad_forms.txt; DESIGN.md §8).
    chain_blocks_c<CMT, 6>(c, in, cm, sout_of(c, m), [&](const float (&x)[6]) {
        const float xx = x[5];
        const float s0 = x[0] * xx, p1 = x[1] * xx;
        float p2 = x[2] * xx;
        asm("" : "+v"(p2));
        const float y = s0 + z1;
        const float t1 = x[3] * y;
        float t2 = x[4] * y;
        asm("" : "+v"(t2));
        z1 = p1 - t1 + z2;
        z2 = p2 - t2;
        return y;
    });
    r[rec::S0] = f2u(z1); r[rec::S1] = f2u(z2);
}

// CounterNode / AccumNode / LatchNode / MaxHold / OnceNode (Core.h:183-404)
template <int CMT = -1>
__device__ __forceinline__ void ser_counter(const Ctx& c, const Member& m, uint32_t cm) {
    rup r = c.recs + m.rec * kRecDwords;
    if (member_nin(c, m) < 1) return szero(m, c.n);
    const SIn in[1] = {sin_of(c, opnd_lane(c, m, 0))};
    float count = u2f(r[rec::S0]);
    chain_blocks_c<CMT, 1>(c, in, cm, sout_of(c, m), chain_step([&](const float (&x)[1]) {
        if ((1.0f - x[0]) <= FLT_EPSILON) { const float y = count; count = count + 1.0f; return y; }
        count = 0.0f;
        return 0.0f;
    }, [&](auto&& g) { g(count); }));
    r[rec::S0] = f2u(count);
}

template <int CMT = -1>
__device__ __forceinline__ void ser_accum(const Ctx& c, const Member& m, uint32_t cm) {
    rup r = c.recs + m.rec * kRecDwords;
    if (member_nin(c, m) < 2) return szero(m, c.n);
    const SIn in[2] = {sin_of(c, opnd_lane(c, m, 0)), sin_of(c, opnd_lane(c, m, 1))};
    float total = u2f(r[rec::S0]), lastIn = u2f(r[rec::S1]);
    chain_blocks_c<CMT, 2>(c, in, cm, sout_of(c, m), chain_step([&](const float (&x)[2]) {
        if (change_tick(lastIn, x[1]) > 0.5f) total = 0.0f;
        total += x[0];
        return total;
    }, [&](auto&& g) { g(total); g(lastIn); }));
    r[rec::S0] = f2u(total); r[rec::S1] = f2u(lastIn);
}

template <int CMT = -1>
__device__ __forceinline__ void ser_latch(const Ctx& c, const Member& m, uint32_t cm) {
    rup r = c.recs + m.rec * kRecDwords;
    if (member_nin(c, m) < 2) return szero(m, c.n);
    const SIn in[2] = {sin_of(c, opnd_lane(c, m, 0)), sin_of(c, opnd_lane(c, m, 1))};
    float z = u2f(r[rec::S0]), hold = u2f(r[rec::S1]);
    chain_blocks_c<CMT, 2>(c, in, cm, sout_of(c, m), chain_step([&](const float (&x)[2]) {
        if (fabsf(z) <= FLT_EPSILON && x[0] > FLT_EPSILON) hold = x[1];
        z = x[0];
        return hold;
    }, [&](auto&& g) { g(z); g(hold); }));
    r[rec::S0] = f2u(z); r[rec::S1] = f2u(hold);
}

template <int CMT = -1>
__device__ __forceinline__ void ser_maxhold(const Ctx& c, const Member& m, uint32_t cm) {
    rup r = c.recs + m.rec * kRecDwords;
    if (member_nin(c, m) < 2) return szero(m, c.n);
    const SIn in[2] = {sin_of(c, opnd_lane(c, m, 0)), sin_of(c, opnd_lane(c, m, 1))};
    const uint32_t hts = r[rec::P0];
    float lastIn = u2f(r[rec::S0]); uint32_t at = r[rec::S1]; float mx = u2f(r[rec::S2]);
    chain_blocks_c<CMT, 2>(c, in, cm, sout_of(c, m), chain_step([&](const float (&x)[2]) {
        if (change_tick(lastIn, x[1]) > 0.5f || ++at >= hts) { mx = x[0]; at = 0; }
        else if (x[0] > mx) { at = 0; mx = x[0]; }
        return mx;
    }, [&](auto&& g) { g(lastIn); g(at); g(mx); }));
    r[rec::S0] = f2u(lastIn); r[rec::S1] = at; r[rec::S2] = f2u(mx);
}

__device__ __forceinline__ void ser_once(const Ctx& c, const Member& m, uint32_t cm) {
    rup r = c.recs + m.rec * kRecDwords;
    if (member_nin(c, m) < 1) return szero(m, c.n);
    const SIn in[1] = {sin_of(c, opnd_lane(c, m, 0))};
    const bool isArmed = u2f(r[rec::S2]) != 0.0f;    // atomic<FloatType> armed, loaded once per block
    float gain = u2f(r[rec::S0]), lastIn = u2f(r[rec::S1]);
    bool disarm = false;
    chain_loop<1>(in, cm, sout_of(c, m), c.n, [&](const float (&x)[1]) {
        const float delta = change_tick(lastIn, x[0]);
        if (isArmed && delta > 0.5f) { gain = 1.0f; disarm = true; }
        if (delta < -0.5f) gain = 0.0f;
        return x[0] * gain;
    });
    r[rec::S0] = f2u(gain); r[rec::S1] = f2u(lastIn);
    if (disarm) r[rec::S2] = f2u(0.0f);
}

// SequenceNode (Core.h:407-573)
__device__ __forceinline__ void ser_seq(const Ctx& c, const Member& m, uint32_t cm) {
    rup r = c.recs + m.rec * kRecDwords;
    gcfp seq = rec_ptr(r, rec::SEQ_PTR);
    const uint32_t len = r[rec::SEQ_LEN];
    uint32_t idx = r[rec::SEQ_INDEX];
    float holdValue = u2f(r[rec::SEQ_HOLDVAL]);
    bool first = r[rec::SEQ_FIRST] != 0;
    bool have = r[rec::SEQ_HAVE] != 0;        // activeSequence != nullptr
    if (r[rec::SEQ_PENDING]) {                // a new sequence arrived since the last block (:468-492)
        r[rec::SEQ_PENDING] = 0;
        have = true;
        // size_t % 0 is UB in the reference; an empty sequence leaves the index untouched here
        if (len) idx = idx % len;
        if (first && len) holdValue = seq[idx];
    }
    const uint32_t nin = member_nin(c, m);
    if (nin < 1 || !have) {
        r[rec::SEQ_INDEX] = idx; r[rec::SEQ_HOLDVAL] = f2u(holdValue); r[rec::SEQ_HAVE] = have;
        return szero(m, c.n);
    }
    const bool hasReset = nin > 1;
    const bool hold = r[rec::SEQ_HOLD] != 0, loop = r[rec::SEQ_LOOP] != 0;
    const uint32_t offset = r[rec::SEQ_OFFSET];
    const SIn in[2] = {sin_of(c, opnd_lane(c, m, 0)), hasReset ? sin_of(c, opnd_lane(c, m, 1)) : sin_const(0.0f)};
    const uint32_t cm2 = hasReset ? cm : (cm | 2u);
    float chg = u2f(r[rec::SEQ_CHANGE]), rchg = u2f(r[rec::SEQ_RCHANGE]);
    chain_loop<2>(in, cm2, sout_of(c, m), c.n, [&](const float (&x)[2]) {
        if (change_tick(rchg, x[1]) > 0.5f) idx = offset;
        if (change_tick(chg, x[0]) > 0.5f) {
            // std::min(seqIndex, size - 1): size_t arithmetic, an empty sequence reads nothing here
            if (len) holdValue = seq[min(idx, len - 1)];
            first = true;
            if ((++idx >= len) && loop) idx = 0;
        }
        if (idx < len) return hold ? holdValue : holdValue * x[0];
        return hold ? holdValue : 0.0f;
    });
    r[rec::SEQ_INDEX] = idx; r[rec::SEQ_HOLDVAL] = f2u(holdValue); r[rec::SEQ_FIRST] = first;
    r[rec::SEQ_CHANGE] = f2u(chg); r[rec::SEQ_RCHANGE] = f2u(rchg); r[rec::SEQ_HAVE] = 1;
}

// Seq2Node (Seq2.h:87-147): rising edges are counted, the index is offset + count
__device__ __forceinline__ void ser_seq2(const Ctx& c, const Member& m, uint32_t cm) {
    rup r = c.recs + m.rec * kRecDwords;
    gcfp seq = rec_ptr(r, rec::SEQ_PTR);
    const uint32_t len = r[rec::SEQ_LEN];
    uint32_t edges = r[rec::S0];
    bool have = r[rec::SEQ_HAVE] != 0;
    if (r[rec::SEQ_PENDING]) { r[rec::SEQ_PENDING] = 0; have = true; }
    const uint32_t nin = member_nin(c, m);
    if (nin < 1 || !have) { r[rec::SEQ_HAVE] = have; return szero(m, c.n); }
    const bool hasReset = nin > 1;
    const bool hold = r[rec::SEQ_HOLD] != 0, loop = r[rec::SEQ_LOOP] != 0;
    const uint32_t offset = r[rec::SEQ_OFFSET];
    const SIn in[2] = {sin_of(c, opnd_lane(c, m, 0)), hasReset ? sin_of(c, opnd_lane(c, m, 1)) : sin_const(0.0f)};
    const uint32_t cm2 = hasReset ? cm : (cm | 2u);
    float chg = u2f(r[rec::SEQ_CHANGE]), rchg = u2f(r[rec::SEQ_RCHANGE]);
    chain_loop<2>(in, cm2, sout_of(c, m), c.n, [&](const float (&x)[2]) {
        if (change_tick(chg, x[0]) > 0.5f) edges++;
        if (change_tick(rchg, x[1]) > 0.5f) edges = 0;          // after the trigger check (:121-127)
        const uint32_t idx = offset + edges;
        // size_t % 0 and at(size - 1) on an empty sequence are UB / throw in the reference; an empty sequence emits 0 here
        const float next = len == 0u ? 0.0f : (idx < len) ? seq[idx] : (loop ? seq[idx % len] : (hold ? seq[len - 1u] : 0.0f));
        return hold ? next : next * x[0];
    });
    r[rec::S0] = edges; r[rec::SEQ_CHANGE] = f2u(chg); r[rec::SEQ_RCHANGE] = f2u(rchg); r[rec::SEQ_HAVE] = 1;
}

// SparSeqNode (SparSeq.h:17-372). The reference moves new sequences and loop points to the realtime thread through a queue it
// drains at the top of process(); here the host patches the record before the block and raises the two flags. The held event
// is an index into the tick-time sorted table (std::map order, first insert of a duplicate key wins: engine.cpp), -1 = end().
__device__ __forceinline__ void ser_sparseq(const Ctx& c, const Member& m, uint32_t cm) {
    rup r = c.recs + m.rec * kRecDwords;
    const uint32_t len = r[rec::SQ_LEN];
    typedef const int32_t __attribute__((address_space(1)))* gcip;
    gcip times = (gcip)rec_ptr(r, rec::SQ_SEQ);
    gcfp vals = (gcfp)(times + len);
    const int32_t offset = (int32_t)r[rec::SQ_OFFSET];
    const bool follow = r[rec::SQ_FOLLOW] != 0;
    const int32_t ho = (int32_t)r[rec::SQ_INTERP];
    const double spc = rec_ld_f64(r, rec::SQ_TICK);
    int32_t edges = (int32_t)r[rec::SQ_EDGES], hold = (int32_t)r[rec::SQ_HOLD];
    uint32_t since = r[rec::SQ_SINCE];
    int32_t ls = (int32_t)r[rec::SQ_LOOP_START], le = (int32_t)r[rec::SQ_LOOP_END];
    bool pend = r[rec::SQ_PEND_FLAG] != 0;
    int32_t pls = (int32_t)r[rec::SQ_PEND_START], ple = (int32_t)r[rec::SQ_PEND_END];
    bool have = r[rec::SQ_HAVE] != 0;
    auto tickTime = [&]() -> int32_t {                       // getTickTime (:154-199)
        int32_t tt = offset + edges;
        if (ls > -1 && le > -1 && tt >= le) {
            const int32_t dur = le - ls;
            if (dur > 0) {
                if (pend) {                                  // follow: the pending points take over at the end of the running loop
                    const int32_t oldEnd = le;
                    ls = pls; le = ple; pend = false;
                    if (ls == -1 && le == -1) return tt;
                    const int32_t nd = le - ls;
                    tt = ls + (nd != 0 ? (tt - oldEnd) % nd : 0);          // (% 0 is undefined in the reference)
                } else {
                    tt = ls + ((tt - le) % dur);
                }
                edges = tt - offset;
            }
        }
        return tt;
    };
    auto find = [&](int32_t tt) -> int32_t {                 // findTickValue (:133-152): last event at or before tt
        if (len == 0u) return -1;
        uint32_t lo = 0u, hi = len;                          // upper_bound
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (times[mid] > tt) hi = mid; else lo = mid + 1u; }
        if (lo == 0u) return times[0] == 0 ? 0 : -1;
        return (int32_t)lo - 1;
    };
    int32_t tt = tickTime();
    const bool newSeq = r[rec::SQ_SEQ_PENDING] != 0, newLoop = r[rec::SQ_LOOP_PENDING] != 0;
    if (newSeq || newLoop) {                                 // the change queue had something (:216-238)
        if (newSeq) have = true;
        if (newLoop) { pend = true; pls = (int32_t)r[rec::SQ_NEW_START]; ple = (int32_t)r[rec::SQ_NEW_END]; }
        r[rec::SQ_SEQ_PENDING] = 0; r[rec::SQ_LOOP_PENDING] = 0;
        hold = have ? find(tt) : -1;
    }
    if (pend && ((ls == -1 && le == -1) || !follow)) {       // (:244-252)
        ls = pls; le = ple; pend = false;
        tt = tickTime();
    }
    const uint32_t nin = member_nin(c, m);
    float chg = u2f(r[rec::SQ_CHANGE]), rchg = u2f(r[rec::SQ_RCHANGE]);
    if (nin < 1 || !have) {
        szero(m, c.n);
    } else {
        const bool hasReset = nin > 1;
        const SIn in[2] = {sin_of(c, opnd_lane(c, m, 0)), hasReset ? sin_of(c, opnd_lane(c, m, 1)) : sin_const(0.0f)};
        const uint32_t cm2 = hasReset ? cm : (cm | 2u);
        chain_loop<2>(in, cm2, sout_of(c, m), c.n, [&](const float (&x)[2]) {
            if (since != 0xFFFFFFFFu) since++;               // (a size_t in the reference: only its min with tickInterval is used)
            const bool trig = change_tick(chg, x[0]) > 0.5f, rst = change_tick(rchg, x[1]) > 0.5f;
            if (rst) edges = 0;
            if (trig) {
                edges = rst ? 0 : edges + 1;
                since = 0u;
                tt = tickTime();
                hold = find(tt);
            }
            if (hold < 0) return 0.0f;
            const float lv = vals[hold];
            if (ho != 1 || (uint32_t)hold + 1u >= len) return lv;
            const int32_t tl = times[hold], tr = times[hold + 1];
            const float rv = vals[hold + 1];
            double alpha = (double)max(0, tt - tl) / (double)(tr - tl);
            if (spc > 0.0) alpha += (fmin((double)since, spc) / spc) / (double)(tr - tl);
            return (float)((double)lv + alpha * (double)(rv - lv));
        });
    }
    r[rec::SQ_EDGES] = (uint32_t)edges; r[rec::SQ_SINCE] = since; r[rec::SQ_HOLD] = (uint32_t)hold;
    r[rec::SQ_CHANGE] = f2u(chg); r[rec::SQ_RCHANGE] = f2u(rchg); r[rec::SQ_HAVE] = have ? 1u : 0u;
    r[rec::SQ_LOOP_START] = (uint32_t)ls; r[rec::SQ_LOOP_END] = (uint32_t)le;
    r[rec::SQ_PEND_FLAG] = pend ? 1u : 0u; r[rec::SQ_PEND_START] = (uint32_t)pls; r[rec::SQ_PEND_END] = (uint32_t)ple;
}

// One output channel of MCSampleNode (mc/Sample.h:83-150) + MCVariablePitchReader::sumInto (:238-278), serial half. The
// reference cuts the block at the trigger's edges and lets both readers sum each segment into the outputs; a reader's read
// position inside a segment is pos + j * rate (not accumulated), its elem::GainFade (4 ms) moves once per sample it actually
// reads, and pos / the loop wrap are applied at the segment's end. Per frame and reader this pass leaves (read index |
// 0xFFFFFFFF = no contribution, fraction, gain) in the node's scratch; the gather pass interpolates (lerpRead :221-236).
__device__ __forceinline__ void ser_mcsample(const Ctx& c, const Member& m, uint32_t cm) {
    rup r = c.recs + m.rec * kRecDwords;
    const uint32_t len = r[rec::SMP_LEN];
    bool have = r[rec::SMP_HAVE] != 0;
    const float inStep = (float)(1.0 / (c.sr * 4.0 / 1000.0)), outStep = -1.0f * inStep;   // GainFade(sampleRate, 4.0, 4.0): GainFade.h:10-12, 74-82
    float tg[2], gn[2], st[2]; double pos[2]; uint32_t so[2], eo[2], lp[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        rcup rr = r + rec::MCS_READER0 + q * rec::MCS_READER_DWORDS;
        tg[q] = u2f(rr[0]); gn[q] = u2f(rr[1]); st[q] = u2f(rr[2]); pos[q] = rec_ld_f64(rr, 3); so[q] = rr[5]; eo[q] = rr[6]; lp[q] = rr[7];
    }
    auto fadeOut = [&](int q) { tg[q] = 0.0f; st[q] = gn[q] > tg[q] ? outStep : inStep; };
    auto fadeIn = [&](int q) { tg[q] = 1.0f; st[q] = gn[q] > tg[q] ? outStep : inStep; };
    if (r[rec::SMP_PENDING]) {                       // a new buffer: fresh readers (:98-103), GainFade(sr, 4, 4) at rest: step = inStep
        r[rec::SMP_PENDING] = 0; have = true;
#pragma unroll
        for (int q = 0; q < 2; ++q) { tg[q] = 0.0f; gn[q] = 0.0f; st[q] = inStep; pos[q] = 0.0; so[q] = 0u; eo[q] = 0u; lp[q] = 0u; }
    }
    if (r[rec::MCS_RESET]) { r[rec::MCS_RESET] = 0; fadeOut(0); fadeOut(1); }      // Runtime::reset -> MCSampleNode::reset (:78-81)
    const uint32_t nin = member_nin(c, m), n = c.n;
    const bool silent = nin < 1 || !have || rec_ptr(r, rec::SMP_BUF) == nullptr;
    if (silent) {
        r[rec::SMP_HAVE] = have;
        for (uint32_t i = 0; i < n; ++i) { lds[m.scratch + i] = u2f(0xFFFFFFFFu); lds[m.scratch + 3u * kSlotWords + i] = u2f(0xFFFFFFFFu); }
    } else {
        const uint32_t mode = r[rec::SMP_MODE];
        const bool wantsLoop = mode == 2u;
        const uint32_t ostart = r[rec::SMP_START], ostop = r[rec::SMP_STOP];
        const double rate = rec_ld_f64(r, rec::MCS_RATE);
        const SIn in0 = sin_of(c, opnd_lane(c, m, 0));
        const bool cell = (cm & 1u) != 0u;
        float chg = u2f(r[rec::SMP_CHANGE]);
        uint32_t cur = r[rec::SMP_CURRENT];
        uint32_t seg = 0;                              // first frame of the running segment
        // one segment [seg, j) of both readers (sumInto): per-frame records + the position / fade each reader ends with
        auto segment = [&](uint32_t j) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const double readStart = (double)so[q];
                const double readStop = (double)len - (double)eo[q];
                for (uint32_t k = 0; k < j - seg; ++k) {
                    double readPos = pos[q] + (double)k * rate;
                    uint32_t idx = 0xFFFFFFFFu; float frac = 0.0f, g = 0.0f;
                    bool reads = true;
                    if (readPos >= readStop) {
                        if (lp[q]) readPos = readStart + fmod(readPos - readStart, readStop - readStart);
                        else reads = false;
                    }
                    if (reads) {
                        const uint32_t left = (readPos >= 0.0 && readPos < 4.0e9) ? (uint32_t)readPos : (readPos < 0.0 ? 0u : 0xFFFFFFFEu);   // static_cast<size_t>
                        idx = left; frac = (float)(readPos - (double)left);
                        if (fabsf(gn[q] - tg[q]) <= 1e-6f) g = tg[q];                       // GainFade::operator() (GainFade.h:43-54)
                        else { g = gn[q]; gn[q] = clampf(gn[q] + st[q], 0.0f, 1.0f); }
                    }
                    const uint32_t w = m.scratch + (uint32_t)q * 3u * kSlotWords + seg + k;
                    lds[w] = u2f(idx); lds[w + kSlotWords] = frac; lds[w + 2u * kSlotWords] = g;
                }
                pos[q] += (double)(j - seg) * rate;
                if (pos[q] >= readStop && lp[q]) pos[q] = readStart + fmod(pos[q] - readStart, readStop - readStart);
            }
            seg = j;
        };
        for (uint32_t j = 0; j < n; ++j) {
            const float x = cell ? in0.cval : sin_at(in0, j);
            const float cv = change_tick(chg, x);
            if (cv > 0.5f) {                                                // rising edge (:116-125)
                segment(j);
                fadeOut((int)(cur & 1u));
                ++cur;
                const int q = (int)(cur & 1u);
                fadeIn(q); so[q] = ostart; eo[q] = ostop; lp[q] = wantsLoop ? 1u : 0u; pos[q] = (double)ostart;   // noteOn (:197-205)
            }
            if (cv < -0.5f && mode != 0u) { segment(j); fadeOut((int)(cur & 1u)); }   // falling edge, not in trigger mode (:127-134)
        }
        segment(n);
        r[rec::SMP_CHANGE] = f2u(chg); r[rec::SMP_CURRENT] = cur; r[rec::SMP_HAVE] = 1;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        rup rr = r + rec::MCS_READER0 + q * rec::MCS_READER_DWORDS;
        rr[0] = f2u(tg[q]); rr[1] = f2u(gn[q]); rr[2] = f2u(st[q]); rec_st_f64(rr, 3, pos[q]); rr[5] = so[q]; rr[6] = eo[q]; rr[7] = lp[q];
    }
}

// gather pass of an mc.sample channel: lerpRead (mc/Sample.h:221-236) of both readers, scaled by the recorded gains
__device__ __forceinline__ void gather_mcsample(const Ctx& c, const Member& m) {
    rcup r = c.recs + m.rec * kRecDwords;
    gcfp buf = rec_ptr(r, rec::SMP_BUF);
    const uint32_t len = UNI(r[rec::SMP_LEN]);
    for (uint32_t i = c.lane; i < c.n; i += 64) {
        float acc = 0.0f;                                   // std::fill_n(outputData[j], numSamples, 0) then both readers add (:105-107)
#pragma unroll
        for (uint32_t q = 0; q < 2; ++q) {
            const uint32_t w = m.scratch + q * 3u * kSlotWords + i;
            const uint32_t idx = ldsu(w);
            if (idx == 0xFFFFFFFFu || !buf) continue;
            float v = 0.0f;
            if (idx < len) v = (idx + 1u >= len) ? buf[idx] : (buf[idx] + lds[w + kSlotWords] * (buf[idx + 1u] - buf[idx]));
            acc += lds[w + 2u * kSlotWords] * v;
        }
        lds[m.outLds + i] = acc;
    }
}

// SampleNode (Sample.h:77-139) + VariablePitchLerpReader::tick (:178-221), serial half: edge detection, reader
// allocation, position / gain recurrences. Nothing here touches the sample data: per frame and reader it leaves
// (unwrapped read index | 0xFFFFFFFF = silent, fraction, gain) in the node's scratch for the gather pass.
__device__ __forceinline__ void ser_sample(const Ctx& c, const Member& m, uint32_t cm) {
    rup r = c.recs + m.rec * kRecDwords;
    const uint32_t len = r[rec::SMP_LEN];
    bool have = r[rec::SMP_HAVE] != 0;
    float tg[2], gn[2]; double pos[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        rcup rr = r + rec::SMP_READER0 + q * rec::SMP_READER_DWORDS;
        tg[q] = u2f(rr[0]); gn[q] = u2f(rr[1]); pos[q] = rec_ld_f64(rr, 2);
    }
    if (r[rec::SMP_PENDING]) {                       // a new buffer: fresh readers (:93-98)
        r[rec::SMP_PENDING] = 0; have = true;
        tg[0] = tg[1] = 0.0f; gn[0] = gn[1] = 0.0f; pos[0] = pos[1] = 0.0;
    }
    const uint32_t nin = member_nin(c, m);
    if (nin < 1 || !have || rec_ptr(r, rec::SMP_BUF) == nullptr) {
        r[rec::SMP_HAVE] = have;
        for (uint32_t i = 0; i < c.n; ++i) { lds[m.scratch + i] = u2f(0xFFFFFFFFu); lds[m.scratch + 3u * kSlotWords + i] = u2f(0xFFFFFFFFu); }
        return;
    }
    const uint32_t mode = r[rec::SMP_MODE];
    const bool loop = mode == 2u;
    const uint32_t ostart = r[rec::SMP_START], ostop = r[rec::SMP_STOP];
    const float alpha = u2f(r[rec::SMP_ALPHA]);
    // size_t arithmetic in the reference: a stop offset beyond the buffer wraps to a huge limit (never reached)
    const double limit = ostop <= len ? (double)(len - ostop) : 1.8446744073709552e19;
    const bool hasRate = nin >= 2;
    const SIn in[2] = {sin_of(c, opnd_lane(c, m, 0)), hasRate ? sin_of(c, opnd_lane(c, m, 1)) : sin_const(1.0f)};
    const uint32_t cm2 = hasRate ? cm : (cm | 2u);
    float chg = u2f(r[rec::SMP_CHANGE]);
    uint32_t cur = r[rec::SMP_CURRENT];
    uint32_t i = 0;
    chain_loop<2>(in, cm2, sout_of(c, m), c.n, [&](const float (&x)[2]) {
        const float cv = change_tick(chg, x[0]);
        const float rate = x[1];
        if (cv > 0.5f) {                               // rising edge: release the current reader, start the other
            if (cur & 1u) tg[1] = 0.0f; else tg[0] = 0.0f;
            ++cur;
            if (cur & 1u) { tg[1] = 1.0f; pos[1] = (double)ostart; } else { tg[0] = 1.0f; pos[0] = (double)ostart; }
        }
        if (cv < -0.5f && mode != 0u) { if (cur & 1u) tg[1] = 0.0f; else tg[0] = 0.0f; }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            uint32_t idx = 0xFFFFFFFFu; float frac = 0.0f, g = 0.0f;
            bool live = !(pos[q] < 0.0 || (gn[q] == 0.0f && tg[q] == 0.0f));
            if (live && pos[q] >= limit) { if (!loop) live = false; else pos[q] = (double)ostart; }
            if (live) {
                const uint32_t left = (uint32_t)pos[q];
                idx = left; frac = (float)(pos[q] - (double)left); g = gn[q];
                const bool settled = fabsf(tg[q] - gn[q]) <= FLT_EPSILON;
                pos[q] = pos[q] + (double)rate;
                gn[q] = settled ? tg[q] : gn[q] + alpha * (tg[q] - gn[q]);
                gn[q] = clampf(gn[q], 0.0f, 1.0f);
            }
            const uint32_t w = m.scratch + (uint32_t)q * 3u * kSlotWords + i;
            lds[w] = u2f(idx); lds[w + kSlotWords] = frac; lds[w + 2u * kSlotWords] = g;
        }
        ++i;
        return 0.0f;
    });
    r[rec::SMP_CHANGE] = f2u(chg); r[rec::SMP_CURRENT] = cur; r[rec::SMP_HAVE] = 1;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        rup rr = r + rec::SMP_READER0 + q * rec::SMP_READER_DWORDS;
        rr[0] = f2u(tg[q]); rr[1] = f2u(gn[q]); rec_st_f64(rr, 2, pos[q]);
    }
}

// PolyBlepOscillatorNode (Oscillators.h:19-94)
__device__ __forceinline__ float blep(float phase, float inc) {
    // the two correction branches (:23-33) share their one division: same operations on the same values, half the
    // divide sequences in a wave where some lane takes either branch
    const bool lo = phase < inc, hi = !lo && phase > (1.0f - inc);
    if (!(lo || hi)) return 0.0f;
    const float p = (lo ? phase : phase - 1.0f) / inc;
    return lo ? (2.0f - p) * p - 1.0f : (p + 2.0f) * p + 1.0f;
}

// serial part: only `phase += inc; if (phase >= 1) phase -= 1`. The out slot carries inc[t] in
// (from the pre-pass) and the pre-tick phase[t] out (for the post-pass).
__device__ __forceinline__ void ser_blep_phase(const Ctx& c, const Member& m, uint32_t cm) {
    rup r = c.recs + m.rec * kRecDwords;
    float phase = u2f(r[rec::S0]);
    if (cm & 1u) {
        // constant frequency: the increment is one scalar, no pre-pass, nothing to load
        const float inc = lds[opnd_lane(c, m, 0) & kOpValMask] / c.srF;
        const SIn in[1] = {sin_const(inc)};
        if (inc >= 0.0f && inc < 1.0f && phase >= 0.0f && phase < 1.0f) {
            // t = phase + inc lies in [0, 2): `if (t >= 1) t -= 1` == t - floor(t) exactly == v_fract_f32
            chain_blocks_m<1, 1u>(c, in, sout_of(c, m), [&](const float (&x)[1]) {
                const float y = phase;
                phase = __builtin_amdgcn_fractf(phase + x[0]);
                return y;
            });
        } else {
            chain_blocks_m<1, 1u>(c, in, sout_of(c, m), [&](const float (&x)[1]) {
                const float y = phase;
                phase += x[0];
                if (phase >= 1.0f) phase -= 1.0f;
                return y;
            });
        }
    } else {
        const SIn in[1] = {sin_lds(m.outLds)};
        chain_loop_m<1, 0u>(in, sout_lds(m.outLds), c.n, [&](const float (&x)[1]) {
            const float y = phase;
            phase += x[0];
            if (phase >= 1.0f) phase -= 1.0f;
            return y;
        });
    }
    r[rec::S0] = f2u(phase);
}

// OP_PHASE (device.h): a `phasor` lane or the phase half of a blepsaw / blepsquare lane, both with a constant frequency.
// Per lane its own node's increment formula; the loop is shared. The fast form needs every lane's phase and increment in
// range (otherwise each lane runs its node's general expressions: same values, more instructions).
__device__ __forceinline__ void ser_phase(const Ctx& c, const Member& m, bool blepLane) {
    rup r = c.recs + m.rec * kRecDwords;
    float phase = u2f(r[rec::S0]);
    const float f = sin_of(c, opnd_lane(c, m, 0)).cval;
    const float rsr = 1.0f / c.srF;
    const float inc = blepLane ? f / c.srF : f * rsr;
    const bool fast = blepLane ? (inc >= 0.0f && inc < 1.0f && phase >= 0.0f && phase < 1.0f) : (inc >= 0.0f && phase >= 0.0f);
    const SIn in[1] = {sin_const(inc)};
    if (__all(fast)) {
        // phasor: next >= 0, so next - floor(next) is exactly v_fract_f32(next); oscillator: t = phase + inc lies in [0, 2), where
        // `if (t >= 1) t -= 1` is t - floor(t) exactly as well
        chain_blocks_m<1, 1u>(c, in, sout_of(c, m), chain_step<true>([&](const float (&x)[1]) {   // (two VALU ops per frame: written out)
            const float y = phase;
            phase = __builtin_amdgcn_fractf(phase + x[0]);
            return y;
        }, [&](auto&& g) { g(phase); }));
    } else {
        chain_blocks_m<1, 1u>(c, in, sout_of(c, m), chain_step([&](const float (&x)[1]) {
            const float y = phase;
            const float t = phase + x[0];
            phase = blepLane ? (t >= 1.0f ? t - 1.0f : t) : t - floorf(t);
            return y;
        }, [&](auto&& g) { g(phase); }));
    }
    r[rec::S0] = f2u(phase);
}

__device__ __forceinline__ void ser_blep_acc(const Ctx& c, const Member& m) {   // triangle integrator (:58-59)
    rup r = c.recs + m.rec * kRecDwords;
    float acc = u2f(r[rec::S1]);
    const SIn in[1] = {sin_lds(m.outLds)};
    chain_loop<1>(in, 0u, sout_lds(m.outLds), c.n, [&](const float (&x)[1]) { acc += x[0]; return acc; });
    r[rec::S1] = f2u(acc);
}

// ---- double-state filters as wave scans -----------------------------------------------------------
// SVF / shelf / mm1p keep their state in double in the reference (filters/SVF.h:112-120,
// MultiMode1p.h:110); their per-sample update is an affine map of the state whose coefficients
// depend only on the inputs, so one wave evaluates a whole block as a scan of affine maps:
// lane l owns samples [8l, 8l+8), composes them locally, a 6-step Kogge-Stone scan over the 64
// lane aggregates yields each lane's incoming state, and the lane then replays its 8 samples to
// form the outputs. Re-association moves results by O(1e-16) relative — far inside the 1e-6 bar
// for these (stable, contractive) recurrences — and removes the 512-step f64 dependency chain.
struct Aff2 { double m11, m12, m21, m22, q1, q2; };   // s' = M s + q

__device__ __forceinline__ Aff2 aff2_after(const Aff2& f, const Aff2& g) {   // apply f, then g
    Aff2 r;
    r.m11 = g.m11 * f.m11 + g.m12 * f.m21; r.m12 = g.m11 * f.m12 + g.m12 * f.m22;
    r.m21 = g.m21 * f.m11 + g.m22 * f.m21; r.m22 = g.m21 * f.m12 + g.m22 * f.m22;
    r.q1 = g.m11 * f.q1 + g.m12 * f.q2 + g.q1;
    r.q2 = g.m21 * f.q1 + g.m22 * f.q2 + g.q2;
    return r;
}
__device__ __forceinline__ double shfl_up_f64(double v, int d) {
    const int lo = __shfl_up(__double2loint(v), d), hi = __shfl_up(__double2hiint(v), d);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double shfl_f64(double v, int l) {
    const int lo = __shfl(__double2loint(v), l), hi = __shfl(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// Exclusive scan over lanes of per-lane aggregates; returns the composition of lanes [0, lane).
__device__ __forceinline__ Aff2 aff2_exclusive_scan(Aff2 a, uint32_t lane, Aff2& total) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        Aff2 p;
        p.m11 = shfl_up_f64(a.m11, d); p.m12 = shfl_up_f64(a.m12, d); p.m21 = shfl_up_f64(a.m21, d);
        p.m22 = shfl_up_f64(a.m22, d); p.q1 = shfl_up_f64(a.q1, d); p.q2 = shfl_up_f64(a.q2, d);
        if (lane >= (uint32_t)d) a = aff2_after(p, a);
    }
    total.m11 = shfl_f64(a.m11, 63); total.m12 = shfl_f64(a.m12, 63); total.m21 = shfl_f64(a.m21, 63);
    total.m22 = shfl_f64(a.m22, 63); total.q1 = shfl_f64(a.q1, 63); total.q2 = shfl_f64(a.q2, 63);
    Aff2 e;
    e.m11 = shfl_up_f64(a.m11, 1); e.m12 = shfl_up_f64(a.m12, 1); e.m21 = shfl_up_f64(a.m21, 1);
    e.m22 = shfl_up_f64(a.m22, 1); e.q1 = shfl_up_f64(a.q1, 1); e.q2 = shfl_up_f64(a.q2, 1);
    if (lane == 0) { e.m11 = 1.0; e.m12 = 0.0; e.m21 = 0.0; e.m22 = 1.0; e.q1 = 0.0; e.q2 = 0.0; }
    return e;
}

// SVF / shelf coefficient pre-pass (updateCoeffs, filters/SVF.h:72-80, SVFShelf.h:66-83): the
// double tan / pow / divisions are the expensive, state-free part, so they run sample-parallel on
// every free wave one stage before the scan and land in the member's scratch as doubles:
// a1,a2,a3 (svf) or a1,a2,a3,k,A (shelf), each array spanning two float slots.
// tan on (0, pi/2) — the only range the clamped cutoff reaches (pi * [20, sr / 2.0001] / sr): sine and cosine Taylor
// polynomials on [0, pi/4] (x <= pi/4) or of pi/2 - x (then the quotient is flipped), one division. Within 2 ulp of libm
// over the whole range (checked against glibc on 400 k cutoffs), a third of the instructions of the general-argument tan —
// the pre-pass is the heaviest sample-parallel task of a filter voice.
__device__ __forceinline__ double tan_q1(double x) {
    const bool inv = x > 0.7853981633974483;
    const double y = inv ? (1.5707963267948966 - x) + 6.123233995736766e-17 : x;
    const double z = y * y;
    double sn = -7.647163731819816e-13;   // -1/15!
    sn = __builtin_fma(sn, z, 1.6059043836821613e-10);   //  1/13!
    sn = __builtin_fma(sn, z, -2.505210838544172e-08);   // -1/11!
    sn = __builtin_fma(sn, z, 2.7557319223985893e-06);   //  1/9!
    sn = __builtin_fma(sn, z, -1.984126984126984e-04);   // -1/7!
    sn = __builtin_fma(sn, z, 8.333333333333333e-03);   //  1/5!
    sn = __builtin_fma(sn, z, -1.6666666666666666e-01);   // -1/3!
    sn = __builtin_fma(sn, z, 1.0);
    sn = sn * y;
    double cs = 4.779477332387385e-14;   //  1/16!
    cs = __builtin_fma(cs, z, -1.1470745597729725e-11);   // -1/14!
    cs = __builtin_fma(cs, z, 2.08767569878681e-09);   //  1/12!
    cs = __builtin_fma(cs, z, -2.755731922398589e-07);   // -1/10!
    cs = __builtin_fma(cs, z, 2.48015873015873e-05);   //  1/8!
    cs = __builtin_fma(cs, z, -1.388888888888889e-03);   // -1/6!
    cs = __builtin_fma(cs, z, 4.1666666666666664e-02);   //  1/4!
    cs = __builtin_fma(cs, z, -0.5);
    cs = __builtin_fma(cs, z, 1.0);
    return inv ? cs / sn : sn / cs;
}

template <bool Shelf, int V>
__device__ __forceinline__ void run_svf_coef(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim) {
    if (member_nin(c, m) < (Shelf ? 4u : 3u)) return;
    const uint32_t mode = Shelf ? UNI(c.recs[m.rec * kRecDwords + rec::P0]) : 0u;
    double* A1 = reinterpret_cast<double*>(lds + m.scratch);
    double* A2 = A1 + kSlotWords; double* A3 = A2 + kSlotWords;
    double* KK = A3 + kSlotWords; double* AA = KK + kSlotWords;
    const double sr = c.sr;
    float fcv[V], qv[V], gv[V];
    const uint32_t oF = opnd_uniform(c, m, 0), oQ = opnd_uniform(c, m, 1);
    vload<V>(pin_of(c, oF), i, fcv);
    vload<V>(pin_of(c, oQ), i, qv);
    if (Shelf) vload<V>(pin_of(c, opnd_uniform(c, m, 2)), i, gv);
    // a cutoff / resonance that is a broadcast cell (or absent) is the same for every frame: evaluate its tan /
    // reciprocal once per call instead of once per frame — the same double operations on the same values
    const bool constF = ((oF >> 30) & 1u) != 0u, constQ = ((oQ >> 30) & 1u) != 0u;
    double gC = 0.0, kC = 0.0, a1C = 0.0, a2C = 0.0, a3C = 0.0;
    if (constF) gC = tan_q1(3.14159265359 * clampd((double)fcv[0], 20.0, sr / 2.0001) / sr);
    if (constQ) kC = 1.0 / clampd((double)qv[0], 0.25, 20.0);
    const bool constAll = !Shelf && constF && constQ;
    if (constAll) { a1C = 1.0 / (1.0 + gC * (gC + kC)); a2C = gC * a1C; a3C = gC * a2C; }
#pragma unroll
    for (int q_ = 0; q_ < V; ++q_) {
        const uint32_t t = i + q_;
        if (constAll) { if (t < nlim) { A1[t] = a1C; A2[t] = a2C; A3[t] = a3C; } continue; }
        const double fc = (double)fcv[q_], q = (double)qv[q_];
        double g = constF ? gC : tan_q1(3.14159265359 * clampd(fc, 20.0, sr / 2.0001) / sr);
        double k = constQ ? kC : 1.0 / clampd(q, 0.25, 20.0);
        if (Shelf) {
            const double A = pow(10.0, (double)gv[q_] / 40.0);
            if (mode == 0) g /= A;
            if (mode == 1) g *= A;
            if (mode == 2) k /= A;
            if (t < nlim) { KK[t] = k; AA[t] = A; }
        }
        const double a1 = 1.0 / (1.0 + g * (g + k));
        const double a2 = g * a1;
        if (t < nlim) { A1[t] = a1; A2[t] = a2; A3[t] = g * a2; }
    }
}

// StateVariableFilterNode (filters/SVF.h:48-105) and StateVariableShelfFilterNode
// (filters/SVFShelf.h:44-124), whole wave on one node.
//   tick:  v3 = v0 - ic2; v1 = ic1*a1 + v3*a2; v2 = ic2 + ic1*a2 + v3*a3; ic1 = 2 v1 - ic1; ic2 = 2 v2 - ic2
//   =>     ic1' = (2a1-1) ic1 - 2a2 ic2 + 2a2 v0 ;  ic2' = 2a2 ic1 + (1-2a3) ic2 + 2a3 v0
template <bool Shelf>
__device__ __forceinline__ void scan_svf(const Ctx& c, const Member& m) {
    rup r = c.recs + m.rec * kRecDwords;
    const uint32_t n = c.n, need = Shelf ? 4u : 3u;
    if (member_nin(c, m) < need) { for (uint32_t i = c.lane; i < n; i += 64) lds[m.outLds + i] = 0.0f; return; }
    const uint32_t mode = UNI(r[rec::P0]);
    const PIn pQ = pin_of(c, opnd_uniform(c, m, 1));
    const PIn pX = pin_of(c, opnd_uniform(c, m, Shelf ? 3 : 2));
    const double* A1 = reinterpret_cast<const double*>(lds + m.scratch);
    const double* A2 = A1 + kSlotWords; const double* A3 = A2 + kSlotWords;
    const double* KK = A3 + kSlotWords; const double* AA = KK + kSlotWords;
    const uint32_t t0 = c.lane * 8u;
    double a1[8], a2[8], a3[8], v0[8];
    // `fuse_svf_coef` plans (plan.cpp) give an svf no coefficient pre-pass and no scratch: every lane evaluates updateCoeffs
    // (filters/SVF.h:72-80) for its own 8 frames here — the same double operations on the same values as run_svf_coef, so the
    // two forms are bit-identical; the island saves 6 of a filter voice's 10 LDS block buffers, which is what lets K lane-packed
    // voices keep a deep block pipeline.
    const bool fusedCoef = !Shelf && m.scratch == kNone;
    if (fusedCoef) {
        const PIn pF = pin_of(c, opnd_uniform(c, m, 0));
        const double sr = c.sr;
        const bool constF = !pF.isG && pF.step == 0u, constQ = !pQ.isG && pQ.step == 0u;
        double gC = 0.0, kC = 0.0;
        if (constF) gC = tan_q1(3.14159265359 * clampd((double)lds[pF.base], 20.0, sr / 2.0001) / sr);
        if (constQ) kC = 1.0 / clampd((double)lds[pQ.base], 0.25, 20.0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t t = t0 + j;
            const uint32_t tt = t < n ? t : 0u;          // (frames past the block: any in-range frame, the results are not used)
            const double g = constF ? gC : tan_q1(3.14159265359 * clampd((double)(pF.isG ? pF.g[tt] : lds[pF.base + tt * pF.step]), 20.0, sr / 2.0001) / sr);
            const double k = constQ ? kC : 1.0 / clampd((double)(pQ.isG ? pQ.g[tt] : lds[pQ.base + tt * pQ.step]), 0.25, 20.0);
            a1[j] = 1.0 / (1.0 + g * (g + k));
            a2[j] = g * a1[j];
            a3[j] = g * a2[j];
        }
    }
    {   // lane-owned 8 samples: 16-byte LDS reads
        if (!fusedCoef) {
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            const v2d p1 = ld2d(&A1[t0 + j]);
            const v2d p2 = ld2d(&A2[t0 + j]);
            const v2d p3 = ld2d(&A3[t0 + j]);
            a1[j] = p1.x; a1[j + 1] = p1.y; a2[j] = p2.x; a2[j + 1] = p2.y; a3[j] = p3.x; a3[j + 1] = p3.y;
        }
        }
        if (pX.isG) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v0[j] = (double)pX.g[t0 + j];
        } else if (pX.step) {
            const v4f xa = ld4(pX.base + t0);
            const v4f xb = ld4(pX.base + t0 + 4);
            v0[0] = xa.x; v0[1] = xa.y; v0[2] = xa.z; v0[3] = xa.w; v0[4] = xb.x; v0[5] = xb.y; v0[6] = xb.z; v0[7] = xb.w;
        } else {
            const double x = (double)lds[pX.base];
#pragma unroll
            for (int j = 0; j < 8; ++j) v0[j] = x;
        }
    }
    Aff2 agg; agg.m11 = 1.0; agg.m12 = 0.0; agg.m21 = 0.0; agg.m22 = 1.0; agg.q1 = 0.0; agg.q2 = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (t0 + j < n) {
            Aff2 s;
            s.m11 = 2.0 * a1[j] - 1.0; s.m12 = -2.0 * a2[j];
            s.m21 = 2.0 * a2[j];       s.m22 = 1.0 - 2.0 * a3[j];
            s.q1 = 2.0 * a2[j] * v0[j]; s.q2 = 2.0 * a3[j] * v0[j];
            agg = aff2_after(agg, s);
        }
    }
    Aff2 total;
    const Aff2 pre = aff2_exclusive_scan(agg, c.lane, total);
    const double s1 = rec_ld_f64(r, rec::S0), s2 = rec_ld_f64(r, rec::S2);
    double ic1 = pre.m11 * s1 + pre.m12 * s2 + pre.q1;
    double ic2 = pre.m21 * s1 + pre.m22 * s2 + pre.q2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t t = t0 + j;
        if (t < n) {
            const double v3 = v0[j] - ic2;
            const double v1 = ic1 * a1[j] + v3 * a2[j];
            const double v2 = ic2 + ic1 * a2[j] + v3 * a3[j];
            ic1 = v1 * 2.0 - ic1;
            ic2 = v2 * 2.0 - ic2;
            float y;
            if (!Shelf) {   // SVF.h:57-69
                if (mode == 0)      y = (float)v2;
                else if (mode == 1) y = (float)v1;
                else {
                    const float qf = pQ.isG ? pQ.g[t] : lds[pQ.base + t * pQ.step];
                    const double k = 1.0 / clampd((double)qf, 0.25, 20.0);
                    if (mode == 2)      y = (float)(v0[j] - k * v1 - v2);
                    else if (mode == 3) y = (float)(v0[j] - k * v1);
                    else                y = (float)(v0[j] - 2.0 * k * v1);
                }
            } else {        // SVFShelf.h:54-63
                const double A = AA[t], k = KK[t];
                if (mode == 2)      y = (float)(v0[j] + k * (A * A - 1.0) * v1);
                else if (mode == 0) y = (float)(v0[j] + k * (A - 1.0) * v1 + (A * A - 1.0) * v2);
                else                y = (float)(A * A * v0[j] + k * (1.0 - A) * A * v1 + (1.0 - A * A) * v2);
            }
            lds[m.outLds + t] = y;
        }
    }
    if (c.lane == 0) {
        rec_st_f64(r, rec::S0, total.m11 * s1 + total.m12 * s2 + total.q1);
        rec_st_f64(r, rec::S2, total.m21 * s1 + total.m22 * s2 + total.q2);
    }
}

// MultiMode1p (filters/MultiMode1p.h:79-107): v = (x - z) G; lp = v + z; z' = lp + v
//   =>  z' = (1 - 2G) z + 2G x  (1-D affine scan); lp is formed from the pre-sample state.
__device__ __forceinline__ void scan_mm1p(const Ctx& c, const Member& m) {
    rup r = c.recs + m.rec * kRecDwords;
    const uint32_t n = c.n;
    if (member_nin(c, m) < 2) { for (uint32_t i = c.lane; i < n; i += 64) lds[m.outLds + i] = 0.0f; return; }
    const uint32_t mode = UNI(r[rec::P0]);
    const PIn pGn = pin_of(c, opnd_uniform(c, m, 0)), pX = pin_of(c, opnd_uniform(c, m, 1));
    const uint32_t t0 = c.lane * 8u;
    double G[8]; float xs[8];
    double am = 1.0, aq = 0.0;   // z' = am z + aq over this lane's samples
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t t = t0 + j;
        const bool live = t < n;
        const uint32_t tc = live ? t : 0u;
        auto rd = [&](const PIn& p) { return p.isG ? p.g[tc] : lds[p.base + tc * p.step]; };
        const double g = clampd((double)rd(pGn), 0.0, 0.9999);
        G[j] = g / (1.0 + g);
        xs[j] = rd(pX);
        if (live) {
            const double mm = 1.0 - 2.0 * G[j], qq = 2.0 * G[j] * (double)xs[j];
            am = mm * am; aq = mm * aq + qq;
        }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double pm = shfl_up_f64(am, d), pq = shfl_up_f64(aq, d);
        if (c.lane >= (uint32_t)d) { aq = am * pq + aq; am = am * pm; }
    }
    const double tm = shfl_f64(am, 63), tq = shfl_f64(aq, 63);
    double em = shfl_up_f64(am, 1), eq = shfl_up_f64(aq, 1);
    if (c.lane == 0) { em = 1.0; eq = 0.0; }
    const double z0 = rec_ld_f64(r, rec::S0);
    double z = em * z0 + eq;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t t = t0 + j;
        if (t < n) {
            const float xn = xs[j];
            const double v = ((double)xn - z) * G[j];
            const double lp = v + z;
            z = lp + v;
            float y;
            if (mode == 0)      y = (float)lp;
            else if (mode == 2) y = xn - (float)lp;
            else                y = (float)(lp + lp - (double)xn);
            lds[m.outLds + t] = y;
        }
    }
    if (c.lane == 0) rec_st_f64(r, rec::S0, tm * z0 + tq);
}


// blepsaw / blepsquare waveform (Oscillators.h:36-57) from the pre-tick phase the recurrence task left in
// the out slot and the frequency operand; in place, sample-parallel (any wave, any frame range).
template <bool Square, int V>
__device__ __forceinline__ void run_blep_shape(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim) {
    if (member_nin(c, m) < 1) return vzero<V>(c, m, i, nlim);
    const uint32_t o = opnd_uniform(c, m, 0);
    float f[V], ph[V];
    vload<V>(pin_of(c, o), i, f);
#ifdef ELEMHIP_SPEC   // the phase recurrence may have streamed its block to the HBM arena (member operand slot 5 names the buffer)
    vload<V>((m.sops[5] & kOpKindMask) == kOpHbm ? pin_of(c, m.sops[5]) : PIn{m.outLds, 1u, (gcfp)nullptr, false}, i, ph);
#else
    vload<V>(PIn{m.outLds, 1u, (gcfp)nullptr, false}, i, ph);
#endif
    const float sr = c.srF;
    // a constant frequency (broadcast cell) has one increment for the whole block: divide once
    const bool constF = ((o >> 30) & 1u) != 0u;
    const float incU = constF ? f[0] / sr : 0.0f;
#pragma unroll
    for (int q = 0; q < V; ++q) {
        const float inc = constF ? incU : f[q] / sr;
        const float phase = ph[q];
        if (!Square) ph[q] = 2.0f * phase - 1.0f - blep(phase, inc);
        else {
            const float naive = phase < 0.5f ? 1.0f : -1.0f;
            const float halfPhase = fmodf(phase + 0.5f, 1.0f);
            ph[q] = naive + blep(phase, inc) - blep(halfPhase, inc);
        }
    }
    vstore<V>(c, m, i, nlim, ph);
}

} // namespace (ops)
