// island.inc — the interpreter build of the island kernel (program tables read from LDS at run time), the epilogue /
// patch kernels and the host launchers. The op bodies live in island_ops.inc.
#include "island_ops.inc"

namespace {

// ---- task dispatch ------------------------------------------------------------------------------
struct TaskU { uint32_t opcode, stage, flags, s0, s1, first, count, o0, o1, outLds, nin, outHbm; };

// Visit the members of a task (wave-uniform). Sample-parallel math ops of a single-member task
// (`lite`) take everything from the task header; other ops also need the member's record / scratch.
template <bool Lite, typename F>
__device__ __forceinline__ void for_members_x(const Ctx& c, const TaskU& t, F&& f) {
    if (Lite && t.count == 1 && t.nin != 0xFFFEu) {
        Member m;
        m.rec = kNone; m.opnd = kNone; m.scratch = kNone;
        m.nin = t.nin == 0xFFFFu ? (uint32_t)kNone : t.nin;
        m.outLds = t.outLds == 0xFFFFu ? (uint32_t)kNone : t.outLds;
        m.outHbm = t.outHbm; m.pad0_ = t.o0; m.pad1_ = t.o1;
        if (m.nin > 2u && m.nin != kNone) {   // operands beyond the inlined two live in the table
            m.opnd = UNI(ldsu(c.members + t.first * 8u + 1u));
        } else if (m.nin == kNone) {
            m.opnd = UNI(ldsu(c.members + t.first * 8u + 1u));
        }
        f(m);
        return;
    }
    for (uint32_t k = 0; k < t.count; ++k) { const Member m = member_uniform(c, t.first + k); f(m); }
}
template <typename F>
__device__ __forceinline__ void for_members(const Ctx& c, const TaskU& t, F&& f) { for_members_x<false>(c, t, f); }

// Stateful task: whole-wave scans for the double-state filters; otherwise a sample-parallel
// pre-pass over all members, the lane-per-member chain, and a sample-parallel post-pass.
__device__ __forceinline__ void run_stateful(const Ctx& c, const TaskU& t) {
    const uint32_t n = c.n;
    const uint32_t op = t.opcode;
    const uint32_t cm = t.flags & 0x3Fu;   // bit 6: kTaskOwnsWave
    if (op == OP_SVF || op == OP_SVFSHELF || op == OP_MM1P) {
        for_members(c, t, [&](const Member& m) {
            if (op == OP_SVF) scan_svf<false>(c, m);
            else if (op == OP_SVFSHELF) scan_svf<true>(c, m);
            else scan_mm1p(c, m);
        });
    } else {
        const bool isBlep = (op == OP_BLEPSAW || op == OP_BLEPSQUARE || op == OP_BLEPTRIANGLE);
        if (isBlep && !(cm & 1u)) {   // pre-pass: inc[t] = f/sr into the out slot (skipped for a constant frequency)
            const float sr = c.srF;
            for_members(c, t, [&](const Member& m) {
                if (member_nin(c, m) < 1) return;
                const PIn p = pin_of(c, opnd_uniform(c, m, 0));
                if (n == 512) {   // full block: 8 consecutive frames per lane, vector LDS traffic
                    float x[8];
                    vload<8>(p, c.lane * 8u, x);
                    v4f a, b;
                    a.x = x[0] / sr; a.y = x[1] / sr; a.z = x[2] / sr; a.w = x[3] / sr;
                    b.x = x[4] / sr; b.y = x[5] / sr; b.z = x[6] / sr; b.w = x[7] / sr;
                    st4(m.outLds + c.lane * 8u, a); st4(m.outLds + c.lane * 8u + 4u, b);
                } else {
                    for (uint32_t i = c.lane; i < n; i += 64) lds[m.outLds + i] = pget(p, i) / sr;
                }
            });
            WAVE_SYNC();
        }
        if (c.lane < t.count && n > 0) {
            const Member m = member_lane(c, t.first + c.lane);
            switch (op) {
                case OP_PHASOR:   ser_phasor(c, m, cm); break;
                case OP_SPHASOR:  ser_sphasor(c, m, cm); break;
                case OP_POLE:     ser_pole(c, m, cm); break;
                case OP_ENV:      ser_env(c, m, cm); break;
                case OP_BIQUAD:   ser_biquad(c, m, cm); break;
                case OP_COUNTER:  ser_counter(c, m, cm); break;
                case OP_ACCUM:    ser_accum(c, m, cm); break;
                case OP_LATCH:    ser_latch(c, m, cm); break;
                case OP_MAXHOLD:  ser_maxhold(c, m, cm); break;
                case OP_ONCE:     ser_once(c, m, cm); break;
                case OP_SEQ:      ser_seq(c, m, cm); break;
                case OP_SEQ2:     ser_seq2(c, m, cm); break;
                case OP_SPARSEQ:  ser_sparseq(c, m, cm); break;
                case OP_SAMPLE:   ser_sample(c, m, cm); break;
                case OP_MCSAMPLE: ser_mcsample(c, m, cm); break;
                case OP_BLEPSAW: case OP_BLEPSQUARE: case OP_BLEPTRIANGLE:
                    if (member_nin(c, m) < 1) szero(m, n); else ser_blep_phase(c, m, cm);
                    break;
                case OP_PHASE: ser_phase(c, m, c.lane >= t.s0); break;
                default: break;
            }
        }
        WAVE_SYNC();
        if (op == OP_MCSAMPLE) for_members(c, t, [&](const Member& m) { gather_mcsample(c, m); });
        if (op == OP_SAMPLE) {   // gather pass (VariablePitchLerpReader::tick :196-211): both readers, linear interpolation, frame-parallel
            for_members(c, t, [&](const Member& m) {
                rcup r = c.recs + m.rec * kRecDwords;
                gcfp buf = rec_ptr(r, rec::SMP_BUF);
                const uint32_t len = UNI(r[rec::SMP_LEN]);
                for (uint32_t i = c.lane; i < n; i += 64) {
                    float acc = 0.0f;
#pragma unroll
                    for (uint32_t q = 0; q < 2; ++q) {
                        const uint32_t w = m.scratch + q * 3u * kSlotWords + i;
                        const uint32_t idx = ldsu(w);
                        float y = 0.0f;
                        if (idx != 0xFFFFFFFFu && buf && len) {
                            uint32_t l = idx, rr = idx + 1u;
                            if (l >= len) l -= len;
                            if (rr >= len) rr -= len;
                            if (l >= len) l %= len;          // the reference reads out of bounds here (start offset beyond the buffer)
                            if (rr >= len) rr %= len;
                            const float left = buf[l], right = buf[rr];
                            y = lds[w + 2u * kSlotWords] * (left + lds[w + kSlotWords] * (right - left));
                        }
                        acc = q == 0u ? y : acc + y;
                    }
                    lds[m.outLds + i] = acc;
                }
            });
        }
        if (op == OP_BLEPTRIANGLE) {   // post-pass: waveform from (phase, inc); saw / square have theirs as a task of the next stage (run_blep_shape)
            const float sr = c.srF;
            for_members(c, t, [&](const Member& m) {
                if (member_nin(c, m) < 1) return;
                const PIn p = pin_of(c, opnd_uniform(c, m, 0));
                // a constant frequency (broadcast cell, task flag bit 0) has one increment for the whole block: divide once
                const bool constF = (cm & 1u) != 0u;
                const float incU = constF ? pget(p, 0) / sr : 0.0f;
                auto wave = [&](float f, float phase) {
                    const float inc = constF ? incU : f / sr;
                    const float naive = phase < 0.5f ? 1.0f : -1.0f;
                    const float halfPhase = fmodf(phase + 0.5f, 1.0f);
                    const float square = naive + blep(phase, inc) - blep(halfPhase, inc);
                    return 4.0f * inc * square;
                };
                if (n == 512) {
                    float f[8], ph[8];
                    vload<8>(p, c.lane * 8u, f);
                    vload<8>(PIn{m.outLds, 1u, (gcfp)nullptr, false}, c.lane * 8u, ph);
                    v4f a, b;
                    a.x = wave(f[0], ph[0]); a.y = wave(f[1], ph[1]); a.z = wave(f[2], ph[2]); a.w = wave(f[3], ph[3]);
                    b.x = wave(f[4], ph[4]); b.y = wave(f[5], ph[5]); b.z = wave(f[6], ph[6]); b.w = wave(f[7], ph[7]);
                    st4(m.outLds + c.lane * 8u, a); st4(m.outLds + c.lane * 8u + 4u, b);
                } else {
                    for (uint32_t i = c.lane; i < n; i += 64) lds[m.outLds + i] = wave(pget(p, i), lds[m.outLds + i]);
                }
            });
            WAVE_SYNC();
            if (c.lane < t.count && n > 0) {
                const Member m = member_lane(c, t.first + c.lane);
                if (member_nin(c, m) >= 1) ser_blep_acc(c, m);
            }
        }
    }
    WAVE_SYNC();
    if (op == OP_BLEPSAW || op == OP_BLEPSQUARE) return;   // the out slot holds the phase; the shape task exports
    // chain outputs are produced in LDS; copy out the ones another island (or the epilogue) reads
    // (OP_PHASE: only its phasor members, the first s0; an oscillator member's out slot holds the phase for its shape task)
    const uint32_t exporting = op == OP_PHASE ? t.s0 : t.count;
    for (uint32_t k = 0; k < exporting; ++k) {
        const Member m = member_uniform(c, t.first + k);
        if (m.outHbm == kNone) continue;
        for (uint32_t i = c.lane; i < n; i += 64) hbm_buf(c, m.outHbm)[i] = lds[m.outLds + i];
    }
}

// Fast path for the overwhelmingly common sample-parallel task: one node, one or two operands that
// all live in LDS (buffers / broadcast cells), enough inputs for the node's arity. The planner
// marks such tasks (flags bit 7); everything they need is in the 8-dword header, so there is no
// operand-kind decoding and no member/operand table access: load, apply, store.
template <int V>
__device__ __forceinline__ void fast_load(uint32_t o, uint32_t i, float (&x)[V]) {
    const uint32_t w = o & kOpValMask;
    if ((o >> 30) == 0u) {
        if constexpr (V == 1) x[0] = lds[w + i];
        else if constexpr (V == 2) { const v2f a = *reinterpret_cast<const v2f*>(__builtin_assume_aligned(&lds[w + i], 8)); x[0] = a.x; x[1] = a.y; }
        else {
#pragma unroll
            for (int q = 0; q < V; q += 4) { const v4f a = ld4(w + i + q); x[q] = a.x; x[q + 1] = a.y; x[q + 2] = a.z; x[q + 3] = a.w; }
        }
    } else {
        const float v = lds[(o >> 30) == 1u ? w : 0u];
#pragma unroll
        for (int q = 0; q < V; ++q) x[q] = v;
    }
}

template <int V>
__device__ __forceinline__ void run_fast(const Ctx& c, const TaskU& t, uint32_t i) {
    float x[V], y[V];
    fast_load<V>(t.o0, i, x);
    const uint32_t op = t.opcode;
    if (op >= OP_LE) {   // binary / two-operand reduce: one switch per task, straight-line loops inside each case
        fast_load<V>(t.o1, i, y);
        switch (op) {
#define FB(OPC, EXPR) case OPC: _Pragma("unroll") for (int q = 0; q < V; ++q) x[q] = (EXPR); break;
            FB(OP_ADD, x[q] + y[q]) FB(OP_SUB, x[q] - y[q]) FB(OP_MUL, x[q] * y[q])
            FB(OP_DIV, reduce_eval(OP_DIV, x[q], y[q])) FB(OP_MIN, reduce_eval(OP_MIN, x[q], y[q])) FB(OP_MAX, reduce_eval(OP_MAX, x[q], y[q]))
            FB(OP_MOD, fmodf(x[q], y[q]))
            FB(OP_LE, binary_eval(OP_LE, x[q], y[q])) FB(OP_LEQ, binary_eval(OP_LEQ, x[q], y[q])) FB(OP_GE, binary_eval(OP_GE, x[q], y[q]))
            FB(OP_GEQ, binary_eval(OP_GEQ, x[q], y[q])) FB(OP_POW, binary_eval(OP_POW, x[q], y[q])) FB(OP_EQ, binary_eval(OP_EQ, x[q], y[q]))
            FB(OP_AND, binary_eval(OP_AND, x[q], y[q]))
            default: _Pragma("unroll") for (int q = 0; q < V; ++q) x[q] = binary_eval(OP_OR, x[q], y[q]); break;
#undef FB
        }
    } else {
        switch (op) {   // one switch per task, the loops inside each case are straight-line
#define FU(OPC) case OPC: _Pragma("unroll") for (int q = 0; q < V; ++q) x[q] = unary_eval(OPC, x[q]); break;
            FU(OP_SIN) FU(OP_COS) FU(OP_TAN) FU(OP_TANH) FU(OP_ASINH) FU(OP_LN) FU(OP_LOG) FU(OP_LOG2)
            FU(OP_CEIL) FU(OP_FLOOR) FU(OP_ROUND) FU(OP_SQRT) FU(OP_EXP)
            default: _Pragma("unroll") for (int q = 0; q < V; ++q) x[q] = fabsf(x[q]); break;
#undef FU
        }
    }
    if (t.outLds != 0xFFFFu) {
        const uint32_t w = t.outLds + i;
        if constexpr (V == 1) lds[w] = x[0];
        else if constexpr (V == 2) { v2f a; a.x = x[0]; a.y = x[1]; *reinterpret_cast<v2f*>(__builtin_assume_aligned(&lds[w], 8)) = a; }
        else {
#pragma unroll
            for (int q = 0; q < V; q += 4) { v4f a; a.x = x[q]; a.y = x[q + 1]; a.z = x[q + 2]; a.w = x[q + 3]; st4(w + q, a); }
        }
    }
    if (t.outHbm != kNone) {
        gfp g = c.hbm + (size_t)t.outHbm * c.stride + i;
        if constexpr (V == 1) g[0] = x[0];
        else if constexpr (V == 2) { v2f a; a.x = x[0]; a.y = x[1]; *(gv2)g = a; }
        else {
#pragma unroll
            for (int q = 0; q < V; q += 4) { v4f a; a.x = x[q]; a.y = x[q + 1]; a.z = x[q + 2]; a.w = x[q + 3]; *(gv4)(g + q) = a; }
        }
    }
}

// sample-parallel opcodes on the canonical mapping, V consecutive frames per lane
template <int V>
__device__ __forceinline__ void run_par(const Ctx& c, const TaskU& t, uint32_t i, uint32_t nlim) {
#define PAR(OPC, FN) case OPC: for_members(c, t, [&](const Member& m) { FN<V>(c, m, i, nlim); }); break;
#define UN(OPC)  case OPC: for_members_x<true>(c, t, [&](const Member& m) { run_unary<OPC, V>(c, m, i, nlim); }); break;
#define BI(OPC)  case OPC: for_members_x<true>(c, t, [&](const Member& m) { run_binary<OPC, V>(c, m, i, nlim); }); break;
#define RE(OPC)  case OPC: for_members_x<true>(c, t, [&](const Member& m) { run_reduce<OPC, V>(c, m, i, nlim); }); break;
    switch (t.opcode) {
        UN(OP_SIN) UN(OP_COS) UN(OP_TAN) UN(OP_TANH) UN(OP_ASINH) UN(OP_LN) UN(OP_LOG) UN(OP_LOG2)
        UN(OP_CEIL) UN(OP_FLOOR) UN(OP_ROUND) UN(OP_SQRT) UN(OP_EXP) UN(OP_ABS)
        BI(OP_LE) BI(OP_LEQ) BI(OP_GE) BI(OP_GEQ) BI(OP_POW) BI(OP_EQ) BI(OP_AND) BI(OP_OR)
        RE(OP_ADD) RE(OP_SUB) RE(OP_MUL) RE(OP_DIV) RE(OP_MOD) RE(OP_MIN) RE(OP_MAX)
        PAR(OP_IN, run_in) PAR(OP_COPY, run_copy) PAR(OP_ROOT, run_root) PAR(OP_PREWARP, run_prewarp)
        PAR(OP_TIME, run_time) PAR(OP_METRO, run_metro) PAR(OP_TAPIN, run_tapin) PAR(OP_TAPOUT, run_tapout)
        PAR(OP_TABLE, run_table) PAR(OP_SPARSEQ2, run_sparseq2)
        PAR(OP_CONST, run_fill) PAR(OP_SR, run_fill)
        case OP_SVF_COEF:   for_members(c, t, [&](const Member& m) { run_svf_coef<false, V>(c, m, i, nlim); }); break;
        case OP_SHELF_COEF: for_members(c, t, [&](const Member& m) { run_svf_coef<true, V>(c, m, i, nlim); }); break;
        case OP_SAW_SHAPE:    for_members(c, t, [&](const Member& m) { run_blep_shape<false, V>(c, m, i, nlim); }); break;
        case OP_SQUARE_SHAPE: for_members(c, t, [&](const Member& m) { run_blep_shape<true, V>(c, m, i, nlim); }); break;
        default: break;
    }
#undef PAR
#undef UN
#undef BI
#undef RE
}

__device__ __forceinline__ void run_task(const Ctx& c, const TaskU& t, uint32_t lo, uint32_t hi) {
    switch (t.opcode) {
        // whole-block, single-wave ops with their own state handling
        case OP_RAND:   for_members(c, t, [&](const Member& m) { run_rand(c, m, 0, c.n); }); return;
        case OP_Z:      for_members(c, t, [&](const Member& m) { run_z(c, m, 0, c.n); }); return;
        case OP_SDELAY: for_members(c, t, [&](const Member& m) { run_sdelay(c, m, 0, c.n); }); return;
        case OP_DELAY:  for_members(c, t, [&](const Member& m) { run_delay(c, m, 0, c.n); }); return;
        case OP_SAMPLESEQ: for_members(c, t, [&](const Member& m) { run_sampleseq(c, m, 0, c.n); }); return;
        case OP_METER:    for_members(c, t, [&](const Member& m) { run_meter(c, m, 0, c.n); }); return;
        case OP_SNAPSHOT: for_members(c, t, [&](const Member& m) { run_snapshot(c, m, 0, c.n); }); return;
        case OP_SCOPE:    for_members(c, t, [&](const Member& m) { run_scope(c, m, 0, c.n); }); return;
        case OP_FFT:      for_members(c, t, [&](const Member& m) { run_fft(c, m, 0, c.n); }); return;
        case OP_CAPTURE:  for_members(c, t, [&](const Member& m) { run_capture(c, m, 0, c.n); }); return;
        case OP_PHASOR: case OP_SPHASOR: case OP_COUNTER: case OP_ACCUM: case OP_LATCH: case OP_MAXHOLD: case OP_ONCE:
        case OP_SEQ: case OP_SEQ2: case OP_SPARSEQ: case OP_SAMPLE: case OP_MCSAMPLE: case OP_POLE: case OP_ENV: case OP_BIQUAD: case OP_MM1P: case OP_SVF: case OP_SVFSHELF:
        case OP_BLEPSAW: case OP_BLEPSQUARE: case OP_BLEPTRIANGLE: case OP_PHASE:
            run_stateful(c, t);
            return;
        default: break;
    }
    // sample-parallel: frames [s0, s1) of this workgroup's slice, 64*V of them
    const uint32_t s0 = max(t.s0, lo), s1 = min(t.s1, hi);
    if (s0 >= s1 || s0 >= c.n) return;
    const uint32_t V = (s1 - s0) >> 6;
    const uint32_t nlim = min(s1, c.n);
    const uint32_t i = s0 + c.lane * V;
    switch (V) {
        case 1: run_par<1>(c, t, i, nlim); break;
        case 2: run_par<2>(c, t, i, nlim); break;
        case 4:   // the heavy pre/post passes have a 4-frame body of their own; everything else runs as two 2-frame passes (same lane, same 4 frames)
            if (t.opcode == OP_SVF_COEF)          for_members(c, t, [&](const Member& m) { run_svf_coef<false, 4>(c, m, i, nlim); });
            else if (t.opcode == OP_SHELF_COEF)   for_members(c, t, [&](const Member& m) { run_svf_coef<true, 4>(c, m, i, nlim); });
            else if (t.opcode == OP_SAW_SHAPE)    for_members(c, t, [&](const Member& m) { run_blep_shape<false, 4>(c, m, i, nlim); });
            else if (t.opcode == OP_SQUARE_SHAPE) for_members(c, t, [&](const Member& m) { run_blep_shape<true, 4>(c, m, i, nlim); });
            else { run_par<2>(c, t, i, nlim); run_par<2>(c, t, i + 2, nlim); }
            break;
        case 8: run_par<8>(c, t, i, nlim); break;
        default: break;   // the planner only emits 64, 128, 256 or 512-frame ranges
    }
}

// RootNode::stillRunning (Core.h:28-31) and the channel test of RootRenderSequence::process
// (GraphRenderSequence.h:214-219)
__device__ __forceinline__ bool root_running(gcup recs, uint32_t rootRec, uint32_t numOut) {
    gcup r = recs + rootRec * kRecDwords;
    const float tg = u2f(r[rec::ROOT_TARGET]), g = u2f(r[rec::ROOT_GAIN]);
    const bool on = tg > 0.5f;
    const bool settled = fabsf(tg - g) <= 1e-6f;
    const int ch = (int)r[rec::ROOT_CHANNEL];
    return (on || !settled) && ch >= 0 && (uint32_t)ch < numOut;
}

} // namespace

// ---- kernels ---------------------------------------------------------------------------------------
// One launch renders one island level for `batch` consecutive blocks (1 = the realtime path).
//   * batch == 1, or a stateless island: stages are separated by workgroup barriers; a stateless island's
//     blocks are spread over gridDim.y (nothing carries over from block to block).
//   * stateful island, batch > 1: software pipeline over blocks. The island keeps `copies` (D) blocks in
//     flight, block b in buffer set b % D with its own program copy. The planner cuts the S stages into D phases
//     of consecutive stages (balanced by estimated cost); in macro-step m every wave runs its phase-p tasks of block m - p. A task of
//     stage s waits (LDS counters) until the previous non-empty stage of ITS block is complete and until
//     block b - D has left the pipeline, so its buffer set is free. Every wait refers to work of an earlier
//     macro/micro step and all waves walk the steps in the same order, so the schedule cannot deadlock.
//     Node state lives in the node records; the same wave renders a node for every block, in block order.
__device__ __forceinline__ void wait_counter(uint32_t word, uint32_t need) {
    uint32_t* p = reinterpret_cast<uint32_t*>(lds + word);
    while (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < need) __builtin_amdgcn_s_sleep(1);
}

// (resident.hip builds this body as a device function — one island of one block per call, the workgroup's place in the launch
// grid handed in — and walks a plan's levels itself; in the two kernel builds the ISL_* names ARE the launch grid's.)
#ifdef ELEMHIP_RESIDENT
#define ISL_BX islandIndex_
#define ISL_BY 0u
#define ISL_GY 1u
__device__ __forceinline__
void island_body(const PlanView& pv, uint32_t* recs, float* hbm, const Globals* g, const uint32_t* lcg,
                 uint32_t levelBegin, uint32_t islandIndex_, uint32_t batch, uint32_t arenaFloats) {
#else
#define ISL_BX blockIdx.x
#define ISL_BY blockIdx.y
#define ISL_GY gridDim.y
__global__ __launch_bounds__(ELEMHIP_ISLAND_THREADS)
void ELEMHIP_ISLAND_KERNEL(PlanView pv, uint32_t* recs, float* hbm, const Globals* g, const uint32_t* lcg,
                           uint32_t levelBegin, uint32_t batch, uint32_t arenaFloats) {
#endif
    const uint64_t tStart = clock64();
    if (__builtin_amdgcn_groupstaticsize() != 0u) __builtin_trap();   // wlds_* address the dynamic LDS segment from byte 0
    const uint32_t entry = UNI(pv.levelIslands[levelBegin + ISL_BX]);
    const Island isl = uni_pod(pv.islands[entry & 0xFFFFFFu]);
    const uint32_t splitIdx = entry >> 24;
    const uint32_t numOut = UNI(g->numOut);
    if (!root_running((gcup)recs, isl.rootRec, numOut)) return;
    constexpr uint32_t kRunWaves = ELEMHIP_ISLAND_THREADS / 64u;      // physical waves; each covers program waves w, w + kRunWaves, ...
    constexpr uint32_t kHalves = kWaves / kRunWaves;
    const bool pipe = kHalves == 1u && batch > 1u && !isl.stateless;
    if (pipe && ISL_BY != 0u) return;                       // a stateful island renders all its blocks in one workgroup
    if (!pipe && ISL_BY >= batch) return;

    // stage the island program in LDS (one coalesced copy), then fill the broadcast cells
    uint32_t* progLds = reinterpret_cast<uint32_t*>(lds + isl.ldsProg);
    gcup prog = (gcup)(pv.prog + isl.progBegin);
    for (uint32_t k = threadIdx.x; k < isl.progDwords; k += ELEMHIP_ISLAND_THREADS) progLds[k] = prog[k];
    if (threadIdx.x < kSlot0) lds[threadIdx.x] = 0.0f;
    for (uint32_t k = threadIdx.x; k < isl.numStages * isl.copies; k += ELEMHIP_ISLAND_THREADS) reinterpret_cast<uint32_t*>(lds + isl.ldsCounters)[k] = 0u;
    for (uint32_t k = threadIdx.x; k < isl.numStages * kWaves; k += ELEMHIP_ISLAND_THREADS) reinterpret_cast<uint32_t*>(lds + isl.ldsNext)[k] = 0u;
    // node records of this island: global -> LDS (written back when every wave is done)
    {
        gcup recTab = (gcup)(pv.prog + isl.progBegin + isl.recOff);
        uint32_t* recLds = reinterpret_cast<uint32_t*>(lds + isl.ldsRecs);
        for (uint32_t k = threadIdx.x; k < isl.numRecs * kRecDwords; k += ELEMHIP_ISLAND_THREADS)
            recLds[k] = ((gcup)recs)[recTab[k / kRecDwords] * kRecDwords + (k % kRecDwords)];
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < isl.numCells; k += ELEMHIP_ISLAND_THREADS) {
        const uint32_t word = progLds[isl.cellOff + 2 * k], rec_ = progLds[isl.cellOff + 2 * k + 1];
        lds[word] = u2f(((gcup)recs)[rec_ * kRecDwords + rec::P0]);
    }
    __syncthreads();

    Ctx c;
    c.recs = (rup)reinterpret_cast<uint32_t*>(lds + isl.ldsRecs); c.hbm = (gfp)hbm; c.g = g; c.lcg = (gcup)lcg;
    c.hbmS = (gfp)hbm; c.hbm0 = (gfp)hbm; c.offE = 0u; c.offS = 0u; c.bset = 0u; c.lo = 0u; c.hi = 0xFFFFu;   // (the interpreter's programs have no stream buffers)
    c.members = isl.ldsProg + isl.memOff; c.operands = isl.ldsProg + isl.opndOff;
    c.n = UNI(g->numSamples); c.stride = UNI(g->blockStride); c.numIn = UNI(g->numIn);
    c.lane = threadIdx.x & 63u;
    c.srF = uni_pod(g->sampleRateF); c.sr = uni_pod(g->sampleRate);
    const int64_t sampleTime0 = uni_pod(g->sampleTime);
    c.sampleTime = sampleTime0;
    c.defer = nullptr;
    const uint32_t wave = UNI(threadIdx.x >> 6);
    // frames this workgroup renders (whole block unless the island is split)
    const uint32_t lo = isl.split > 1 ? (splitIdx * c.stride) / isl.split : 0u;
    const uint32_t hi = isl.split > 1 ? ((splitIdx + 1) * c.stride) / isl.split : 0xFFFFu;

    unsigned long long* trace = (ISL_BX == 0 && ISL_BY == 0 && g->trace) ? reinterpret_cast<unsigned long long*>(g->trace) : nullptr;
    const uint64_t tProlog = clock64();
    const uint32_t S = isl.numStages, D = pipe ? isl.copies : 1u;
    const uint32_t tabT = isl.ldsProg + isl.stageOff, tabPrev = tabT + S, tabBegin0 = tabPrev + S;

    const uint32_t lastStage = S - 1u;                           // the planner never leaves the last stage empty
    const uint32_t myBlocks = (batch - ISL_BY + ISL_GY - 1u) / ISL_GY;
    const uint32_t steps = myBlocks * S * kHalves;
    uint32_t traceSlot = 0;
    uint64_t prevT1 = clock64();
    // pipelined walk: this wave's own (stage, phase) slots, macro-step by macro-step
    const uint32_t walkOffs = isl.ldsProg + isl.schedOff;
    const uint32_t e0 = UNI(ldsu(walkOffs + wave)), e1 = UNI(ldsu(walkOffs + wave + 1u));
    const uint32_t walkBase = walkOffs + kWaves + 1u;            // the planner pads in front of the offsets: entries are 16-byte aligned
    const uint32_t lastT = UNI(ldsu(tabT + lastStage));
    // Dataflow walk: every (stage) slot of this wave carries its own next-block counter (wave-private LDS words). The
    // wave polls its slots — later stages first, so older blocks drain and free their buffer sets — and runs the first
    // one whose block is ready: the previous non-empty stage of that block is complete and the buffer set is free. A slot
    // renders its blocks in order (node state), different slots advance independently: nothing but real dependencies
    // holds a wave back. (A first version stepped all slots of a wave in lock-step "macro-steps"; that coupled, e.g., the
    // final stage of block b to the coefficient stage of block b+2 on the same wave and cost ~20 % throughput.)
    const uint32_t myEntries = pipe ? e1 - e0 : 0u;
    const uint32_t nbBase = isl.ldsNext + wave * S;
    uint32_t pe = e0, remaining = myEntries;
    bool progress = false;
    uint32_t bbi = 0, bs_ = 0, bh = 0;          // barrier walk: block of this workgroup, stage, program-wave group
    Persist ps;
    ps.on = 0u; ps.done = 0u; ps.batch = batch; ps.D = D; ps.ctr = isl.ldsCounters; ps.lastStage = lastStage; ps.lastT = lastT;
    ps.slotArea = isl.slotArea; ps.b = 0u; ps.s = 0u; ps.prev = kNone; ps.prevT = 0u;
    c.ps = &ps;
    for (uint32_t it = 0; pipe ? remaining > 0u : it < steps; ++it) {
        uint32_t b, s, tb, te, use = 0u, copy = 0u, idx = 0u;
        const uint64_t tPoll = trace ? clock64() : 0;
        if (pipe) {
            idx = pe - e0;
            v4u ea, eb; uint32_t nbv;
            wlds_ld8_1(walkBase + pe * 8u, nbBase + idx, ea, eb, nbv);
            bool wrapped = false;
            if (++pe == e1) { pe = e0; wrapped = true; }
            s = UNI(ea.x); tb = UNI(ea.z); te = UNI(ea.w);
            const uint32_t prev = UNI(eb.x), prevT = UNI(eb.y);
            ps.prev = prev; ps.prevT = prevT;
            b = UNI(nbv);
            bool run = false;
            if (b < batch) {
                use = D == 4u ? b >> 2 : D == 5u ? b / 5u : D == 3u ? b / 3u : D == 2u ? b >> 1 : D == 6u ? b / 6u : b;
                copy = b - use * D;
                // completion counters are per (stage, buffer set): block b is use number b / D of set b % D
                const uint32_t wLast = isl.ldsCounters + lastStage * D + copy;
                const uint32_t wPrev = prev == kNone ? wLast : isl.ldsCounters + prev * D + copy;
                uint32_t cPrev, cLast;
                wlds_ld2(wPrev, wLast, cPrev, cLast);
                run = (prev == kNone || UNI(cPrev) >= (use + 1u) * prevT) && (use == 0u || UNI(cLast) >= use * lastT);
            }
            if (run) { progress = true; pe = e0; }               // after running a slot, look at the highest-priority one again
            else { if (wrapped) { if (!progress) __builtin_amdgcn_s_sleep(2); progress = false; } continue; }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        } else {
            b = ISL_BY + bbi * ISL_GY;
            s = bs_;
            const uint32_t tabBegin = tabBegin0 + (wave + bh * kRunWaves) * (S + 1u);
            const bool newStage = bh == 0u;
            if (++bh == kHalves) { bh = 0u; if (++bs_ == S) { bs_ = 0u; ++bbi; } }
            if (newStage && it > 0u) __syncthreads();
            tb = UNI(ldsu(tabBegin + s)); te = UNI(ldsu(tabBegin + s + 1u));
            if (tb == te) continue;
        }
        const uint32_t progBase = isl.ldsProg + copy * isl.copyDwords;
        c.members = progBase + isl.memOff; c.operands = progBase + isl.opndOff;
        c.hbm = (gfp)hbm + (size_t)b * arenaFloats; c.bset = b;
        c.sampleTime = sampleTime0 + (int64_t)b * (int64_t)c.n;
        for (uint32_t ti = tb; ti < te; ++ti) {
            v4u h, h2;
            wlds_ld8(progBase + ti * 8u, h, h2);
            const uint32_t d0 = UNI(h.x), d1 = UNI(h.y), d6 = UNI(h2.z);
            TaskU t;
            t.opcode = d0 & 0xFFFFu;
            t.stage = (d0 >> 16) & 0xFFu; t.flags = d0 >> 24;
            t.s0 = d1 & 0xFFFFu; t.s1 = d1 >> 16;
            t.first = UNI(h.z); t.count = UNI(h.w);
            t.o0 = UNI(h2.x); t.o1 = UNI(h2.y); t.outLds = d6 & 0xFFFFu; t.nin = d6 >> 16; t.outHbm = UNI(h2.w);
            // ELEMHIP trace hook: [wave][slot] = {opcode | stage << 16, start, end} in shader clocks
            const uint64_t t0 = trace ? clock64() : 0;
            // the lane id is re-made here, inside the innermost loop of the walk: whatever a task body derives from it (lane
            // masks of the scans, per-lane addresses) is then computed by that body only, not hoisted in front of every task
            c.lane = opaque_lane();
            ps.on = (pipe && (t.flags & kTaskOwnsWave)) ? 1u : 0u;
            ps.b = b; ps.s = s;
            if ((t.flags & 0x80u) && t.s1 <= c.n && isl.split <= 1u) {
                const uint32_t V = (t.s1 - t.s0) >> 6, i = t.s0 + c.lane * V;
                if (V == 2u) run_fast<2>(c, t, i);
                else if (V == 8u) run_fast<8>(c, t, i);
                else if (V == 4u) run_fast<4>(c, t, i);
                else run_fast<1>(c, t, i);
            } else
            run_task(c, t, lo, hi);
            if (trace) {
                const uint64_t t1 = clock64();
                if (c.lane == 0 && traceSlot < 62) {
                    unsigned long long* w = trace + (size_t)wave * 192 + 3 * (traceSlot + 2);
                    // bits 48-55: (start of the successful poll - end of the previous task) / 64, bits 56-63: (task start - poll start) / 64
                    const unsigned long long ga = min((tPoll - prevT1) >> 6, 255ull), gb = min((t0 - tPoll) >> 6, 255ull);
                    w[0] = (d0 & 0xFFFFFFFFull) | ((unsigned long long)(b & 0xFFFFu) << 32) | (ga << 48) | (gb << 56); w[1] = t0; w[2] = t1;
                }
                ++traceSlot;
                prevT1 = t1;
            }
        }
        // (ps.done is written by the member lanes only: make it a wave-wide fact before branching on it)
        if (pipe && __builtin_amdgcn_ballot_w64(ps.done != 0u) != 0ull) remaining = 0u;   // the task rendered and published every block itself (kTaskOwnsWave: its wave has no other slot)
        else if (pipe) {
            // Publish the slot: what other waves read from this one goes through LDS only (block buffers; exports to the HBM
            // arena are for later launches, node records and rings are re-read by this same wave). LDS operations of a wave
            // complete in issue order, so the counter update below is ordered behind the data without draining the global
            // stores of the node state — a full release fence here cost ~1.5 k cycles per slot in vmcnt(0) waits.
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_s_waitcnt(0xC07F);                  // lgkmcnt(0): this wave's LDS writes have landed
            if (opaque_lane() == 0) wlds_publish(isl.ldsCounters + s * D + copy, te - tb, nbBase + idx, b + 1u);
            WAVE_SYNC();
            if (b + 1u == batch) --remaining;
        }
    }
    if (trace && c.lane == 0) {
        unsigned long long* w = trace + (size_t)wave * 192;
        w[0] = traceSlot; w[1] = tStart; w[2] = tProlog; w[3] = clock64();
    }
    // node records: LDS -> global
    __syncthreads();
    {
        gcup recTab = (gcup)(pv.prog + isl.progBegin + isl.recOff);
        const uint32_t* recLds = reinterpret_cast<const uint32_t*>(lds + isl.ldsRecs);
        for (uint32_t k = threadIdx.x; k < isl.numRecs * kRecDwords; k += ELEMHIP_ISLAND_THREADS)
            ((gup)recs)[recTab[k / kRecDwords] * kRecDwords + (k % kRecDwords)] = recLds[k];
    }
}

// RootRenderSequence::promoteTapBuffers (GraphRenderSequence.h:200-210, 297-308): every tapOut of an active root hands its
// private block to the shared buffer of its name, in render-sequence order.
__device__ __forceinline__ void promote_taps(const PlanView& pv, gup recs, uint32_t n) {
    for (uint32_t k = 0; k < pv.numTaps; ++k) {
        const TapEntry te = pv.taps[k];
        gcup rr = recs + te.rootRec * kRecDwords;
        if (!(u2f(rr[rec::ROOT_TARGET]) > 0.5f)) continue;      // promotion needs root.active()
        gcup tr = recs + te.rec * kRecDwords;
        gfp shared = rec_ptr(tr, rec::TAP_SHARED);
        gcfp priv = rec_ptr(tr, rec::TAP_PRIVATE);
        if (!shared || !priv) continue;
        __syncthreads();   // earlier promotions into the same name complete first (last writer wins)
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) shared[i] = priv[i];
    }
}

// Epilogue: one workgroup. (1) zero + sum running roots into the output bus in render-sequence
// order (GraphRenderSequence.h:286-295, 227-231); (2) promote tap buffers of active roots
// (:306-308, Feedback.h:90-109); (3) advance root fades (GainFade.h:70-71); (4) advance the block.
#ifdef ELEMHIP_AUX
// output bus of one block: zero + sum the running roots per channel in render-sequence order
__device__ __forceinline__ void bus_sum(const PlanView& pv, gcup recs, gcfp hbm, gfp out, uint32_t n, uint32_t numOut, uint32_t stride) {
    __shared__ int rootChan[1024];        // channel of root r if it ran this block, else -1
    __shared__ uint16_t chanList[1024];   // running roots grouped by channel, render-sequence order inside a channel
    __shared__ uint16_t chanStart[kMaxOutBus + 1];
    const uint32_t nr = min(pv.numRoots, 1024u);
    for (uint32_t r = threadIdx.x; r < nr; r += blockDim.x) {
        const uint32_t rr = pv.roots[r].rec;
        rootChan[r] = root_running(recs, rr, numOut) ? (int)recs[rr * kRecDwords + rec::ROOT_CHANNEL] : -1;
    }
    __syncthreads();
    if (threadIdx.x < numOut) {           // thread ch counts its roots
        uint32_t cnt = 0;
        for (uint32_t r = 0; r < nr; ++r) cnt += rootChan[r] == (int)threadIdx.x;
        chanStart[threadIdx.x + 1] = (uint16_t)cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) { chanStart[0] = 0; for (uint32_t c = 0; c < numOut; ++c) chanStart[c + 1] += chanStart[c]; }
    __syncthreads();
    if (threadIdx.x < numOut) {
        uint32_t q = chanStart[threadIdx.x];
        for (uint32_t r = 0; r < nr; ++r) if (rootChan[r] == (int)threadIdx.x) chanList[q++] = (uint16_t)r;
    }
    __syncthreads();
    // 16-byte form (every block size that is a multiple of 4 frames): four frames per thread and step — the sum loop of a set's
    // epilogue is a chain of dependent round trips per thread (C4: 128 channels x 512 frames over 1024 threads = 64 of them at one
    // float each, 214 us per 1024-block set; C3's 8 channels: 13 us of a 70 us set)
    if (((n | stride) & 3u) == 0u && pv.numRoots <= 1024u && ((uintptr_t)out & 15u) == 0u && ((uintptr_t)hbm & 15u) == 0u) {
        typedef float bf4 __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(1))) const bf4* gcf4p;
        typedef __attribute__((address_space(1))) bf4* gf4p;
        const uint32_t n4 = n >> 2;
        for (uint32_t idx = threadIdx.x; idx < numOut * n4; idx += blockDim.x) {
            const uint32_t ch = idx / n4, i = (idx - ch * n4) << 2;
            bf4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
            for (uint32_t q = chanStart[ch]; q < chanStart[ch + 1]; ++q) acc += *(gcf4p)(hbm + (size_t)pv.roots[chanList[q]].hbm * stride + i);
            *(gf4p)(out + (size_t)ch * stride + i) = acc;
        }
        return;
    }
    for (uint32_t idx = threadIdx.x; idx < numOut * n; idx += blockDim.x) {
        const uint32_t ch = idx / n, i = idx - ch * n;
        float acc = 0.0f;
        for (uint32_t q = chanStart[ch]; q < chanStart[ch + 1]; ++q) acc += hbm[(size_t)pv.roots[chanList[q]].hbm * stride + i];
        for (uint32_t r = nr; r < pv.numRoots; ++r) {   // > 1024 roots: slow path
            const RootEntry re = pv.roots[r];
            if (root_running(recs, re.rec, numOut) && recs[re.rec * kRecDwords + rec::ROOT_CHANNEL] == ch)
                acc += hbm[(size_t)re.hbm * stride + i];
        }
        out[(size_t)ch * stride + i] = acc;
    }
}

// Epilogue of a multi-block launch: workgroup b sums block b's roots into output-ring slot b. The host only
// batches blocks while every running root's fade is settled and the plan has no taps / convolvers, so there
// is no per-block state to advance besides the sample clock.
// `doneFlag` (elemhip_process, a set of ONE block whose output bus is the host's mapped block): the workgroup ends by publishing
// `doneValue` to a word in mapped host memory, behind its output — the host spins on that word instead of synchronising the stream
// (publish_done).
__device__ __forceinline__ void publish_done(uint32_t* doneFlag, uint32_t doneValue) {
    __syncthreads();                                            // every thread's stores of the output block have completed ...
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");         // ... and are in host memory (0.5 us: profiles/r05/micro_fence_and_flag_costs.txt)
        __hip_atomic_store(doneFlag, doneValue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ __launch_bounds__(1024)
void elemhip_epilogue_batch_kernel(PlanView pv, uint32_t* recs_, const float* hbm_, Globals* g, float* outRing,
                                   uint32_t batch, uint32_t arenaFloats, uint32_t* doneFlag, uint32_t doneValue) {
    const uint32_t b = blockIdx.x;
    const uint32_t n = g->numSamples, numOut = min(g->numOut, (uint32_t)kMaxOutBus), stride = g->blockStride;
    bus_sum(pv, (gcup)recs_, (gcfp)hbm_ + (size_t)b * arenaFloats, (gfp)(outRing + (size_t)b * numOut * stride), n, numOut, stride);
    if (b == 0) promote_taps(pv, (gup)recs_, n);          // once per set: what the last block's promotion leaves behind
    if (b == 0 && threadIdx.x == 0) { g->sampleTime += (int64_t)n * (int64_t)batch; g->blockSlot = 0; }
    if (doneFlag && b == 0) publish_done(doneFlag, doneValue);
}

__global__ __launch_bounds__(1024)
void elemhip_epilogue_kernel(PlanView pv, uint32_t* recs_, const float* hbm_, Globals* g, float* outRing, uint32_t* doneFlag, uint32_t doneValue) {
    gup recs = (gup)recs_; gcfp hbm = (gcfp)hbm_;
    const uint32_t n = g->numSamples, numOut = min(g->numOut, (uint32_t)kMaxOutBus), stride = g->blockStride;
    gfp out = (gfp)(outRing + (size_t)g->blockSlot * numOut * stride);
    bus_sum(pv, recs, hbm, out, n, numOut, stride);
    promote_taps(pv, recs, n);
    __syncthreads();
    for (uint32_t r = threadIdx.x; r < pv.numRoots; r += blockDim.x) {
        gup rr = recs + pv.roots[r].rec * kRecDwords;
        if (!root_running(recs, pv.roots[r].rec, numOut)) continue;
        const float gcur = u2f(rr[rec::ROOT_GAIN]), tg = u2f(rr[rec::ROOT_TARGET]), step = u2f(rr[rec::ROOT_STEP]);
        if (gcur != tg && (rr[rec::ROOT_HASIN] || g->numIn > 0) /* fade.process ran (Core.h:74-77) */)
            rr[rec::ROOT_GAIN] = f2u(clampf(gcur + step * (float)(int)n, 0.0f, 1.0f));
    }
    // convolve nodes: commit the input-block position their main workgroups reached (conv.hip)
    for (uint32_t k = threadIdx.x; k < pv.numConvs; k += blockDim.x) {
        gup st = (gup)rec_ptr(recs + pv.convs[k].rec * kRecDwords, rec::CONV_STATE);
        if (!st) continue;
        st[conv::H_FILL] = st[conv::H_FILL_NEXT];
        st[conv::H_BLK] = st[conv::H_BLK_NEXT];
    }
    const uint32_t nextSlot = (g->blockSlot + 1) % g->ringSlots;
    if (g->inRing && nextSlot < g->inBlocks) {   // stage the next block's host inputs (elemhip_process_blocks)
        const uint32_t words = g->numIn * stride;
        gcfp src = (gcfp)reinterpret_cast<const float*>(g->inRing) + (size_t)nextSlot * words;
        gfp dst = (gfp)const_cast<float*>(hbm_);
        for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) dst[i] = src[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        g->sampleTime += (int64_t)n;
        g->blockSlot = nextSlot;
    }
    if (doneFlag) publish_done(doneFlag, doneValue);
}

// Multi-GPU hosts (elemhip_sum_buses, include/elemhip.h): the output buses of the ranks, gathered on one device, added in rank
// order — float addition is not associative and a ring all-reduce picks its own order; this one is reproducible bit for bit.
struct BusParts { const float* p[64]; uint32_t count; };
__global__ __launch_bounds__(256)
void elemhip_bus_sum_kernel(BusParts parts, float* dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float acc = parts.p[0][i];
    for (uint32_t r = 1; r < parts.count; ++r) acc += parts.p[r][i];
    dst[i] = acc;
}

// Host -> device parameter patches, applied at a block boundary (the reference's per-node
// atomics / SPSC queues drained at the top of process(), e.g. Delays.h:92-95).
__global__ void elemhip_patch_kernel(const Patch* patches, uint32_t count, uint32_t* recs, uint32_t* globals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const Patch p = patches[i];
    if (p.kind == 0) recs[p.index] = p.value;
    else if (p.kind == 1) { if (u2f(recs[p.index]) == 0.0f) recs[p.index] = p.value; }   // OnceNode arm, Core.h:359-362
    else globals[p.index] = p.value;
}

// ---- host launchers ------------------------------------------------------------------------------------
namespace elemhip {

hipError_t configure_kernels(uint32_t maxLdsBytes) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(elemhip_island_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)maxLdsBytes);
    if (e != hipSuccess) return e;
    return configure_kernels_rt(maxLdsBytes);
}

void launch_level(hipStream_t s, const PlanView& pv, uint32_t* recs, float* hbm, const Globals* g, const uint32_t* lcg,
                  uint32_t levelBegin, uint32_t numIslands, uint32_t ldsBytes, uint32_t batch, uint32_t arenaFloats, uint32_t statelessRows) {
    if (batch <= 1u) return launch_level_rt(s, pv, recs, hbm, g, lcg, levelBegin, numIslands, ldsBytes);
    // gridDim.y: blocks of a batch that stateless islands render concurrently
    const uint32_t gy = batch < statelessRows ? batch : (statelessRows ? statelessRows : 1u);
    hipLaunchKernelGGL(elemhip_island_kernel, dim3(numIslands, gy), dim3(kThreads), ldsBytes, s, pv, recs, hbm, g, lcg, levelBegin, batch, arenaFloats);
}

void launch_epilogue(hipStream_t s, const PlanView& pv, uint32_t* recs, const float* hbm, Globals* g, float* outRing, uint32_t* doneFlag, uint32_t doneValue) {
    hipLaunchKernelGGL(elemhip_epilogue_kernel, dim3(1), dim3(1024), 0, s, pv, recs, hbm, g, outRing, doneFlag, doneValue);
}

void launch_epilogue_batch(hipStream_t s, const PlanView& pv, uint32_t* recs, const float* hbm, Globals* g, float* outRing,
                           uint32_t batch, uint32_t arenaFloats, uint32_t* doneFlag, uint32_t doneValue) {
    hipLaunchKernelGGL(elemhip_epilogue_batch_kernel, dim3(batch), dim3(1024), 0, s, pv, recs, hbm, g, outRing, batch, arenaFloats,
                       batch == 1u ? doneFlag : nullptr, doneValue);
}

hipError_t launch_bus_sum(hipStream_t s, float* dst, const float* const* partials, uint32_t count, size_t n) {
    if (count == 0u || count > 64u || !dst || !partials) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    BusParts parts{};
    parts.count = count;
    for (uint32_t r = 0; r < count; ++r) { if (!partials[r]) return hipErrorInvalidValue; parts.p[r] = partials[r]; }
    hipLaunchKernelGGL(elemhip_bus_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, parts, dst, n);
    return hipGetLastError();
}

void launch_patches(hipStream_t s, const Patch* patches, uint32_t count, uint32_t* recs, uint32_t* globals) {
    if (!count) return;
    hipLaunchKernelGGL(elemhip_patch_kernel, dim3((count + 255) / 256), dim3(256), 0, s, patches, count, recs, globals);
}

} // namespace elemhip
#elif !defined(ELEMHIP_RESIDENT)   // the single-block (realtime) build of the island kernel: 4 waves, no register spills
namespace elemhip {

hipError_t configure_kernels_rt(uint32_t maxLdsBytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(ELEMHIP_ISLAND_KERNEL),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)maxLdsBytes);
}

void launch_level_rt(hipStream_t s, const PlanView& pv, uint32_t* recs, float* hbm, const Globals* g, const uint32_t* lcg,
                     uint32_t levelBegin, uint32_t numIslands, uint32_t ldsBytes) {
    hipLaunchKernelGGL(ELEMHIP_ISLAND_KERNEL, dim3(numIslands, 1), dim3(ELEMHIP_ISLAND_THREADS), ldsBytes, s, pv, recs, hbm, g, lcg, levelBegin, 1u, 0u);
}

} // namespace elemhip
#endif
