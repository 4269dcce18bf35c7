// island_spec.inc — skeleton of a per-island-SHAPE specialised kernel (compiled at run time, jit.cpp).
//
// The interpreter kernel (island.inc) decodes an island's program from LDS tables at run time: on the lone wavefront
// every task of a pipelined island runs on, that decode costs 1-2 k shader cycles per light op, more than the op. A
// specialised kernel is generated for one island shape (codegen.cpp): the task list of every (wave, stage) slot, every
// LDS address, operand kind, arity, frame range and lane count are compile-time constants, so what is left after
// inlining is the straight-line body of each op. The op bodies are the SAME functions the interpreter runs
// (island_ops.inc) — one implementation, one set of float semantics.
//
// What the generator provides before this file is included (namespace gen):
//   struct P { S, D, slotArea, ldsProg, memOff, opndOff, cellOff, numCells, recOff, numRecs, progDwords, ldsCounters,
//              ldsRecs, lastStage, lastT, block; static constexpr int waveSlots[8]; }
//   template <int W, int J> struct Slot { stage, prev, prevT, ntasks; static void run(Ctx&, uint32_t off); }
// and, per task, a descriptor T { opcode, flags, s0, s1, count; member<K>(c, off); member_lane(c, off, lane) }.
//
// Block pipeline protocol: identical to the interpreter's dataflow walk (same LDS completion counters per (stage, buffer
// set), same readiness rule, same publish), so it carries the same no-deadlock argument; only the decode is gone.

namespace gen { template <int W, int J> struct Slot; }   // specialised by the generated text for every (wave, slot)

namespace {

// (IntC / static_for: island_ops.inc)

// lane-wise choice between two members of a recurrence task (every field: the lanes of a task differ in all of them)
__device__ __forceinline__ Member spec_sel(bool pick, const Member& a, const Member& b) {
    Member m;
    m.rec = pick ? a.rec : b.rec; m.opnd = pick ? a.opnd : b.opnd; m.nin = pick ? a.nin : b.nin;
    m.outLds = pick ? a.outLds : b.outLds; m.outHbm = pick ? a.outHbm : b.outHbm; m.scratch = pick ? a.scratch : b.scratch;
    m.pad0_ = pick ? a.pad0_ : b.pad0_; m.pad1_ = pick ? a.pad1_ : b.pad1_;
#pragma unroll
    for (int j = 0; j < 6; ++j) m.sops[j] = pick ? a.sops[j] : b.sops[j];
    m.off = a.off; m.gdirect = pick ? a.gdirect : b.gdirect;
    return m;
}

__device__ __forceinline__ bool spec_root_running(gcup recs, uint32_t rootRec, uint32_t numOut) {   // Core.h:28-31, GraphRenderSequence.h:214-219
    gcup r = recs + rootRec * kRecDwords;
    const float tg = u2f(r[rec::ROOT_TARGET]), g = u2f(r[rec::ROOT_GAIN]);
    const bool on = tg > 0.5f;
    const bool settled = fabsf(tg - g) <= 1e-6f;
    const int ch = (int)r[rec::ROOT_CHANNEL];
    return (on || !settled) && ch >= 0 && (uint32_t)ch < numOut;
}

// ---- sample-parallel op, V consecutive frames per lane --------------------------------------------------------
template <uint16_t OPC, int V>
__device__ __forceinline__ void spec_par_op(const Ctx& c, const Member& m, uint32_t i, uint32_t nlim) {
    if constexpr (OPC >= OP_SIN && OPC <= OP_ABS) run_unary<OPC, V>(c, m, i, nlim);
    else if constexpr (OPC >= OP_LE && OPC <= OP_OR) run_binary<OPC, V>(c, m, i, nlim);
    else if constexpr (OPC >= OP_ADD && OPC <= OP_MAX) run_reduce<OPC, V>(c, m, i, nlim);
    else if constexpr (OPC == OP_IN) run_in<V>(c, m, i, nlim);
    else if constexpr (OPC == OP_COPY) run_copy<V>(c, m, i, nlim);
    else if constexpr (OPC == OP_ROOT) run_root<V>(c, m, i, nlim);
    else if constexpr (OPC == OP_PREWARP) run_prewarp<V>(c, m, i, nlim);
    else if constexpr (OPC == OP_TIME) run_time<V>(c, m, i, nlim);
    else if constexpr (OPC == OP_METRO) run_metro<V>(c, m, i, nlim);
    else if constexpr (OPC == OP_TAPIN) run_tapin<V>(c, m, i, nlim);
    else if constexpr (OPC == OP_TAPOUT) run_tapout<V>(c, m, i, nlim);
    else if constexpr (OPC == OP_TABLE) run_table<V>(c, m, i, nlim);
    else if constexpr (OPC == OP_SPARSEQ2) run_sparseq2<V>(c, m, i, nlim);
    else if constexpr (OPC == OP_CONST || OPC == OP_SR) run_fill<V>(c, m, i, nlim);
    else if constexpr (OPC == OP_SVF_COEF) run_svf_coef<false, V>(c, m, i, nlim);
    else if constexpr (OPC == OP_SHELF_COEF) run_svf_coef<true, V>(c, m, i, nlim);
    else if constexpr (OPC == OP_SAW_SHAPE) run_blep_shape<false, V>(c, m, i, nlim);
    else if constexpr (OPC == OP_SQUARE_SHAPE) run_blep_shape<true, V>(c, m, i, nlim);
    else static_assert(OPC == OP_INVALID, "opcode without a sample-parallel body");
}

// ---- stateful task (mirror of the interpreter's run_stateful) ---------------------------------------------------
template <class T>
__device__ __forceinline__ void spec_stateful(const Ctx& c, uint32_t off) {
    constexpr uint32_t op = T::opcode, cm = T::flags & 0x3Fu, count = T::count;
    const uint32_t n = c.n;
    if constexpr (op == OP_SVF || op == OP_SVFSHELF || op == OP_MM1P) {
        static_for<0, (int)count>([&](auto K) {
            const Member m = T::template member<K.value>(c, off);
            if constexpr (op == OP_SVF) scan_svf<false>(c, m);
            else if constexpr (op == OP_SVFSHELF) scan_svf<true>(c, m);
            else scan_mm1p(c, m);
        });
    } else {
        constexpr bool isBlep = (op == OP_BLEPSAW || op == OP_BLEPSQUARE || op == OP_BLEPTRIANGLE);
        if constexpr (isBlep && !(cm & 1u)) {   // pre-pass: inc[t] = f/sr into the out slot (skipped for a constant frequency)
            const float sr = c.srF;
            static_for<0, (int)count>([&](auto K) {
                const Member m = T::template member<K.value>(c, off);
                if (member_nin(c, m) < 1) return;
                const PIn p = pin_of(c, opnd_uniform(c, m, 0));
                if (n == 512) {
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
        if (n > 0) {
            // Lane-per-node recurrence. EVERY lane runs it (lanes >= count repeat the last member: same loads, same
            // arithmetic, same stores of the same values): a lone wave issues a VALU op in 4.07 cycles with all 64 lanes
            // enabled and in 5.09 with a partial EXEC mask (tools/micro/issue2.hip), and nothing else hides the difference.
            // A task of up to 16 plain float recurrences is laid out in quads (chain_skew.h): member m in lanes 4m .. 4m+3, so that
            // the four lanes of a member can run its chain 0, 4, 8 and 12 frames late and share the stores of a group. (The wide
            // biquad keeps one lane per member: its 6-operand loop sits at the register limit of its kernels.)
            constexpr bool quad = chain_skew::applies(count) &&
                (op == OP_PHASOR || op == OP_SPHASOR || op == OP_POLE || op == OP_ENV || op == OP_COUNTER || op == OP_ACCUM ||
                 op == OP_LATCH || op == OP_MAXHOLD || op == OP_PHASE);
            const uint32_t mlane = quad ? chain_skew::lane_member(c.lane, count) : c.lane;
            Member m = T::member_lane(c, off, mlane);
            if constexpr (quad) m.cnt |= kCntQuad;
            if constexpr (op == OP_PHASOR) ser_phasor<(int)cm>(c, m, cm);
            else if constexpr (op == OP_SPHASOR) ser_sphasor<(int)cm>(c, m, cm);
            else if constexpr (op == OP_POLE) ser_pole<(int)cm>(c, m, cm);
            else if constexpr (op == OP_ENV) ser_env<(int)cm>(c, m, cm);
            else if constexpr (op == OP_BIQUAD) ser_biquad<(int)cm>(c, m, cm);
            else if constexpr (op == OP_COUNTER) ser_counter<(int)cm>(c, m, cm);
            else if constexpr (op == OP_ACCUM) ser_accum<(int)cm>(c, m, cm);
            else if constexpr (op == OP_LATCH) ser_latch<(int)cm>(c, m, cm);
            else if constexpr (op == OP_MAXHOLD) ser_maxhold<(int)cm>(c, m, cm);
            else if constexpr (op == OP_ONCE) ser_once(c, m, cm);
            else if constexpr (op == OP_SEQ) ser_seq(c, m, cm);
            else if constexpr (op == OP_SEQ2) ser_seq2(c, m, cm);
            else if constexpr (op == OP_SPARSEQ) ser_sparseq(c, m, cm);
            else if constexpr (op == OP_SAMPLE) ser_sample(c, m, cm);
            else if constexpr (op == OP_MCSAMPLE) ser_mcsample(c, m, cm);
            else if constexpr (isBlep) { if (member_nin(c, m) < 1) szero(m, n); else ser_blep_phase(c, m, cm); }
            // (the kind goes with the MEMBER, not the lane: a lane past the task's members repeats the last member and must repeat
            //  its arithmetic too — in a task of phasors only it used to run the oscillator form, inc = f / sr instead of
            //  f * (1 / sr), and raced its own final phase into the phasor's record: wrong by 512 x an ulp of inc at every launch
            //  boundary, invisible inside a launch set where the phase stays in lane 0's register)
            else if constexpr (op == OP_PHASE) ser_phase(c, m, (mlane < count ? mlane : count - 1u) >= T::s0);
            else static_assert(op == OP_INVALID, "opcode without a recurrence body");
        }
        WAVE_SYNC();
        if constexpr (op == OP_MCSAMPLE) static_for<0, (int)count>([&](auto K) { gather_mcsample(c, T::template member<K.value>(c, off)); });
        if constexpr (op == OP_SAMPLE) {   // gather pass (VariablePitchLerpReader::tick, Sample.h:196-211): both readers, frame-parallel
            static_for<0, (int)count>([&](auto K) {
                const Member m = T::template member<K.value>(c, off);
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
                            if (l >= len) l %= len;
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
        if constexpr (op == OP_BLEPTRIANGLE) {   // post-pass: square wave from (phase, inc), then the leaky-free integrator (Oscillators.h:58-59)
            const float sr = c.srF;
            static_for<0, (int)count>([&](auto K) {
                const Member m = T::template member<K.value>(c, off);
                if (member_nin(c, m) < 1) return;
                const PIn p = pin_of(c, opnd_uniform(c, m, 0));
                constexpr bool constF = (cm & 1u) != 0u;
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
            if (n > 0) {
                const Member m = T::member_lane(c, off, c.lane);
                if (member_nin(c, m) >= 1) ser_blep_acc(c, m);
            }
        }
    }
    WAVE_SYNC();
    if constexpr (op == OP_BLEPSAW || op == OP_BLEPSQUARE) return;   // the out slot holds the phase; the shape task exports
    // chain outputs are produced in LDS; copy out the ones another island (or the epilogue) reads
    static_for<0, (int)count>([&](auto K) {
        if constexpr (T::template hasHbm<K.value>() && !T::gdirect && (op != OP_PHASE || (uint32_t)K.value < T::s0)) {
            const Member m = T::template member<K.value>(c, off);
            for (uint32_t i = c.lane; i < n; i += 64) hbm_buf(c, m.outHbm)[i] = lds[m.outLds + i];
        }
    });
}

// ---- one task ---------------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ void spec_task(const Ctx& c, uint32_t off) {
    constexpr uint32_t op = T::opcode, count = T::count;
    if constexpr (op == OP_RAND || op == OP_Z || op == OP_SDELAY || op == OP_DELAY || op == OP_SAMPLESEQ ||
                  op == OP_METER || op == OP_SNAPSHOT || op == OP_SCOPE || op == OP_CAPTURE || op == OP_FFT) {
        static_for<0, (int)count>([&](auto K) {
            const Member m = T::template member<K.value>(c, off);
            if constexpr (op == OP_RAND) run_rand(c, m, 0, c.n);
            else if constexpr (op == OP_Z) run_z(c, m, 0, c.n);
            else if constexpr (op == OP_SDELAY) run_sdelay(c, m, 0, c.n);
            else if constexpr (op == OP_DELAY) run_delay(c, m, 0, c.n);
            else if constexpr (op == OP_SAMPLESEQ) run_sampleseq(c, m, 0, c.n);
            else if constexpr (op == OP_METER) run_meter(c, m, 0, c.n);
            else if constexpr (op == OP_SNAPSHOT) run_snapshot(c, m, 0, c.n);
            else if constexpr (op == OP_CAPTURE) run_capture(c, m, 0, c.n);
            else if constexpr (op == OP_FFT) run_fft(c, m, 0, c.n);
            else run_scope(c, m, 0, c.n);
        });
    } else if constexpr (op == OP_PHASOR || op == OP_SPHASOR || op == OP_COUNTER || op == OP_ACCUM || op == OP_LATCH || op == OP_MAXHOLD ||
                         op == OP_ONCE || op == OP_SEQ || op == OP_SEQ2 || op == OP_SPARSEQ || op == OP_SAMPLE || op == OP_MCSAMPLE || op == OP_POLE || op == OP_ENV || op == OP_BIQUAD ||
                         op == OP_MM1P || op == OP_SVF || op == OP_SVFSHELF || op == OP_BLEPSAW || op == OP_BLEPSQUARE || op == OP_BLEPTRIANGLE || op == OP_PHASE) {
        spec_stateful<T>(c, off);
    } else {
        // sample-parallel: frames [s0, s1), 64 * V of them, lane l owns V consecutive frames
        constexpr uint32_t s0 = T::s0, s1 = T::s1;
        constexpr int V = (int)((s1 - s0) >> 6);
        static_assert(V == 1 || V == 2 || V == 4 || V == 8, "the planner emits 64, 128, 256 or 512-frame ranges");
        if (s0 >= c.n || s0 < c.lo || s0 >= c.hi) return;       // (lo / hi: a split island's workgroup renders its own part of the block)
        const uint32_t nlim = min(s1, c.n);
        const uint32_t i = s0 + c.lane * (uint32_t)V;
        static_for<0, (int)count>([&](auto K) {
            const Member m = T::template member<K.value>(c, off);
            spec_par_op<(uint16_t)op, V>(c, m, i, nlim);
        });
    }
}

// ---- a sample-parallel task at a run-time frame offset (wave-uniform stateless islands: one body for all waves) ----
template <class T>
__device__ __forceinline__ void spec_task_at(const Ctx& c, uint32_t delta) {
    constexpr uint32_t op = T::opcode, count = T::count;
    constexpr int V = (int)((T::s1 - T::s0) >> 6);
    static_assert(V == 1 || V == 2 || V == 4 || V == 8, "the planner emits 64, 128, 256 or 512-frame ranges");
    const uint32_t s0 = T::s0 + delta, s1 = T::s1 + delta;
    if (s0 >= c.n || s0 < c.lo || s0 >= c.hi) return;
    const uint32_t nlim = min(s1, c.n);
    const uint32_t i = s0 + c.lane * (uint32_t)V;
    static_for<0, (int)count>([&](auto K) {
        const Member m = T::template member<K.value>(c, 0u);
        spec_par_op<(uint16_t)op, V>(c, m, i, nlim);
    });
}

// ---- the block pipeline of one wave -----------------------------------------------------------------------------
template <class P, int W>
__device__ __forceinline__ void spec_wave(Ctx& c, float* hbm, uint32_t batch, uint32_t arenaFloats, uint32_t streamBase, uint32_t streamSlice,
                                          int64_t sampleTime0, unsigned long long* trace) {
    constexpr int K = P::waveSlots[W];
    if constexpr (K > 0) {
        constexpr uint32_t D = P::D;
        uint32_t nb[K], cp[K], us[K];              // per slot: next block, its buffer set (b % D) and use number (b / D)
        unsigned long long busy[K];
#pragma unroll
        for (int j = 0; j < K; ++j) { nb[j] = 0u; cp[j] = 0u; us[j] = 0u; busy[j] = 0ull; }
        uint32_t remaining = (uint32_t)K;
        Deferred dq; dq.addrBytes = 0u; dq.add = 0u; dq.pending = 0u;
        c.defer = &dq;
        while (remaining > 0u) {
            bool ran = false;
            // slots are listed later stages first: older blocks drain (and release their buffer sets) before younger ones start
            static_for<0, K>([&](auto J) {
                constexpr int j = J.value;
                using S = typename gen::template Slot<W, j>;
                if (ran || nb[j] >= batch) return;
                const uint32_t copy = cp[j], use = us[j];
                const uint32_t wLast = P::ldsCounters + P::lastStage * D + copy;
                const uint32_t wPrev = S::prev == kNone ? wLast : P::ldsCounters + S::prev * D + copy;
                uint32_t cPrev, cLast;
                wlds_ld2(wPrev, wLast, cPrev, cLast);
                bool ready = (S::prev == kNone || UNI(cPrev) >= (use + 1u) * S::prevT) && (use == 0u || UNI(cLast) >= use * P::lastT);
                if (!ready) return;
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                const uint32_t b = nb[j];
                // the block's arena slice (host inputs, exports) and its slice of the stream ring (set b % D, like the LDS buffers)
                c.hbm = (gfp)hbm + (size_t)b * arenaFloats; c.offE = b * arenaFloats * 4u; c.bset = b;
                c.hbmS = (gfp)hbm + (size_t)(streamBase + copy * streamSlice); c.offS = (streamBase + copy * streamSlice) * 4u;
                c.sampleTime = sampleTime0 + (int64_t)b * (int64_t)c.n;
                const unsigned long long t0 = trace ? clock64() : 0ull;
                S::run(c, copy * P::slotArea);
                if (trace) busy[j] += clock64() - t0;
                // publish: what other waves read from this one goes through LDS only; LDS operations of a wave complete in
                // issue order, so the counter update is ordered behind the block's samples
                if (dq.pending) { __builtin_amdgcn_s_waitcnt(0x0070); deferred_publish_now(dq); }   // (nothing in S::run took it)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                if constexpr (S::deferPublish) {
                    // a slot of streamed recurrences: its last arena stores are still on their way to L2; the counter update
                    // travels with the wave's next piece of work (island_ops.inc, Deferred)
                    dq.addrBytes = (P::ldsCounters + S::stage * D + copy) << 2; dq.add = (uint32_t)S::ntasks; dq.pending = 1u;
                } else {
                    // a slot that wrote arena buffers other waves of this launch read: the stores must have reached L2 first
                    if constexpr (S::writesStreams) __builtin_amdgcn_s_waitcnt(0x0070);   // vmcnt(0) lgkmcnt(0)
                    else __builtin_amdgcn_s_waitcnt(0xC07F);                              // lgkmcnt(0)
                    if (c.lane == 0) {
                        uint32_t t0_, t1_;
                        asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3\n\tds_add_u32 %0, %1" : "=&v"(t0_), "=&v"(t1_)
                                     : "s"((P::ldsCounters + S::stage * D + copy) << 2), "s"((uint32_t)S::ntasks) : "memory");
                    }
                    WAVE_SYNC();
                    // waiting waves sleep between polls (a poll is two LDS reads, and seven back-to-back pollers keep the LDS
                    // instruction queue busy enough to slow the recurrence waves' own loads and stores by a third); they are NOT
                    // pinged awake: s_wakeup breaks other waves' hazard wait states (island_ops.inc)
                }
                nb[j] = b + 1u;
                if (++cp[j] == D) { cp[j] = 0u; ++us[j]; }
                if (b + 1u == batch) --remaining;
                ran = true;
            });
            if (!ran) {
                if (dq.pending) { __builtin_amdgcn_s_waitcnt(0x0070); deferred_publish_now(dq); }   // nothing to hand it to: publish now
                else __builtin_amdgcn_s_sleep(1);   // ~64 * N cycles between two polls
            }
        }
        if (dq.pending) { __builtin_amdgcn_s_waitcnt(0x0070); deferred_publish_now(dq); }
        if (trace && c.lane == 0) {
            typedef __attribute__((address_space(1))) unsigned long long* gtp;   // (global, not FLAT: a pending FLAT access makes the
            gtp w = (gtp)(trace + (size_t)W * 192);                             //  compiler's wait counts for vector memory conservative)
            w[0] = (unsigned long long)K;
#pragma unroll
            for (int j = 0; j < K; ++j) { w[4 + 2 * j] = busy[j]; w[5 + 2 * j] = nb[j]; }
        }
    }
}

// ---- a stateless island (mixers, root gains: sample-parallel tasks only): no block pipeline ----------------------
// Nothing carries over from block to block, so the blocks of a launch set are spread over gridDim.y and each workgroup walks its
// blocks stage by stage with a workgroup barrier in between (the interpreter's scheme for such islands, minus its decode: a
// 128-input mixer is one straight-line left fold per wave). A split island is one workgroup per part (Ctx::lo / hi).
template <class P, int W, int STAGE>
__device__ __forceinline__ void spec_stateless_stage(Ctx& c) {
    constexpr int K = P::waveSlots[W];
    static_for<0, K>([&](auto J) {
        using S = typename gen::template Slot<W, J.value>;
        if constexpr ((int)S::stage == STAGE) S::run(c, 0u);
    });
}
template <class P>
__device__ __forceinline__ void spec_stateless_blocks(Ctx& c, float* hbm, uint32_t batch, uint32_t arenaFloats, int64_t sampleTime0) {
    const uint32_t wave = UNI(threadIdx.x >> 6);
    for (uint32_t b = blockIdx.y; b < batch; b += gridDim.y) {
        c.hbm = (gfp)hbm + (size_t)b * arenaFloats; c.offE = b * arenaFloats * 4u; c.bset = b;
        c.sampleTime = sampleTime0 + (int64_t)b * (int64_t)c.n;
        static_for<0, (int)P::S>([&](auto Sc) {
            constexpr int s = Sc.value;
            if constexpr (P::uniform) P::template ustage<s>(c, wave);
            else
            switch (wave) {
                case 0: spec_stateless_stage<P, 0, s>(c); break;
                case 1: spec_stateless_stage<P, 1, s>(c); break;
                case 2: spec_stateless_stage<P, 2, s>(c); break;
                case 3: spec_stateless_stage<P, 3, s>(c); break;
                case 4: spec_stateless_stage<P, 4, s>(c); break;
                case 5: spec_stateless_stage<P, 5, s>(c); break;
                case 6: spec_stateless_stage<P, 6, s>(c); break;
                default: spec_stateless_stage<P, 7, s>(c); break;
            }
            __syncthreads();     // the next stage (or the next block's first) reads / rewrites what this one produced
        });
    }
}

template <class P>
__device__ __forceinline__ void spec_island_main(const PlanView& pv, uint32_t* recs, float* hbm, const Globals* g, const uint32_t* lcg,
                                                 const uint32_t* islandList, uint32_t batch, uint32_t arenaFloats,
                                                 uint32_t streamBase, uint32_t streamSlice) {
    const unsigned long long tStart = clock64();
    const uint32_t entry = UNI(islandList[blockIdx.x]), islIdx = entry & 0xFFFFFFu, splitIdx = entry >> 24;   // (levelIslands entry format)
    const uint32_t progBegin = UNI(pv.islands[islIdx].progBegin), rootRec = UNI(pv.islands[islIdx].rootRec);
    const uint32_t numOut = UNI(g->numOut);
    if (!spec_root_running((gcup)recs, rootRec, numOut)) return;
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)lds != 0u) __builtin_trap();   // wlds_* address LDS from byte 0

    // stage the island program in LDS (buffer set 0's tables are the only ones read), then fill the broadcast cells
    uint32_t* progLds = reinterpret_cast<uint32_t*>(lds + P::ldsProg);
    gcup prog = (gcup)(pv.prog + progBegin);
    for (uint32_t k = threadIdx.x; k < P::progDwords; k += 512u) progLds[k] = prog[k];
    if (threadIdx.x < kSlot0) lds[threadIdx.x] = 0.0f;
    for (uint32_t k = threadIdx.x; k < P::S * P::D; k += 512u) reinterpret_cast<uint32_t*>(lds + P::ldsCounters)[k] = 0u;
    {
        gcup recTab = (gcup)(pv.prog + progBegin + P::recOff);
        uint32_t* recLds = reinterpret_cast<uint32_t*>(lds + P::ldsRecs);
        for (uint32_t k = threadIdx.x; k < P::numRecs * kRecDwords; k += 512u)
            recLds[k] = ((gcup)recs)[recTab[k / kRecDwords] * kRecDwords + (k % kRecDwords)];
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < P::numCells; k += 512u) {
        const uint32_t word = progLds[P::cellOff + 2 * k], rec_ = progLds[P::cellOff + 2 * k + 1];
        lds[word] = u2f(((gcup)recs)[rec_ * kRecDwords + rec::P0]);
    }
    __syncthreads();

    Ctx c;
    c.recs = (rup)reinterpret_cast<uint32_t*>(lds + P::ldsRecs); c.hbm = (gfp)hbm; c.g = g; c.lcg = (gcup)lcg;
    c.hbm0 = (gfp)hbm; c.hbmS = (gfp)hbm + streamBase; c.offE = 0u; c.offS = streamBase * 4u; c.bset = 0u;
    c.members = P::ldsProg + P::memOff; c.operands = P::ldsProg + P::specOpndOff;   // the variant's own operand table
    c.n = P::block;                                   // a specialised kernel renders full blocks only
    c.stride = P::block; c.numIn = UNI(g->numIn);
    c.lane = threadIdx.x & 63u;
    c.srF = uni_pod(g->sampleRateF); c.sr = uni_pod(g->sampleRate);
    const int64_t sampleTime0 = uni_pod(g->sampleTime);
    c.sampleTime = sampleTime0;
    c.ps = nullptr; c.defer = nullptr;
    c.lo = 0u; c.hi = 0xFFFFu;
    if constexpr (P::stateless) {
        if constexpr (P::split > 1u) { c.lo = (splitIdx * P::block) / P::split; c.hi = ((splitIdx + 1u) * P::block) / P::split; }
        spec_stateless_blocks<P>(c, hbm, batch, arenaFloats, sampleTime0);
        return;                  // (no node state: nothing to write back)
    }
    unsigned long long* trace = (blockIdx.x == 0 && g->trace) ? reinterpret_cast<unsigned long long*>(g->trace) : nullptr;
    const unsigned long long tProlog = clock64();
    const uint32_t wave = UNI(threadIdx.x >> 6);
    switch (wave) {
        case 0: spec_wave<P, 0>(c, hbm, batch, arenaFloats, streamBase, streamSlice, sampleTime0, trace); break;
        case 1: spec_wave<P, 1>(c, hbm, batch, arenaFloats, streamBase, streamSlice, sampleTime0, trace); break;
        case 2: spec_wave<P, 2>(c, hbm, batch, arenaFloats, streamBase, streamSlice, sampleTime0, trace); break;
        case 3: spec_wave<P, 3>(c, hbm, batch, arenaFloats, streamBase, streamSlice, sampleTime0, trace); break;
        case 4: spec_wave<P, 4>(c, hbm, batch, arenaFloats, streamBase, streamSlice, sampleTime0, trace); break;
        case 5: spec_wave<P, 5>(c, hbm, batch, arenaFloats, streamBase, streamSlice, sampleTime0, trace); break;
        case 6: spec_wave<P, 6>(c, hbm, batch, arenaFloats, streamBase, streamSlice, sampleTime0, trace); break;
        default: spec_wave<P, 7>(c, hbm, batch, arenaFloats, streamBase, streamSlice, sampleTime0, trace); break;
    }
    if (trace && (threadIdx.x & 63u) == 0u) {
        typedef __attribute__((address_space(1))) unsigned long long* gtp;
        gtp w = (gtp)(trace + (size_t)wave * 192);
        w[1] = tStart; w[2] = tProlog; w[3] = clock64();
    }
    // node records: LDS -> global
    __syncthreads();
    {
        gcup recTab = (gcup)(pv.prog + progBegin + P::recOff);
        const uint32_t* recLds = reinterpret_cast<const uint32_t*>(lds + P::ldsRecs);
        for (uint32_t k = threadIdx.x; k < P::numRecs * kRecDwords; k += 512u)
            ((gup)recs)[recTab[k / kRecDwords] * kRecDwords + (k % kRecDwords)] = recLds[k];
    }
}

} // namespace
