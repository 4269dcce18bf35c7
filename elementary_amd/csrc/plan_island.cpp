// plan_island.cpp — the planner's work on ONE island (PlanBuilder::planIsland): a convolve / call-out descriptor, or an island
// program — from the program cache (unchanged island, structural twin) or scheduled: stages, LDS slots by liveness, wave tasks,
// block-pipeline tables, the specialised-kernel variant, the blob. plan.cpp holds the graph-level passes around it.
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <numeric>
#include <unordered_set>

#include "plan_build.h"

namespace elemhip {

namespace {

// inputs a leaf node of this type would read from the host channels (its reference arity)
uint32_t leafArity(uint16_t op) {
    switch (op) {
        case OP_PHASOR: case OP_COUNTER: case OP_ONCE: case OP_BLEPSAW: case OP_BLEPSQUARE: case OP_BLEPTRIANGLE:
        case OP_Z: case OP_SDELAY: case OP_PREWARP: case OP_ROOT: case OP_TAPOUT: case OP_SAMPLESEQ: case OP_MCSAMPLE: case OP_FFT: return 1;
        case OP_SPHASOR: case OP_ACCUM: case OP_LATCH: case OP_MAXHOLD: case OP_SEQ: case OP_SEQ2: case OP_SPARSEQ: case OP_CAPTURE: case OP_SAMPLE: case OP_POLE: case OP_MM1P: case OP_SNAPSHOT: return 2;
        case OP_ENV: case OP_SVF: case OP_DELAY: return 3;
        case OP_SCOPE: return 4;
        case OP_SVFSHELF: return 4;
        case OP_BIQUAD: return 6;
        case OP_LE: case OP_LEQ: case OP_GE: case OP_GEQ: case OP_POW: case OP_EQ: case OP_AND: case OP_OR: return 2;
        case OP_ADD: case OP_SUB: case OP_MUL: case OP_DIV: case OP_MOD: case OP_MIN: case OP_MAX: case OP_IN: return kMaxHostIn;
        case OP_CONST: case OP_SR: case OP_RAND: case OP_TIME: case OP_METRO: case OP_TAPIN: return 0;
        default: return 1;   // unary math
    }
}

// blepsaw / blepsquare take two stages: the phase recurrence (one lane, serial), then the waveform as a sample-parallel
// task (OP_SAW_SHAPE / OP_SQUARE_SHAPE) that any wave can run — the recurrence is the longest serial item of a synth voice
// and bounds a pipelined island's block rate, so nothing else rides on its wave.
bool blepSplit(uint16_t op) { return op == OP_BLEPSAW || op == OP_BLEPSQUARE; }

} // namespace

uint32_t leafArityOfOp(uint16_t op) {
    if (op == OP_SAW_SHAPE || op == OP_SQUARE_SHAPE || op == OP_PHASE) return 1;
    if (op == OP_SVF_COEF) return leafArity(OP_SVF);
    if (op == OP_SHELF_COEF) return leafArity(OP_SVFSHELF);
    return leafArity(op);
}

namespace {

// estimated shader cycles of one task on a lone wave (measured on the pipelined C2 voice island, tests/_trace.py pipe32)
constexpr uint32_t kSlotGap = 2500u;   // hand-over into a (stage, wave) slot: publish, poll, acquire
uint32_t taskCost(uint16_t op, uint32_t units, uint32_t count) {
    const uint32_t gap = 900u;                                                              // header decode + dispatch around every task
    if (op == OP_SVF_COEF || op == OP_SHELF_COEF) return gap + 2300u * units * count;      // double tan + divides per frame
    if (op == OP_SVF || op == OP_SVFSHELF || op == OP_MM1P) return gap + 9500u * count;    // wave scan
    if (op == OP_SAW_SHAPE || op == OP_SQUARE_SHAPE) return gap + 500u * units * count;
    if (op == OP_BLEPSAW || op == OP_BLEPSQUARE || op == OP_PHASE) return gap + 12500u;     // phase recurrence only
    if (op == OP_BLEPTRIANGLE) return gap + 30000u;
    if (op == OP_POLE || op == OP_ENV || op == OP_BIQUAD) return gap + 15300u;
    if (kindOf(op) == K_CHAIN) return gap + 12000u;
    if (kindOf(op) == K_SINGLE) return gap + 4000u * count;
    if (op == OP_ROOT) return gap + 1000u + 250u * units * count;
    if (op >= OP_SIN && op <= OP_EXP) return gap + 900u + 280u * units * count;            // tanh: 3.1 k for a whole block
    return gap + 900u + 80u * units * count;                                                // light op: 1.5 k for a whole block
}

std::vector<uint32_t> membersOf(const std::vector<NI>& ni, const IslandBuild& B) {
    std::vector<uint32_t> m;
    m.reserve(4 * B.nodes.size());
    for (int k : B.nodes) { const NI& x = ni[k]; m.insert(m.end(), {(uint32_t)x.n->id, (uint32_t)x.n->op | (x.ch << 16), x.rec, x.hbm}); }
    return m;
}

} // namespace

// ---- 3/4. per-island schedule, LDS allocation, task emission -------------------------------------
bool PlanBuilder::planIsland(size_t ii) {
    IslandBuild& B = ib[ii];
    Island& I = p.islands[ii];
    I.rootRec = seqRoots[B.seq]->rec;
    p.islandRoot[ii] = seqRoots[B.seq]->id;
    if (ni[B.nodes[0]].kind == K_CONV) { emitConvDesc(ii); return true; }
    if (ni[B.nodes[0]].kind == K_HOST) { emitHostDesc(ii); return true; }
    const auto tIsl0 = std::chrono::steady_clock::now();
    IslandSchedule s(*this, ii);
    if (e.planCache != 0 && s.takeFromCache()) return true;
    if (!s.assignStages()) return false;
    s.allocateLds();
    s.emitTasks();
    if (s.copies > 1) s.balanceWaves();
    s.orderTasks();
    s.pipelineTables();
    s.specVariant();
    s.packBlob();
    s.recordProgram();
    if (planTiming()) std::fprintf(stderr, "[elemhip] plan   island %zu scheduled in %.3f ms (%zu nodes)\n", ii, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tIsl0).count(), B.nodes.size());
    return true;
}

// one node, no island program: a ConvDesc instead
void PlanBuilder::emitConvDesc(size_t ii) {
    IslandBuild& B = ib[ii];
    Island& I = p.islands[ii];
    NI& x = ni[B.nodes[0]];
    ConvDesc d{};
    d.rec = x.n->rec; d.outHbm = x.hbm; d.rootRec = I.rootRec; d.slices = std::max<uint32_t>(1, x.n->convSlices);
    d.fuseRootRec = kNone;
    if (x.fusedRoot >= 0) { d.outHbm = ni[x.fusedRoot].hbm; d.fuseRootRec = ni[x.fusedRoot].n->rec; }
    if (x.n->inlets.empty()) d.inKind = 3;                                      // leaf: host input 0
    else {
        const Inlet& in = x.n->inlets[0];
        const int si = srcOf(in);
        if (si < 0) d.inKind = 4;
        else if (ni[si].elided) { d.inKind = 5; d.inIdx = ni[si].n->rec; }   // host channel named by the `in` record
        else if (ni[si].kind == K_CONST) { d.inKind = 2; d.inIdx = ni[si].n->rec; }
        else { d.inKind = 1; d.inIdx = ni[si].hbm; }
    }
    I = Island{};
    I.rootRec = d.rootRec; I.split = 0;                                         // no island-kernel workgroup
    convLevel.push_back(B.level);
    p.convs.push_back(d);
    p.convNodeIds.push_back(x.n->id);
}

// call-out node (Runtime::registerNodeType): no device program, a HostDesc for the engine
void PlanBuilder::emitHostDesc(size_t ii) {
    IslandBuild& B = ib[ii];
    Island& I = p.islands[ii];
    NI& x = ni[B.nodes[0]];
    Plan::HostDesc d{};
    d.nodeId = x.n->id; d.rootId = seqRoots[B.seq]->id; d.outHbm = x.hbm; d.level = (uint32_t)B.level;
    {
        auto a = seqRoots[B.seq]->props.find("active");
        d.active = a != seqRoots[B.seq]->props.end() && a->second.isBool() && a->second.b;
    }
    d.leaf = x.n->inlets.empty();
    for (auto& in : x.n->inlets) {
        const int si = srcOf(in);
        if (si < 0) d.inputs.push_back({0, 0u, 0.0f});
        else if (ni[si].kind == K_CONST && !ni[si].elided) d.inputs.push_back({2, ni[si].n->rec, 0.0f});
        else if (ni[si].elided && ni[si].n->op == OP_IN) d.inputs.push_back({3, ni[si].n->rec, 0.0f});
        else d.inputs.push_back({1, ni[si].hbm, 0.0f});
    }
    I = Island{};
    I.rootRec = seqRoots[B.seq]->rec; I.split = 0;
    p.hosts.push_back(std::move(d));
}

IslandSchedule::IslandSchedule(PlanBuilder& b, size_t island)
    : pb(b), e(b.e), p(b.p), ni(b.ni), ii(island), B(b.ib[island]), I(b.p.islands[island]), bs(b.bs), packed(b.packCount[island]),
      pairsTaps(b.islandPairsTaps[island] != 0), streamStart(b.p.numStreamBuffers), memberIds(membersOf(b.ni, b.ib[island])) {}

// ---- island program cache (commit -> first block): a re-plan after "one voice replaced" meets the other
// islands unchanged. Everything below is a function of the island's nodes (ids, opcodes, records, edges), of where its
// exports / imports sit in the arena, of the stream buffers handed out so far and of the planner options: keyed by a hash
// of exactly that, an unchanged island takes its Island header, program blob and kernel text from the previous build.
// `plan_cache` = 2 schedules anyway and compares (tests).
//
// ONE walk over the island's members and inlets feeds both keys. The exact key mixes node ids, records and arena buffers as
// themselves (and the first stream buffer); the structural key leaves the ids out and replaces every record / arena buffer by the
// ordinal of its first appearance (canonRecs / canonHbms: the island's STRUCTURE), every in-island source by its position.
uint64_t IslandSchedule::islandKey(bool structural) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint64_t v) { h ^= v; h *= 1099511628211ull; h ^= h >> 29; };
    auto rec = [&](uint32_t r) -> uint32_t {
        if (!structural || r == kNone) return r;
        for (size_t q = 0; q < canonRecs.size(); ++q) if (canonRecs[q] == r) return (uint32_t)q;
        canonRecs.push_back(r); return (uint32_t)canonRecs.size() - 1u;
    };
    auto hbm = [&](uint32_t b) -> uint32_t {
        if (!structural || b == kNone) return b;
        if (b < kMaxHostIn) return 0x40000000u | b;             // host input slots are the same for everybody
        for (size_t q = 0; q < canonHbms.size(); ++q) if (canonHbms[q] == b) return (uint32_t)q;
        canonHbms.push_back(b); return (uint32_t)canonHbms.size() - 1u;
    };
    auto posIn = [&](int niIndex) -> uint32_t {          // position of an island member (B.nodes is sorted)
        auto f = std::lower_bound(B.nodes.begin(), B.nodes.end(), niIndex);
        return (f != B.nodes.end() && *f == niIndex) ? (uint32_t)(f - B.nodes.begin()) : 0xFFFFu;
    };
    if (structural) { canonRecs.clear(); canonHbms.clear(); }
    mix(bs); mix(pb.maxCopies); mix(pb.splitCoefStage); mix(pb.wantSpec); mix(e.fuseSvfCoef); mix(e.mergePhases);
    mix(e.mixerSplit); mix(packed); mix((uint32_t)pairsTaps);
    if (!structural) mix(streamStart);
    mix(B.nodes.size());       // (the owning root's record is not an input of the schedule: Island::rootRec is re-made per plan)
    for (int k : B.nodes) {
        const NI& x = ni[k];
        if (!structural) mix((uint32_t)x.n->id);
        mix(x.n->op); mix(rec(x.rec)); mix(x.ch); mix((uint32_t)x.kind); mix(x.exported); mix(hbm(x.hbm)); mix(x.elided);
        mix(x.fusedRoot >= 0 ? rec(ni[(size_t)x.fusedRoot].n->rec) : kNone); mix(x.needLds);
        const int tw = pb.tapWriter[(size_t)k];
        if (!structural) mix((uint32_t)(tw >= 0 ? ni[(size_t)tw].n->id : 0));
        else mix(tw >= 0 ? (posIn(tw) != 0xFFFFu ? posIn(tw) : 0x10000u | rec(ni[(size_t)tw].rec)) : 0xFFFFFFu);
        mix(x.n->inlets.size());
        for (auto& in : x.n->inlets) {
            if (!structural) mix((uint32_t)in.source);
            mix(in.channel);
            const int si = pb.srcOf(in);
            if (si < 0) { mix(0xDEADu); continue; }
            const NI& sn = ni[si];
            const bool inside = sn.island == x.island;
            mix((uint32_t)sn.kind); mix(inside);
            if (structural) mix(inside ? posIn(si) : 0xFFFFu);
            mix(hbm(sn.hbm)); mix(rec(sn.rec)); mix(sn.elided); mix(sn.n->op);
        }
    }
    return h;
}

// true: the island took its program from the cache (an exact hit, or a structural twin's program renamed) and is done
bool IslandSchedule::takeFromCache() {
    ikey = islandKey(false);
    // (only for islands the exact key does not find: an unchanged island of a live graph pays for one walk, not two)
    auto it = e.islandCache.find(ikey);
    const bool exactKnown = e.planCache == 1 && it != e.islandCache.end();
    if (e.relocatePrograms && !exactKnown) skey = islandKey(true);
    if (it != e.islandCache.end() && it->second->heap == e.progHeap) {
        // the key is 64 bits of hash: a hit is only taken when the members it was built from are the members in front of us
        if (it->second->members == memberIds) cached = it->second; else e.st.planCacheMismatches++;
    }
    if (cached && e.planCache == 1) { adoptCached(); return true; }
    // ---- same structure, other nodes (another voice of the patch; the voice that replaces one): the twin's program with the
    // i-th record / arena buffer it names replaced by this island's i-th, stream buffers moved to this island's first. Any
    // reference the canonical walk did not meet makes the attempt fail and the island is scheduled as usual.
    if (skey == 0 || cached) return false;
    auto ts = e.islandShapeCache.find(skey);
    if (ts == e.islandShapeCache.end() || ts->second->canonRecs.size() != canonRecs.size() || ts->second->canonHbms.size() != canonHbms.size() ||
        ts->second->members.size() != memberIds.size()) return false;
        // the structural key is 64 bits of hash too: before another island's program is renamed into this one, the two
        // must at least agree member by member on opcode and output channel
    for (size_t q = 1; q < memberIds.size(); q += 4)
        if (ts->second->members[q] != memberIds[q]) { e.st.planRelocationMismatches++; return false; }
    return relocateTwin(ts->second);
}

void IslandSchedule::adoptCached() {
    I = cached->I;
    I.progBegin = cached->heapBegin;          // the program is on the device already
    I.rootRec = pb.seqRoots[B.seq]->rec;
    adoptProgram(cached);
    e.st.planIslandsReused++;
}

// the twin's program with its records / arena / stream buffers renamed to this island's. true: adopted (plan_cache = 1);
// false: a reference the canonical walk did not meet, or plan_cache = 2 (the renamed blob waits in `relocated` for the fresh schedule)
bool IslandSchedule::relocateTwin(const std::shared_ptr<IslandProgram>& twin) {
    std::vector<uint32_t> blob(twin->blob);
    const Island& T = twin->I;
    bool ok = true;
    auto mapRec = [&](uint32_t r) -> uint32_t {
        for (size_t q = 0; q < twin->canonRecs.size(); ++q) if (twin->canonRecs[q] == r) return canonRecs[q];
        ok = false; return r;
    };
    auto mapHbm = [&](uint32_t b) -> uint32_t {          // an arena index as stored in outHbm fields / operand values (kNone handled by callers)
        if (b & kOpStream) return kOpStream | ((b & ~kOpStream) - twin->streamStart + streamStart);
        if (b < kMaxHostIn) return b;
        for (size_t q = 0; q < twin->canonHbms.size(); ++q) if (twin->canonHbms[q] == b) return canonHbms[q];
        ok = false; return b;
    };
    auto mapOpnd = [&](uint32_t o) -> uint32_t { return (o & kOpKindMask) == kOpHbm ? (kOpHbm | mapHbm(o & kOpValMask)) : o; };
    const uint32_t numMembers = twin->numMembers, numOperands = twin->numOperands;
    for (uint32_t d = 0; d < T.copies && ok; ++d) {
        uint32_t* c0 = blob.data() + (size_t)d * T.copyDwords;
        for (uint32_t t = 0; t < T.numTasks; ++t) {
            Task* tk = reinterpret_cast<Task*>(c0 + t * 8u);
            tk->o0 = mapOpnd(tk->o0); tk->o1 = mapOpnd(tk->o1);
            if (tk->outHbm != kNone) tk->outHbm = mapHbm(tk->outHbm);
        }
        for (uint32_t m = 0; m < numMembers; ++m) {
            Member* mb = reinterpret_cast<Member*>(c0 + T.memOff + m * 8u);
            if (mb->outHbm != kNone) mb->outHbm = mapHbm(mb->outHbm);
        }
        for (uint32_t o = 0; o < numOperands; ++o) c0[T.opndOff + o] = mapOpnd(c0[T.opndOff + o]);
    }
    for (uint32_t q = 0; q < T.numCells && ok; ++q) blob[T.cellOff + 2u * q + 1u] = mapRec(blob[T.cellOff + 2u * q + 1u]);
    for (uint32_t q = 0; q < T.numRecs && ok; ++q) blob[T.recOff + q] = mapRec(blob[T.recOff + q]);
    // behind the record table: the specialised variant's arena table, then its operand table (to the end of the program)
    const uint32_t tail0 = T.recOff + T.numRecs, tailN = T.progDwords - tail0;
    if (ok && tailN < twin->specHbmTab) ok = false;
    for (uint32_t q = 0; q < twin->specHbmTab && ok; ++q) blob[tail0 + q] = mapHbm(blob[tail0 + q]);
    for (uint32_t q = twin->specHbmTab; q < tailN && ok; ++q) blob[tail0 + q] = mapOpnd(blob[tail0 + q]);
    if (!ok) { e.st.planRelocationMismatches++; return false; }
    if (e.planCache != 1) { relocated.swap(blob); return false; }   // plan_cache = 2: schedule anyway, then compare with this
    I = T;
    I.progBegin = (uint32_t)p.prog.size();      // (local to this build's staging; moved into the heap by placePrograms)
    I.rootRec = pb.seqRoots[B.seq]->rec;
    p.prog.insert(p.prog.end(), blob.begin(), blob.end());
    auto ent = newEntry(std::move(blob));
    ent->spec = twin->spec;
    ent->numMembers = twin->numMembers; ent->numOperands = twin->numOperands; ent->streamDelta = twin->streamDelta;
    ent->specHbmTab = twin->specHbmTab;
    adoptProgram(ent);
    e.islandCache[ikey] = ent;
    e.st.planIslandsRelocated++;
    return true;
}

// a program this build made (scheduled, or renamed from a twin): p.prog holds its blob, I.progBegin is relative to it
std::shared_ptr<IslandProgram> IslandSchedule::newEntry(std::vector<uint32_t>&& blob) {
    auto ent = std::make_shared<IslandProgram>();
    ent->I = I; ent->blob = std::move(blob); ent->members = memberIds;
    if (skey != 0) { ent->canonRecs = canonRecs; ent->canonHbms = canonHbms; ent->streamStart = streamStart; ent->shapeKey = skey; }
    pb.scheduled.push_back((uint32_t)ii);
    return ent;
}

// what the plan keeps of an island's program, wherever it came from (I is final)
void IslandSchedule::adoptProgram(const std::shared_ptr<IslandProgram>& ent) {
    p.islandProg[ii] = ent;
    p.progDwordsTotal += ent->blob.size();
    p.numStreamBuffers = streamStart + ent->streamDelta;
    if (packed > 1u) pb.minPackedCopies = pb.minPackedCopies ? std::min(pb.minPackedCopies, I.copies) : I.copies;
    p.maxCopies = std::max(p.maxCopies, I.copies);
    p.maxLdsBytes = std::max(p.maxLdsBytes, I.ldsWords * 4u);
    if (ent->spec) { if (p.specText.size() < pb.ib.size()) p.specText.resize(pb.ib.size()); p.specText[ii] = ent->spec; }
    p.numTasks += I.numTasks; p.numMembers += ent->numMembers; p.numOperands += ent->numOperands;
}

int IslandSchedule::importFor(uint32_t hbm) {
    for (size_t q = 0; q < imports.size(); ++q) if (imports[q].hbm == hbm) return (int)q;
    imports.push_back(Import{hbm, 0, kNone});
    return (int)imports.size() - 1;
}

// stage of every member (and the last stage that reads it, imports included). false: the island is too deep
bool IslandSchedule::assignStages() {
    bool anyImport = false;
    for (int k : B.nodes) {
        NI& x = ni[k];
        if (x.kind != K_CHAIN) continue;
        if (x.n->inlets.empty()) { if (leafArity(x.n->op) > 0) anyImport = true; continue; }
        for (auto& in : x.n->inlets) {
            const int si = pb.srcOf(in);
            if (si < 0) continue;
            NI& s = ni[si];
            if (s.kind != K_CONST && s.island != x.island) anyImport = true;
        }
    }
    base = anyImport ? 1 : 0;
    fuseCoef = e.fuseSvfCoef == 1 || (e.fuseSvfCoef == 2 && packed > 1u);
    maxStage = 0;
    for (int k : B.nodes) {
        NI& x = ni[k];
        int lv = base, sub = 0;
        for (auto& in : x.n->inlets) {
            const int si = pb.srcOf(in);
            if (si < 0) continue;
            NI& s = ni[si];
            if (s.kind == K_CONST || s.island != x.island) continue;
            // Sample-parallel ops are lane-local (lane l reads and writes only samples l + 64j of
            // its slice), so a sample-parallel consumer of a sample-parallel producer can run in
            // the SAME stage on the same wave, right after it, with no barrier in between.
            const bool xsvf = (x.n->op == OP_SVF || x.n->op == OP_SVFSHELF) && !coefFused(x.n->op);   // its coefficient pre-pass is such an op too
            // (xsvf && pb.splitCoefStage: the pre-pass gets a stage of its own, so its light producers run unsplit on one
            // wave instead of four times with four times the per-task overhead)
            // (a split oscillator's waveform task is sample-parallel as well: its consumers may follow it in its stage)
            const bool fuse = (x.kind == K_PAR || (xsvf && !pb.splitCoefStage)) && (s.kind == K_PAR || blepSplit(s.n->op));
            const int need = fuse ? s.level : s.level + 1;
            if (need > lv) { lv = need; sub = 0; }
            if (fuse && s.level == lv) sub = std::max(sub, s.sub + 1);
        }
        x.sub = sub;
        if (x.n->op == OP_TAPOUT && pairsTaps) {   // behind every tapIn (a leaf: stage `base`) that reads its buffer
            bool paired = false;
            for (int k2 : B.nodes) paired = paired || (pb.tapWriter[(size_t)k2] >= 0 && ni[(size_t)pb.tapWriter[(size_t)k2]].n == x.n);
            if (paired && lv < base + 1) { lv = base + 1; x.sub = 0; }
        }
        // svf / shelf take two stages: sample-parallel coefficient pre-pass, then the scan
        if ((x.n->op == OP_SVF || x.n->op == OP_SVFSHELF) && !coefFused(x.n->op)) lv += 1;
        if (blepSplit(x.n->op)) lv += 1;   // recurrence at lv - 1, waveform (the node's output) at lv
        x.level = lv;
        x.lastUse = lv;
        maxStage = std::max(maxStage, lv);
    }
    if (maxStage > 250) { std::fprintf(stderr, "[elemhip] plan: island too deep\n"); return false; }
    for (int k : B.nodes) {
        NI& x = ni[k];
        for (auto& in : x.n->inlets) {
            const int si = pb.srcOf(in);
            if (si < 0) continue;
            NI& s = ni[si];
            if (s.kind == K_CONST) continue;
            if (s.island == x.island) s.lastUse = std::max(s.lastUse, x.level);
            else if (x.kind == K_CHAIN) { Import& im = imports[importFor(s.hbm)]; im.lastUse = std::max(im.lastUse, x.level); }
        }
        if (x.kind == K_CHAIN && x.n->inlets.empty()) {
            const uint32_t ar = std::min<uint32_t>(leafArity(x.n->op), kMaxHostIn);
            for (uint32_t c = 0; c < ar; ++c) { Import& im = imports[importFor(c)]; im.lastUse = std::max(im.lastUse, x.level); }
        }
    }
    return true;
}

uint32_t IslandSchedule::takeSlots(int stage, uint32_t count, int lastUse) {
    const int region = (count == 1 && lastUse - stage >= 2) ? 1 : 0;
    std::vector<int>& fr = slotFreeAt[region];
    const uint32_t tag = region ? kLongBit : 0u;
    // `count` consecutive slots free at `stage`
    const size_t S = fr.size();
    for (size_t s0 = 0; s0 + count <= S; ++s0) {
        bool ok = true;
        for (uint32_t c = 0; c < count; ++c) if (fr[s0 + c] > stage) { ok = false; break; }
        if (ok) { for (uint32_t c = 0; c < count; ++c) fr[s0 + c] = lastUse + 1; return tag | (uint32_t)s0; }
    }
    // extend (reuse a free tail if there is one)
    size_t s0 = S;
    while (s0 > 0 && fr[s0 - 1] <= stage && S - (s0 - 1) <= count) --s0;
    fr.resize(s0 + count, 0);
    for (uint32_t c = 0; c < count; ++c) fr[s0 + c] = lastUse + 1;
    return tag | (uint32_t)s0;
}

// LDS slots by liveness. Words 0..3 = zero cell; slots start at word kSlot0.
// Two regions keep the allocation dense: buffers that live for one stage (and the multi-slot scratch areas, which
// need consecutive slots) recycle the low region; buffers that stay live across several stages go to their own
// region, so they never leave holes in front of a scratch request. (C2 voice: 13 slots -> 10, i.e. one more block in
// flight in the same LDS.)
void IslandSchedule::allocateLds() {
    for (auto& im : imports) im.lds = takeSlots(0, 1, im.lastUse);
    // A paired tapOut's output slot belongs to it for the whole block, every block: with one block in flight the slot still
    // holds block b when the tapIns of block b + 1 run (stage `base`, before the tapOut's own stage), so the hand-over never
    // leaves LDS — the same completion counters that order every other buffer of the island order it (run_tapin).
    std::vector<int> pairedOut;
    if (pairsTaps)
        for (int k : B.nodes) if (pb.tapWriter[(size_t)k] >= 0 && std::find(pairedOut.begin(), pairedOut.end(), pb.tapWriter[(size_t)k]) == pairedOut.end()) pairedOut.push_back(pb.tapWriter[(size_t)k]);
    for (int k : pairedOut) ni[(size_t)k].lds = takeSlots(0, 1, maxStage);
    for (int stage = base; stage <= maxStage; ++stage) {
        for (int k : B.nodes) {   // coefficient scratch of the svf's that scan in the NEXT stage
            NI& x = ni[k];
            if (x.level != stage + 1 || (x.n->op != OP_SVF && x.n->op != OP_SVFSHELF) || coefFused(x.n->op)) continue;
            x.scratch = takeSlots(stage, scratchSlots(x.n->op), stage + 1);
        }
        for (int k : B.nodes) {   // out slot of a split oscillator: carries the phase from the recurrence stage on
            NI& x = ni[k];
            if (x.level == stage + 1 && blepSplit(x.n->op) && x.needLds) x.lds = takeSlots(stage, 1, x.lastUse);
        }
        for (int k : B.nodes) {
            NI& x = ni[k];
            if (x.level != stage) continue;
            if (x.needLds && !blepSplit(x.n->op) && std::find(pairedOut.begin(), pairedOut.end(), k) == pairedOut.end()) x.lds = takeSlots(stage, 1, x.lastUse);
            const uint32_t sc = scratchSlots(x.n->op);
            if (sc && x.n->op != OP_SVF && x.n->op != OP_SVFSHELF) x.scratch = takeSlots(stage, sc, stage);
        }
    }
    {   // slot index -> LDS word: short-lived region first, long-lived region behind it
        const uint32_t nShort = (uint32_t)slotFreeAt[0].size();
        auto resolve = [&](uint32_t v) { return v == kNone ? v : kSlot0 + ((v & kLongBit) ? nShort + (v & ~kLongBit) : v) * kSlotWords; };
        for (auto& im : imports) im.lds = resolve(im.lds);
        for (int k : B.nodes) { ni[k].lds = resolve(ni[k].lds); ni[k].scratch = resolve(ni[k].scratch); }
        // a paired tapIn names its writer's slot (Member::scratch; run_tapin reads it from the set's second block on)
        for (int k : B.nodes) if (pb.tapWriter[(size_t)k] >= 0) ni[k].scratch = ni[(size_t)pb.tapWriter[(size_t)k]].lds;
    }
    slotArea = (uint32_t)(slotFreeAt[0].size() + slotFreeAt[1].size()) * kSlotWords;      // block-buffer words of one copy
    statelessIsland = true;
    for (int k : B.nodes) if (ni[k].kind != K_PAR || ni[k].n->op == OP_TAPIN || ni[k].n->op == OP_TAPOUT) statelessIsland = false;
    // blocks kept in flight by a multi-block launch: as many buffer sets as fit in ~140 KB of LDS (one such workgroup per CU)
    copies = 1;
    if (!statelessIsland && slotArea > 0) copies = std::max<uint32_t>(1, std::min<uint32_t>(pb.maxCopies, (35u * 1024u) / slotArea));
    if (pairsTaps) copies = 1;          // a feedback loop through a tap: one block in flight
    slotWords = kSlot0 + copies * slotArea;                    // first word after every copy's buffers
}

uint32_t IslandSchedule::cellFor(Node* c) {
    auto it = cellOf.find(c->rec);
    if (it != cellOf.end()) return it->second;
    const uint32_t word = slotWords + (uint32_t)cellOf.size();
    cellOf.emplace(c->rec, word);
    cells.push_back(ConstCell{word, c->rec});
    return word;
}

uint32_t IslandSchedule::localOf(uint32_t rec) {
    auto it = localRec.find(rec);
    if (it != localRec.end()) return it->second;
    localRec.emplace(rec, (uint32_t)recTable.size());
    recTable.push_back(rec);
    return (uint32_t)recTable.size() - 1u;
}

Member IslandSchedule::makeMember(NI& x) {
    Member m{};
    memberNode.push_back((int)(&x - ni.data()));
    m.rec = localOf(x.rec);
    m.opnd = (uint32_t)operands.size();
    m.outLds = x.needLds ? x.lds : kNone;
    m.outHbm = x.exported ? x.hbm : kNone;
    m.scratch = x.scratch;
    if (x.n->inlets.empty()) {
        m.nin = kNone;
        const uint32_t ar = std::min<uint32_t>(leafArity(x.n->op), kMaxHostIn);
        for (uint32_t c = 0; c < ar; ++c) {
            if (x.kind == K_CHAIN) { operandSrc.push_back(-2 - importFor(c)); operands.push_back(kOpLds | imports[importFor(c)].lds); }
            else { operandSrc.push_back(-1); operands.push_back(kOpHbm | c); }
        }
        return m;
    }
    m.nin = (uint32_t)x.n->inlets.size();
    for (auto& in : x.n->inlets) {
        const int si = pb.srcOf(in);
        if (si < 0) { operandSrc.push_back(-1); operands.push_back(kOpZero); continue; }
        NI& s = ni[si];
        if (s.kind == K_CONST) { operandSrc.push_back(-1); operands.push_back(kOpConst | cellFor(s.n)); }
        else if (s.island == x.island) { operandSrc.push_back(si); operands.push_back(kOpLds | s.lds); }
        else if (x.kind == K_CHAIN) { operandSrc.push_back(-2 - importFor(s.hbm)); operands.push_back(kOpLds | imports[importFor(s.hbm)].lds); }
        else { operandSrc.push_back(-1); operands.push_back(kOpHbm | s.hbm); }
    }
    return m;
}

// A sample-parallel task covers 64*V frames with V in {1,2,4,8} (lane l owns V consecutive
// frames). The block is cut into 64-frame units handed out as power-of-two runs.
void IslandSchedule::emitRanges(uint16_t op, int stage, uint32_t first, uint32_t count, const std::vector<int>& waves) {
    const uint32_t units = (bs + 63) / 64;                      // 64-frame units (8 for a 512 block)
    std::vector<std::pair<uint32_t, uint32_t>> runs;            // (first unit, units)
    if (units == 8 && waves.size() == 3) runs = {{0, 4}, {4, 2}, {6, 2}};
    else {
        uint32_t f = 1;
        while (f * 2 <= waves.size() && f * 2 <= units) f *= 2; // power-of-two wave count
        uint32_t per = (units + f - 1) / f, p2 = 1;
        while (p2 < per) p2 *= 2;                               // units per wave, power of two
        for (uint32_t u = 0; u < units; u += p2) runs.push_back({u, std::min(p2, units - u)});
    }
    for (size_t w = 0; w < runs.size(); ++w) {
        uint32_t u0 = runs[w].first, un = runs[w].second;
        // a non power-of-two tail (block sizes that are not 64 * 2^k) is cut further
        while (un) {
            uint32_t take = 1; while (take * 2 <= un && take * 2 <= 8) take *= 2;
            tasks.push_back(Task{op, (uint8_t)stage, 0, (uint16_t)(u0 * 64), (uint16_t)((u0 + take) * 64), first, count, 0, 0, 0, 0, 0});
            taskWave.push_back(waves[w % waves.size()]);
            if (loadOut) loadOut[waves[w % waves.size()]] += taskCost(op, take, count);
            u0 += take; un -= take;
        }
    }
}

uint32_t IslandSchedule::constMaskOf(const NI& x) const {
    uint32_t mask = 0;
    for (size_t q = 0; q < x.n->inlets.size() && q < 8; ++q) {
        const int si = pb.srcOf(x.n->inlets[q]);
        if (si < 0) { mask |= 1u << q; continue; }   // zero operand
        if (ni[si].kind == K_CONST) mask |= 1u << q;
    }
    return mask;
}

// constant-frequency phasors and blepsaw / blepsquare phase recurrences of one stage share ONE task (device.h OP_PHASE)
bool IslandSchedule::phaseMergeable(const NI& x) const {
    const uint16_t op = x.n->op;
    return e.mergePhases && (op == OP_PHASOR || blepSplit(op)) && !x.n->inlets.empty() && (constMaskOf(x) & 1u);
}

// ---- tasks, stage by stage ----
void IslandSchedule::emitTasks() {
    // A pure sample-parallel island that streams many arena buffers (a mixer: no imports, its children are read
    // straight from HBM by the reduce) is bound by memory round trips, not by issue: its stages are cut into 64-frame
    // runs over ALL eight waves, so one workgroup keeps 8 x 64 child loads in flight.
    mixerLike = false;
    if (statelessIsland && imports.empty() && bs >= 128) {
        size_t direct = 0;
        for (int k : B.nodes)
            for (auto& in : ni[k].n->inlets) {
                const int si = pb.srcOf(in);
                if (si >= 0 && ni[si].kind != K_CONST && ni[si].island != ni[k].island) direct++;
            }
        mixerLike = direct >= 8;
    }
    if (!imports.empty()) {
        const uint32_t first = (uint32_t)members.size();
        for (auto& im : imports) {
            Member m{};
            m.rec = 0; m.opnd = (uint32_t)operands.size(); m.nin = 1; m.outLds = im.lds; m.outHbm = kNone; m.scratch = kNone;
            operandSrc.push_back(-1);
            operands.push_back(kOpHbm | im.hbm);
            memberNode.push_back(-1);
            members.push_back(m);
        }
        emitRanges(OP_COPY, 0, first, (uint32_t)imports.size(), {0, 1, 2, 3});
    }
    // waves that would stay empty with one wave per (stage, task group): a small island hands them to its heavy
    // sample-parallel stages (a finer split), where a big one needs every wave for a slot of its own
    spareWaves = (int)kWaves;
    {
        std::set<std::pair<int, uint32_t>> groups;
        std::map<int, uint32_t> parTotal;
        for (int k : B.nodes) {
            const NI& x = ni[k];
            const uint16_t op = x.n->op;
            if (x.kind == K_CHAIN) groups.insert({x.level - (blepSplit(op) ? 1 : 0), 0x10000u | (phaseMergeable(x) ? (uint32_t)OP_PHASE : (uint32_t)op)});
            else if (x.kind == K_SINGLE) groups.insert({x.level, 0x20000u | (uint32_t)k});
            else if (x.kind == K_PAR) parTotal[x.level] += taskCost(op, 8, 1);
            if (blepSplit(op)) parTotal[x.level] += taskCost(op == OP_BLEPSAW ? OP_SAW_SHAPE : OP_SQUARE_SHAPE, 8, 1);
            if (op == OP_SVF && !coefFused(op)) parTotal[x.level - 1] += taskCost(OP_SVF_COEF, 8, 1);
            if (op == OP_SVFSHELF) parTotal[x.level - 1] += taskCost(OP_SHELF_COEF, 8, 1);
        }
        spareWaves -= (int)groups.size();
        for (auto& kv : parTotal) spareWaves -= kv.second >= 36000u ? 4 : (kv.second >= 18000u ? 2 : 1);
    }
    loadOut = waveLoad;
    for (int stage = base; stage <= maxStage; ++stage) emitStage(stage);
}

void IslandSchedule::emitStage(int stage) {
    std::map<uint32_t, std::vector<int>> chain;   // key: opcode | constMask << 16
    std::map<uint16_t, std::vector<int>> single;
    std::map<std::pair<int, uint16_t>, std::vector<int>> par;   // (fusion depth, opcode): emitted in dependency order
    std::vector<int> phasePhasors, phaseOscs;          // members of this stage's OP_PHASE task
    for (int k : B.nodes) {
        NI& x = ni[k];
        if (x.level == stage + 1 && x.n->op == OP_SVF && !coefFused(OP_SVF)) par[{1 << 20, OP_SVF_COEF}].push_back(k);
        if (x.level == stage + 1 && x.n->op == OP_SVFSHELF) par[{1 << 20, OP_SHELF_COEF}].push_back(k);
        if (x.level == stage + 1 && blepSplit(x.n->op)) {
            if (phaseMergeable(x)) phaseOscs.push_back(k);
            else chain[(uint32_t)x.n->op | (constMaskOf(x) << 16)].push_back(k);
        }
        if (x.level != stage) continue;
        if (blepSplit(x.n->op)) par[{0, x.n->op == OP_BLEPSAW ? OP_SAW_SHAPE : OP_SQUARE_SHAPE}].push_back(k);
        else if (x.n->op == OP_PHASOR && phaseMergeable(x)) phasePhasors.push_back(k);
        else if (x.kind == K_CHAIN) chain[(uint32_t)x.n->op | (constMaskOf(x) << 16)].push_back(k);
        else if (x.kind == K_SINGLE) single[x.n->op].push_back(k);
        else par[{x.sub, x.n->op}].push_back(k);
    }
    // Wave assignment. Inside one block the tasks of a stage want different waves; across the blocks of
    // a pipelined multi-block launch each wave's TOTAL work per block bounds the throughput, so the
    // heavy (serial) tasks go to the wave with the least work so far, idle-in-this-stage waves first.
    uint32_t busy[kWaves] = {};
    // In a pipelined island the long serial tasks get waves 0..3 to themselves and the sample-parallel work
    // runs on waves 4..7: a light task on the critical path of an older block never queues behind a
    // 15-20 k-cycle recurrence of a younger one.
    const int serialWaves = (int)kWaves;   // (dedicating waves 0..3 to the serial tasks was measured: no gain, worse balance)
    auto pickWave = [&]() {
        int b = 0;
        for (int w = 1; w < serialWaves; ++w)
            if (busy[w] < busy[b] || (busy[w] == busy[b] && waveLoad[w] < waveLoad[b])) b = w;
        return b;
    };
    {   // OP_PHASE: up to 64 lanes per task, phasors in front (Task::s0 = how many)
        size_t pi = 0, oi = 0;
        while (pi < phasePhasors.size() || oi < phaseOscs.size()) {
            const uint32_t first = (uint32_t)members.size();
            uint32_t np = 0, cnt = 0;
            for (; pi < phasePhasors.size() && cnt < 64; ++pi, ++np, ++cnt) members.push_back(makeMember(ni[phasePhasors[pi]]));
            for (; oi < phaseOscs.size() && cnt < 64; ++oi, ++cnt) members.push_back(makeMember(ni[phaseOscs[oi]]));
            const int w = pickWave();
            busy[w] += 1; waveLoad[w] += taskCost(OP_PHASE, 8, 1);
            tasks.push_back(Task{OP_PHASE, (uint8_t)stage, 1u, (uint16_t)np, (uint16_t)bs, first, cnt, 0, 0, 0, 0, 0});
            taskWave.push_back(w);
        }
    }
    for (auto& kv : chain) {
        const uint16_t cop = (uint16_t)(kv.first & 0xFFFFu);
        // the double-state filters are wave scans, one node after the other: every node is a task of its own, so that the
        // nodes of a stage (a packed island has one per voice) spread over the waves instead of queueing on one
        const size_t lanes = (cop == OP_SVF || cop == OP_SVFSHELF || cop == OP_MM1P) ? 1 : 64;
        for (size_t off = 0; off < kv.second.size(); off += lanes) {
            const uint32_t cnt = (uint32_t)std::min<size_t>(lanes, kv.second.size() - off);
            const uint32_t first = (uint32_t)members.size();
            for (uint32_t c = 0; c < cnt; ++c) members.push_back(makeMember(ni[kv.second[off + c]]));
            const int w = pickWave();
            busy[w] += 1; waveLoad[w] += taskCost(cop, 8, (cop == OP_SVF || cop == OP_SVFSHELF || cop == OP_MM1P) ? cnt : 1);
            tasks.push_back(Task{cop, (uint8_t)stage, (uint8_t)(kv.first >> 16), 0, (uint16_t)bs, first, cnt, 0, 0, 0, 0, 0});
            taskWave.push_back(w);
        }
    }
    for (auto& kv : single) {
        for (int k : kv.second) {
            const uint32_t first = (uint32_t)members.size();
            members.push_back(makeMember(ni[k]));
            const int w = pickWave();
            busy[w] += 1; waveLoad[w] += taskCost(kv.first, 8, 1);
            tasks.push_back(Task{kv.first, (uint8_t)stage, 0, 0, (uint16_t)bs, first, 1, 0, 0, 0, 0, 0});
            taskWave.push_back(w);
        }
    }
    std::vector<int> freeWaves;
    for (int w = 0; w < (int)kWaves; ++w) if (busy[w] == 0) freeWaves.push_back(w);
    if (freeWaves.empty()) freeWaves.push_back(pickWave());
    std::sort(freeWaves.begin(), freeWaves.end(), [&](int a, int b) { return waveLoad[a] < waveLoad[b]; });
    // Light sample-parallel ops cost mostly per-task overhead. In a pipelined island (blocks overlap, so
    // there is always other work for the other waves) a stage's ops therefore run unsplit on ONE wave
    // unless their cost says otherwise (below).
    std::vector<int> parWaves = freeWaves;
    if (parWaves.size() > 4 && !mixerLike) parWaves.resize(4);   // a finer split only multiplies per-task overhead
    if (copies > 1) {
        // split a stage's sample-parallel work so that one part is about as long as a serial recurrence
        // (~12 k cycles): light stages run unsplit, a filter-coefficient pre-pass on two waves. A finer split
        // shortens the stage but makes its completion wait for the slowest of more, unrelated wave queues.
        uint32_t total = 0;
        for (auto& kv : par) total += taskCost(kv.first.second, 8, (uint32_t)kv.second.size());
        size_t f = total >= 36000u ? 4 : (total >= 18000u ? 2 : 1);
        if (f == 2 && spareWaves >= 2) { f = 4; spareWaves -= 2; }
        else if (f == 1 && total >= 9000u && spareWaves >= 1) { f = 2; spareWaves -= 1; }
        f = std::min(f, parWaves.size());
        parWaves.resize(f);
    }
    for (auto& kv : par) {
        const uint32_t first = (uint32_t)members.size();
        for (int k : kv.second) members.push_back(makeMember(ni[k]));
        emitRanges(kv.first.second, stage, first, (uint32_t)kv.second.size(), parWaves);
    }
}

void IslandSchedule::balanceWaves() {
    // Pipelined island: re-assign whole (stage, wave) slots to waves, longest first (LPT), now that every slot's cost is
    // known — the stage-by-stage choice above cannot see that, e.g., the long final stage is still to come and
    // parks it on the wave that already carries the coefficient stage. Slots of one stage keep distinct waves.
    struct Slot { int stage, wave; uint32_t cost; };
    std::vector<Slot> slots;
    for (size_t q = 0; q < tasks.size(); ++q) {
        const uint32_t cst = taskCost(tasks[q].opcode, ((uint32_t)tasks[q].s1 - tasks[q].s0 + 63u) / 64u, tasks[q].count);
        bool found = false;
        for (Slot& sl : slots) if (sl.stage == tasks[q].stage && sl.wave == taskWave[q]) { sl.cost += cst; found = true; break; }
        if (!found) slots.push_back(Slot{tasks[q].stage, taskWave[q], kSlotGap + cst});
    }
    std::vector<size_t> order(slots.size());
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return slots[a].cost > slots[b].cost; });
    uint32_t load[kWaves] = {};
    std::map<int, uint32_t> usedInStage;                       // stage -> mask of waves taken
    std::map<std::pair<int, int>, int> remap;                  // (stage, old wave) -> new wave
    for (size_t o : order) {
        const Slot& sl = slots[o];
        uint32_t& used = usedInStage[sl.stage];
        // Waves w and w + 4 of the workgroup share a SIMD, and two busy waves on one SIMD slow each other once they mix
        // memory instructions into their VALU stream (a lone-wave recurrence next to another recurrence: ~20 % slower
        // than next to a light slot). Ties on the wave's own load go to the wave whose SIMD mate carries the least:
        // the four heaviest slots land on four different SIMDs, the fifth joins the lightest of them.
        int best = -1;
        auto better = [&](int w, int b) { return load[w] < load[b] || (load[w] == load[b] && load[w ^ 4] < load[b ^ 4]); };
        for (int w = 0; w < (int)kWaves; ++w) if (!((used >> w) & 1u) && (best < 0 || better(w, best))) best = w;
        if (best < 0) for (int w = 0; w < (int)kWaves; ++w) if (best < 0 || better(w, best)) best = w;
        used |= 1u << best; load[best] += sl.cost;
        remap[{sl.stage, sl.wave}] = best;
    }
    for (size_t q = 0; q < tasks.size(); ++q) taskWave[q] = remap.at({(int)tasks[q].stage, taskWave[q]});
    // Program waves w and w + 4 share a SIMD, and a wave loses issue slots to its mate for about half the mate's busy
    // time (specialised C2 voice, tools/spec_trace.py: a recurrence wave alone on its SIMD 7.3-8.8 k cycles per block,
    // 9.4-10.8 k next to a sample-parallel wave of 3.7-5.2 k). Recurrence waves bound the block rate, so each gets a
    // SIMD of its own as far as SIMDs go, the heaviest of them next to the lightest sample-parallel wave.
    {
        bool serial[kWaves] = {};
        for (size_t q = 0; q < tasks.size(); ++q) if (kindOf(tasks[q].opcode) == K_CHAIN) serial[taskWave[q]] = true;
        std::vector<int> ser, par;
        for (int w = 0; w < (int)kWaves; ++w) (serial[w] ? ser : par).push_back(w);
        std::stable_sort(ser.begin(), ser.end(), [&](int a, int b) { return load[a] > load[b]; });
        std::stable_sort(par.begin(), par.end(), [&](int a, int b) { return load[a] < load[b]; });
        if (ser.size() <= 4 && !ser.empty()) {
            int renum[kWaves];
            std::vector<int> rest;                       // waves still to place, mates first
            size_t pi = 0;
            for (size_t k = 0; k < ser.size(); ++k) { renum[ser[k]] = (int)k; if (pi < par.size()) renum[par[pi++]] = (int)k + 4; }
            int freeIdx[kWaves]; int nf = 0;
            bool taken[kWaves] = {};
            for (size_t k = 0; k < ser.size(); ++k) { taken[k] = true; if (k < par.size()) taken[k + 4] = true; }
            for (int w = 0; w < (int)kWaves; ++w) if (!taken[w]) freeIdx[nf++] = w;
            for (int f = 0; pi < par.size() && f < nf; ++f) renum[par[pi++]] = freeIdx[f];
            for (size_t q = 0; q < tasks.size(); ++q) taskWave[q] = renum[taskWave[q]];
        }
    }
}

void IslandSchedule::orderTasks() {
    {   // per-wave task lists: sort by (wave, stage), keep emission order inside a (wave, stage)
        std::vector<size_t> order(tasks.size());
        std::iota(order.begin(), order.end(), (size_t)0);
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
            return taskWave[a] != taskWave[b] ? taskWave[a] < taskWave[b] : tasks[a].stage < tasks[b].stage; });
        std::vector<Task> sorted; sorted.reserve(tasks.size());
        for (uint32_t w = 0; w <= kWaves; ++w) I.waveTask[w] = 0;
        for (size_t q : order) { sorted.push_back(tasks[q]); I.waveTask[taskWave[q] + 1]++; }
        for (uint32_t w = 0; w < kWaves; ++w) I.waveTask[w + 1] += I.waveTask[w];
        tasks.swap(sorted);
    }
    for (Task& t : tasks) {   // inline member 0 into the task header
        const Member& m0 = members[t.first];
        const uint32_t nops = m0.nin == kNone ? std::min<uint32_t>(leafArityOfOp(t.opcode), kMaxHostIn) : m0.nin;
        t.o0 = nops > 0 ? operands[m0.opnd] : (uint32_t)kOpZero;
        t.o1 = nops > 1 ? operands[m0.opnd + 1] : (uint32_t)kOpZero;
        t.outLds16 = m0.outLds == kNone ? (uint16_t)0xFFFF : (uint16_t)m0.outLds;
        t.nin16 = m0.nin == kNone ? (uint16_t)0xFFFF : (m0.nin >= 0xFFFE ? (uint16_t)0xFFFE : (uint16_t)m0.nin);
        t.outHbm = m0.outHbm;
        // fast sample-parallel task (kernels.hip run_fast): single member, math opcode, all
        // operands in LDS, arity satisfied (no zero-fill case), not a leaf
        const bool unary = t.opcode >= OP_SIN && t.opcode <= OP_ABS;
        const bool binary = t.opcode >= OP_LE && t.opcode <= OP_OR;
        const bool reduce2 = t.opcode >= OP_ADD && t.opcode <= OP_MAX;
        auto inLds = [](uint32_t o) { return (o & kOpKindMask) != kOpHbm; };
        if (t.count == 1 && m0.nin != kNone && (m0.outLds == kNone || m0.outLds < 0xFFFFu) &&
            ((unary && m0.nin >= 1 && inLds(t.o0)) || (binary && m0.nin >= 2 && inLds(t.o0) && inLds(t.o1)) ||
             (reduce2 && m0.nin == 2 && inLds(t.o0) && inLds(t.o1))) &&
            (m0.outLds != kNone || m0.outHbm != kNone))
            t.flags |= 0x80u;
    }
    if (copies > 1) {   // recurrence tasks that have a wave to themselves render all blocks of a launch in one go (kTaskOwnsWave)
        for (uint32_t w = 0; w < kWaves; ++w) {
            if (I.waveTask[w + 1] - I.waveTask[w] != 1u) continue;
            Task& t = tasks[I.waveTask[w]];
            const uint16_t op = t.opcode;
            const bool plain = op == OP_PHASOR || op == OP_SPHASOR || op == OP_POLE || op == OP_ENV || op == OP_BIQUAD || op == OP_COUNTER ||
                               op == OP_ACCUM || op == OP_LATCH || op == OP_MAXHOLD || op == OP_PHASE;
            const bool osc = blepSplit(op) && (t.flags & 1u);            // constant frequency: no per-block pre-pass
            if (!plain && !osc) continue;
            bool ok = (t.flags & 0xC0u) == 0u;
            for (uint32_t k = 0; k < t.count && ok; ++k) {
                const Member& m = members[t.first + k];
                if (m.outHbm != kNone || m.outLds == kNone || m.nin == kNone || m.nin < leafArityOfOp(op)) ok = false;
            }
            if (ok) t.flags |= (uint8_t)kTaskOwnsWave;
        }
    }
    // (A mixer used to run as 8 workgroups, each rendering a 64-frame slice with ONE active wave; the slices are now the
    // eight waves of one workgroup — same latency for a single block, and a multi-block launch gives every block its own
    // workgroup. Level 1 of C2: 48 -> 22 us per launch set. `mixer_split` = 2 keeps two workgroups of four active waves: the
    // single-block launch stays at 13 us where one workgroup of eight needs 21.)
    I.split = 1u;
    if (mixerLike) {   // slices must be whole 64-frame units: the largest divisor of the block's unit count within the option
        const uint32_t units = bs / 64u;
        uint32_t parts = bs % 64u == 0u ? std::max(1u, std::min(e.mixerSplit, units)) : 1u;
        while (parts > 1u && units % parts != 0u) --parts;
        I.split = parts;
    }
}

// stage tables: tasks per stage, previous non-empty stage, per-wave first task of each stage
void IslandSchedule::pipelineTables() {
    S = (uint32_t)maxStage + 1;
    stageTab.assign(2 * S + kWaves * (S + 1) + copies + 1, 0u);
    schedRel = 0;
    for (const Task& t : tasks) stageTab[t.stage]++;
    {
        uint32_t prev = kNone;
        for (uint32_t st = 0; st < S; ++st) { stageTab[S + st] = prev; if (stageTab[st]) prev = st; }
        for (uint32_t w = 0; w < kWaves; ++w) {
            uint32_t* begin = stageTab.data() + 2 * S + w * (S + 1);
            uint32_t ti = I.waveTask[w];
            for (uint32_t st = 0; st <= S; ++st) {
                while (ti < I.waveTask[w + 1] && tasks[ti].stage < st) ++ti;
                begin[st] = ti;
            }
        }
    }
    {   // phases of the block pipeline: `copies` runs of consecutive stages minimising the costliest run,
        // a stage costing what its busiest wave spends in it (the stages of one phase run back to back)
        std::vector<uint32_t> cost(S, 0u);
        {
            std::vector<std::array<uint32_t, kWaves>> perWave(S);
            for (auto& a : perWave) a.fill(0u);
            for (size_t q = 0; q < tasks.size(); ++q) {
                const Task& t = tasks[q];
                uint32_t w = 0; while (w + 1 < kWaves && q >= I.waveTask[w + 1]) ++w;
                const uint16_t op = t.opcode;
                const uint32_t units = ((uint32_t)t.s1 - t.s0 + 63u) / 64u;
                const uint32_t cst = taskCost(op, units, t.count);
                perWave[t.stage][w] += cst;
            }
            for (uint32_t st = 0; st < S; ++st) cost[st] = 1500u + *std::max_element(perWave[st].begin(), perWave[st].end());
        }
        const uint32_t P = std::min<uint32_t>(copies, S);
        // dp[p][j]: best max-run cost covering stages [0, j) with p runs
        const uint64_t INF = ~0ull;
        std::vector<std::vector<uint64_t>> dp(P + 1, std::vector<uint64_t>(S + 1, INF));
        std::vector<std::vector<uint32_t>> cut(P + 1, std::vector<uint32_t>(S + 1, 0u));
        std::vector<uint64_t> pre(S + 1, 0);
        for (uint32_t j = 0; j < S; ++j) pre[j + 1] = pre[j] + cost[j];
        dp[0][0] = 0;
        for (uint32_t pp = 1; pp <= P; ++pp)
            for (uint32_t j = pp; j <= S; ++j)
                for (uint32_t i0 = pp - 1; i0 < j; ++i0) {
                    if (dp[pp - 1][i0] == INF) continue;
                    const uint64_t v = std::max(dp[pp - 1][i0], pre[j] - pre[i0]);
                    if (v < dp[pp][j]) { dp[pp][j] = v; cut[pp][j] = i0; }
                }
        uint32_t* phase = stageTab.data() + 2 * S + kWaves * (S + 1);
        for (uint32_t d = 0; d <= copies; ++d) phase[d] = S;     // unused trailing phases are empty
        uint32_t j = S;
        for (uint32_t pp = P; pp >= 1; --pp) { phase[pp] = j; j = cut[pp][j]; }
        phase[0] = 0;
        for (uint32_t d = P + 1; d <= copies; ++d) phase[d] = S;
    }
    {   // per-wave walk of the block pipeline: only the (stage, phase) slots where the wave has tasks, in the
        // order the kernel visits them inside a macro-step (stage offset inside the phase ascending, oldest
        // block = highest phase first); 8 dwords each: stage, phase, first task, end task, prev stage, its task count
        const size_t base = 2 * S + kWaves * (S + 1);
        std::vector<uint32_t> phaseOf(S, 0u);
        for (uint32_t d = 0; d < copies; ++d) for (uint32_t st = stageTab[base + d]; st < stageTab[base + d + 1]; ++st) phaseOf[st] = d;
        std::vector<uint32_t> offs(kWaves + 1, 0u), entries;
        for (uint32_t w = 0; w < kWaves; ++w) {
            const uint32_t* begin = stageTab.data() + 2 * S + w * (S + 1);
            std::vector<uint32_t> mine;
            for (uint32_t st = 0; st < S; ++st) if (begin[st + 1] > begin[st]) mine.push_back(st);
            std::stable_sort(mine.begin(), mine.end(), [&](uint32_t a, uint32_t b) {
                const uint32_t sla = a - stageTab[base + phaseOf[a]], slb = b - stageTab[base + phaseOf[b]];
                return sla != slb ? sla < slb : phaseOf[a] > phaseOf[b]; });
            // the kernel polls a wave's slots in table order and runs the first ready one: later stages first, so the
            // oldest blocks drain (and release their buffer sets) before younger ones are started
            std::sort(mine.begin(), mine.end(), [](uint32_t a, uint32_t b) { return a > b; });
            for (uint32_t st : mine) {
                const uint32_t prev = stageTab[S + st];
                const uint32_t e[8] = {st, phaseOf[st], begin[st], begin[st + 1], prev, prev == kNone ? 0u : stageTab[prev], 0u, 0u};
                entries.insert(entries.end(), e, e + 8);
            }
            offs[w + 1] = (uint32_t)entries.size() / 8u;
        }
        while ((stageTab.size() + offs.size()) % 4) stageTab.push_back(0u);   // entries are read with 16-byte LDS loads
        schedRel = (uint32_t)stageTab.size();
        stageTab.insert(stageTab.end(), offs.begin(), offs.end());
        stageTab.insert(stageTab.end(), entries.begin(), entries.end());
    }
}

// ---- specialised-kernel variant of the program (codegen.cpp): recurrence streams through the HBM arena --------------
// On a lone wavefront every instruction costs ~4 cycles and an LDS access 12-50, so a specialised kernel moves the
// blocks a float recurrence reads and writes through L2 instead: inputs arrive by scalar loads (16 frames per
// instruction), outputs leave as lane-0 global stores. The interpreter program above is left as it is (same LDS
// layout); the variant only re-routes operands / outputs and names the arena buffers it needs extra.
void IslandSchedule::specVariant() {
    // (stateless islands too — mixers, root gains: their specialised kernel has no block pipeline, blocks go over gridDim.y)
    specIsland = pb.wantSpec && bs % 64u == 0u;   // (vector loads of a 64-frame unit must stay inside their arena buffer)
    if (specIsland) {
        sp.members = members; sp.operands = operands;
        sp.gdirect.assign(tasks.size(), 0);
        std::unordered_map<int, uint32_t> streamOf;        // NI index -> arena buffer carrying the node's output
        auto stream = [&](int k) -> uint32_t {
            if (ni[k].exported) return ni[k].hbm;
            auto it = streamOf.find(k);
            if (it != streamOf.end()) return it->second;
            const uint32_t b = kOpStream | p.numStreamBuffers++;     // a buffer of the stream ring (device.h kOpStream)
            streamOf.emplace(k, b);
            return b;
        };
        auto streamFamily = [&](const Task& t) {
            switch (t.opcode) {
                case OP_PHASOR: case OP_SPHASOR: case OP_POLE: case OP_ENV: case OP_BIQUAD: case OP_COUNTER: case OP_ACCUM:
                case OP_LATCH: case OP_MAXHOLD: case OP_PHASE: return true;
                case OP_BLEPSAW: case OP_BLEPSQUARE: return (t.flags & 1u) != 0u;   // constant frequency: no in-place pre-pass
                default: return false;
            }
        };
        std::unordered_map<int, uint32_t> phaseStream;      // split oscillator: arena buffer of its phase (recurrence -> waveform task)
        std::unordered_set<int> streamed;                   // nodes whose output lives in the arena only (no LDS copy in the variant)
        for (size_t q = 0; q < tasks.size(); ++q) {
            const Task& t = tasks[q];
            if (!streamFamily(t)) continue;
            bool ok = true;
            for (uint32_t k = 0; k < t.count; ++k) {
                const Member& m = members[t.first + k];
                if (m.nin == kNone || m.nin < leafArityOfOp(t.opcode) || memberNode[t.first + k] < 0) ok = false;
            }
            if (!ok) continue;
            sp.gdirect[q] = 1;
            for (uint32_t k = 0; k < t.count; ++k) {
                const uint32_t mi = t.first + k;
                const int x = memberNode[mi];
                const bool osc = blepSplit(ni[x].n->op);            // (an OP_PHASE task carries both kinds)
                uint32_t b;
                if (osc) { b = kOpStream | p.numStreamBuffers++; phaseStream.emplace(x, b); }
                else { b = stream(x); streamed.insert(x); }
                sp.members[mi].outHbm = b;
                for (uint32_t j = 0; j < members[mi].nin; ++j) {
                    const uint32_t oi = members[mi].opnd + j;
                    if ((operands[oi] & kOpKindMask) != kOpLds) continue;
                    const int src = operandSrc[oi];
                    if (src >= 0) sp.operands[oi] = kOpHbm | stream(src);
                    else if (src <= -2) sp.operands[oi] = kOpHbm | imports[(size_t)(-2 - src)].hbm;
                }
            }
        }
        // producers of streamed operands also write the arena; consumers of streamed nodes read it
        for (size_t mi = 0; mi < members.size(); ++mi) {
            const int x = memberNode[mi];
            if (x < 0) continue;
            auto it = streamOf.find(x);
            if (it != streamOf.end() && sp.members[mi].outHbm == kNone) sp.members[mi].outHbm = it->second;
        }
        for (size_t oi = 0; oi < operands.size(); ++oi) {
            const int src = operandSrc[oi];
            if (src >= 0 && streamed.count(src) && (operands[oi] & kOpKindMask) == kOpLds) sp.operands[oi] = kOpHbm | stream(src);
        }
        // the waveform task of a streamed oscillator reads the phase from the arena (member operand slot 5)
        sp.phaseOp.assign(members.size(), (uint32_t)kOpZero);
        for (size_t q = 0; q < tasks.size(); ++q) {
            if (tasks[q].opcode != OP_SAW_SHAPE && tasks[q].opcode != OP_SQUARE_SHAPE) continue;
            for (uint32_t k = 0; k < tasks[q].count; ++k) {
                auto it = phaseStream.find(memberNode[tasks[q].first + k]);
                if (it != phaseStream.end()) sp.phaseOp[tasks[q].first + k] = kOpHbm | it->second;
            }
        }
        // the oscillator's recurrence member and its waveform member are the same node: only the waveform member exports it
        for (size_t q = 0; q < tasks.size(); ++q)
            if ((blepSplit(tasks[q].opcode) || tasks[q].opcode == OP_PHASE) && !sp.gdirect[q])
                for (uint32_t k = 0; k < tasks[q].count; ++k) {
                    const int x = memberNode[tasks[q].first + k];
                    if (x >= 0 && blepSplit(ni[x].n->op)) sp.members[tasks[q].first + k].outHbm = members[tasks[q].first + k].outHbm;
                }
        // arena table: every absolute arena index the variant names, in order of first appearance
        auto ref = [&](uint32_t abs) { for (uint32_t v : sp.hbmTab) if (v == abs) return; sp.hbmTab.push_back(abs); };
        for (const Member& m : sp.members) if (m.outHbm != kNone) ref(m.outHbm);
        for (uint32_t o : sp.operands) if ((o & kOpKindMask) == kOpHbm) ref(o & kOpValMask);
        for (uint32_t o : sp.phaseOp) if ((o & kOpKindMask) == kOpHbm) ref(o & kOpValMask);
    }
}

// pack the blob: copies x [tasks | members | operands] | cells | stage tables
void IslandSchedule::packBlob() {
    static_assert(sizeof(Task) == 32 && sizeof(Member) == 32 && sizeof(ConstCell) == 8, "program layout");
    I.progBegin = (uint32_t)p.prog.size();
    I.numTasks = (uint32_t)tasks.size();
    I.memOff = I.numTasks * 8u;
    I.opndOff = I.memOff + (uint32_t)members.size() * 8u;
    I.copyDwords = (I.opndOff + (uint32_t)operands.size() + 3u) & ~3u;
    I.copies = copies;
    I.slotArea = slotArea;
    I.stateless = statelessIsland ? 1u : 0u;
    I.cellOff = I.copyDwords * copies;
    I.numCells = (uint32_t)cells.size();
    I.stageOff = (I.cellOff + I.numCells * 2u + 3u) & ~3u;
    I.schedOff = I.stageOff + schedRel;
    I.recOff = I.stageOff + (uint32_t)stageTab.size();
    I.numRecs = (uint32_t)recTable.size();
    // + the specialised variant's arena table and its operand table (same indexing as the interpreter's; wide fan-in ops
    //   fetch operand codes from the staged table at run time)
    I.progDwords = I.recOff + I.numRecs + (uint32_t)sp.hbmTab.size() + (uint32_t)sp.operands.size();
    p.prog.resize((size_t)I.progBegin + I.progDwords);
    for (uint32_t d = 0; d < copies; ++d) {
        const uint32_t off = d * slotArea;
        auto adjOp = [&](uint32_t o) { return (o & kOpKindMask) == kOpLds ? o + off : o; };
        std::vector<Task> tc(tasks);
        std::vector<Member> mc(members);
        std::vector<uint32_t> oc(operands);
        for (Task& t : tc) { t.o0 = adjOp(t.o0); t.o1 = adjOp(t.o1); if (t.outLds16 != 0xFFFFu) t.outLds16 = (uint16_t)(t.outLds16 + off); }
        for (Member& m : mc) { if (m.outLds != kNone) m.outLds += off; if (m.scratch != kNone) m.scratch += off; }
        for (uint32_t& o : oc) o = adjOp(o);
        uint32_t* blob = p.prog.data() + I.progBegin + (size_t)d * I.copyDwords;
        if (!tc.empty()) std::memcpy(blob, tc.data(), tc.size() * sizeof(Task));
        if (!mc.empty()) std::memcpy(blob + I.memOff, mc.data(), mc.size() * sizeof(Member));
        if (!oc.empty()) std::memcpy(blob + I.opndOff, oc.data(), oc.size() * 4);
    }
    {
        uint32_t* blob = p.prog.data() + I.progBegin;
        if (!cells.empty()) std::memcpy(blob + I.cellOff, cells.data(), cells.size() * sizeof(ConstCell));
        std::memcpy(blob + I.stageOff, stageTab.data(), stageTab.size() * 4);
        if (!recTable.empty()) std::memcpy(blob + I.recOff, recTable.data(), recTable.size() * 4);
        if (!sp.hbmTab.empty()) std::memcpy(blob + I.recOff + I.numRecs, sp.hbmTab.data(), sp.hbmTab.size() * 4);
        if (!sp.operands.empty()) std::memcpy(blob + I.recOff + I.numRecs + sp.hbmTab.size(), sp.operands.data(), sp.operands.size() * 4);
    }
    while (p.prog.size() % 4) p.prog.push_back(0);   // keep every blob 16-byte aligned
    I.numStages = S;
    I.ldsProg = (slotWords + (uint32_t)cellOf.size() + 3u) & ~3u;
    I.ldsCounters = (I.ldsProg + I.progDwords + 3u) & ~3u;
    I.ldsNext = (I.ldsCounters + S * copies + 3u) & ~3u;
    I.ldsRecs = (I.ldsNext + S * kWaves + 3u) & ~3u;
    I.ldsWords = (I.ldsRecs + I.numRecs * kRecDwords + 3u) & ~3u;
}

// the generated kernel text of the island's shape (null: interpreter only), from the engine's text cache
std::shared_ptr<SpecText> IslandSchedule::specText() {
    if (!specIsland || !(I.split == 1u || statelessIsland)) return nullptr;
    // signature of everything the text is a function of (arena indices by their position in the island's arena table)
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint32_t v) { h ^= v; h *= 1099511628211ull; h ^= h >> 29; };
    auto arenaPos = [&](uint32_t abs) { for (size_t k = 0; k < sp.hbmTab.size(); ++k) if (sp.hbmTab[k] == abs) return (uint32_t)k | (abs & kOpStream); return 0xFFFFu; };
    const uint32_t* iw = reinterpret_cast<const uint32_t*>(&I);
    for (size_t k = 0; k < sizeof(Island) / 4; ++k) if (k != offsetof(Island, progBegin) / 4 && k != offsetof(Island, rootRec) / 4) mix(iw[k]);
    for (const Task& t : tasks) { const uint32_t* w = reinterpret_cast<const uint32_t*>(&t); for (int k = 0; k < 8; ++k) mix(k == 7 ? 0u : w[k]); }   // (t.outHbm: absolute, not part of the text)
    for (const Member& m : sp.members) { mix(m.rec); mix(m.opnd); mix(m.nin); mix(m.outLds); mix(m.outHbm == kNone ? kNone : arenaPos(m.outHbm)); mix(m.scratch); }
    for (uint32_t o : sp.operands) mix((o & kOpKindMask) == kOpHbm ? (kOpHbm | arenaPos(o & kOpValMask)) : o);
    for (uint32_t o : sp.phaseOp) mix((o & kOpKindMask) == kOpHbm ? (kOpHbm | arenaPos(o & kOpValMask)) : o);
    for (uint8_t g : sp.gdirect) mix(g);
    for (uint32_t k = 0; k < 2 * S; ++k) mix(stageTab[k]);
    mix(bs); mix((uint32_t)sp.hbmTab.size());
    auto it = e.specTextCache.find(h);
    if (it == e.specTextCache.end()) {
        auto txt = std::make_shared<SpecText>();
        txt->text = emitSpecSource(I, tasks, sp, stageTab, bs);
        it = e.specTextCache.emplace(h, std::move(txt)).first;
    }
    return it->second;
}

// the fresh program becomes the plan's and the caches'; plan_cache = 2 compares it with what the caches would have given
void IslandSchedule::recordProgram() {
    auto ent = newEntry(std::vector<uint32_t>(p.prog.begin() + I.progBegin, p.prog.end()));
    ent->specHbmTab = (uint32_t)sp.hbmTab.size();
    ent->spec = specText();
    ent->numMembers = (uint32_t)members.size(); ent->numOperands = (uint32_t)operands.size();
    ent->streamDelta = p.numStreamBuffers - streamStart;
    adoptProgram(ent);
    if (skey != 0 && e.planCache != 0 && !e.islandShapeCache.count(skey)) e.islandShapeCache[skey] = ent;
    if (!relocated.empty()) {       // plan_cache = 2: the twin's renamed program must be what was just scheduled
        if (relocated != ent->blob) { e.st.planRelocationMismatches++; std::fprintf(stderr, "[elemhip] plan cache: island %zu: the relocated program of its twin differs from its own schedule\n", ii); }
        else e.st.planIslandsRelocated++;
        relocated.clear();
    }
    if (cached) {          // plan_cache = 2: the cached program must be what was just scheduled
        Island a = cached->I, b2 = I;
        a.progBegin = b2.progBegin = 0u; a.rootRec = b2.rootRec = 0u;
        const bool same = std::memcmp(&a, &b2, sizeof(Island)) == 0 && cached->blob == ent->blob && cached->spec == ent->spec &&
                          cached->streamDelta == ent->streamDelta && cached->numMembers == ent->numMembers;
        if (!same) { e.st.planCacheMismatches++; std::fprintf(stderr, "[elemhip] plan cache: island %zu differs from its cached program\n", ii); }
    }
    if (e.planCache != 0) { e.islandCache[ikey] = std::move(ent); e.st.planIslandsScheduled++; }
}

} // namespace elemhip
