// plan_build.h — private to the planner: what the passes of one plan build share. plan.cpp holds the graph-level passes
// (render order, islands, launch levels, taps), Engine::buildPlan and Engine::describePlan; plan_island.cpp holds the work on
// one island (descriptors, program cache, schedule, LDS allocation, task emission, pipeline tables, specialised variant).
#pragma once
#include <chrono>
#include <cstdlib>
#include <unordered_map>

#include "engine.h"

namespace elemhip {

enum Kind : uint8_t { K_CONST, K_PAR, K_SINGLE, K_CHAIN, K_CONV, K_HOST };

inline Kind kindOf(uint16_t op) {
    switch (op) {
        case OP_CONST: case OP_SR: return K_CONST;
        case OP_RAND: case OP_Z: case OP_SDELAY: case OP_DELAY: case OP_SAMPLESEQ: case OP_METER: case OP_SNAPSHOT: case OP_SCOPE: case OP_CAPTURE: case OP_FFT: return K_SINGLE;
        case OP_CONVOLVE: return K_CONV;   // always an island of its own, rendered by conv.hip
        case OP_HOST: return K_HOST;       // always an island of its own, rendered on the CPU between launch levels
        case OP_PHASOR: case OP_SPHASOR: case OP_COUNTER: case OP_ACCUM: case OP_LATCH: case OP_MAXHOLD:
        case OP_ONCE: case OP_SEQ: case OP_SEQ2: case OP_SPARSEQ: case OP_SAMPLE: case OP_MCSAMPLE: case OP_POLE: case OP_ENV: case OP_BIQUAD: case OP_MM1P: case OP_SVF:
        case OP_SVFSHELF: case OP_BLEPSAW: case OP_BLEPSQUARE: case OP_BLEPTRIANGLE: case OP_PHASE:
            return K_CHAIN;
        default: return K_PAR;
    }
}

inline uint32_t scratchSlots(uint16_t op) {
    switch (op) {
        case OP_SVF: return 6;        // a1,a2,a3 as double (coefficient pre-pass -> scan)
        case OP_SVFSHELF: return 10;  // a1,a2,a3,k,A
        case OP_DELAY: return 1;
        case OP_SAMPLESEQ: return 2;  // per-reader fade gains
        case OP_SAMPLE: case OP_MCSAMPLE: return 6;     // per reader: read index, fraction, gain (serial pass -> gather pass)
        default: return 0;
    }
}

// inputs a task of this opcode reads when its first member is a leaf (codegen.cpp asks too)
uint32_t leafArityOfOp(uint16_t op);
std::string emitSpecSource(const Island& I, const std::vector<Task>& tasks, const SpecProgram& sp,
                           const std::vector<uint32_t>& stageTab, uint32_t blockSize);   // codegen.cpp

inline bool planTiming() { static const bool on = std::getenv("ELEMHIP_PLAN_TIMING") != nullptr; return on; }   // phase times of a build on stderr

struct NI {                      // per-node planning info
    Node* n = nullptr;
    int seq = 0;                 // owning root sequence
    int pos = 0;                 // position in the global render order
    Kind kind = K_PAR;
    int island = -1;
    int level = 0;               // stage inside the island
    int sub = 0;                 // depth inside a fused run of sample-parallel ops of one stage
    bool needLds = false;
    bool exported = false;
    uint32_t lds = kNone;        // LDS word offset of the output slot
    uint32_t hbm = kNone;        // HBM arena index
    uint32_t scratch = kNone;
    int lastUse = 0;             // last in-island consumer stage
    int fusedRoot = -1;          // convolve: NI index of the root whose gain this node applies itself (the root has no task)
    bool elided = false;         // `in` leaf read directly by convolvers / root folded into its convolver: never a task
    uint32_t ch = 0;             // output channel of a multi-output node this entry renders
    uint32_t rec = kNone;        // node record (a multi-output node has one per channel)
};

struct IslandBuild {
    std::vector<int> nodes;      // NI indices in render order
    int seq = 0;
    int level = 0;               // launch level
    std::vector<int> deps;       // islands it imports from
};

// (node id, channel) -> NI index: open addressing, sized once per build. The planner asks this table about every inlet in every
// phase (~20 lookups per node and build); a node-per-entry std::unordered_map made the render-order phase allocation-bound.
struct FlatIdx {
    struct Slot { int64_t first; int second; };
    std::vector<Slot> tab;
    uint64_t mask = 0;
    static constexpr int64_t kEmpty = INT64_MIN;
    static uint64_t hash(int64_t k) { uint64_t h = (uint64_t)k * 0x9E3779B97F4A7C15ull; return h ^ (h >> 29); }
    void reserve(size_t n) { size_t cap = 64; while (cap < 2 * n) cap <<= 1; tab.assign(cap, Slot{kEmpty, 0}); mask = cap - 1; used = 0; }
    size_t used = 0;
    int& operator[](int64_t k) {
        if (2 * (used + 1) > tab.size()) {   // (multi-output nodes add an entry per channel: grow, keep the load under one half)
            std::vector<Slot> old;
            old.swap(tab);
            tab.assign(std::max<size_t>(64, 2 * old.size()), Slot{kEmpty, 0}); mask = tab.size() - 1; used = 0;
            for (const Slot& o : old) if (o.first != kEmpty) (*this)[o.first] = o.second;
        }
        for (uint64_t i = hash(k) & mask;; i = (i + 1) & mask) {
            if (tab[i].first == k) return tab[i].second;
            if (tab[i].first == kEmpty) { tab[i].first = k; ++used; return tab[i].second; }
        }
    }
    const Slot* find(int64_t k) const {
        if (tab.empty()) return nullptr;
        for (uint64_t i = hash(k) & mask;; i = (i + 1) & mask) {
            if (tab[i].first == k) return &tab[i];
            if (tab[i].first == kEmpty) return nullptr;
        }
    }
    size_t count(int64_t k) const { return find(k) ? 1 : 0; }
    int at(int64_t k) const { const Slot* s = find(k); if (!s) throw std::out_of_range("plan index"); return s->second; }
};

struct PlanBuilder {
    Engine& e;
    std::shared_ptr<Plan> plan = std::make_shared<Plan>();
    Plan& p = *plan;
    const uint32_t bs;
    PlanBuilder(Engine& eng, uint32_t packIslands);    // options as the engine has them; `packIslands`: what this attempt packs (buildPlan)
    // null: failed (stderr says why). Plan::heapOverflowDwords set: the program heap lacks room, nothing else of the plan is valid
    std::shared_ptr<Plan> build(uint32_t maxIslandNodes, uint32_t maxCopies);

    // ---- options and results ----
    uint32_t maxIslandNodes = 0, maxCopies = 1;
    bool splitCoefStage = false;
    bool wantSpec = false;                  // also write the specialised-kernel text of every pipelined island
    uint32_t packK = 1;                     // merge up to this many same-shape islands of a launch level into one (lane-packing); 0 = as many as it takes
    uint32_t packMax = 2, cuCount = 256;    // ... to bring the fullest launch level down to the CU count, at most packMax
    bool packRoots = false;                 // option "pack_roots": merge across root sequences (active roots only)
    uint32_t packedIslands = 0;             // out: islands that disappeared into another
    uint32_t minPackedCopies = 0;           // out: fewest buffer sets of an island that carries more than one original island
    uint32_t statefulIslandsMax = 0;        // out: most stateful islands of one launch level (before packing)

    // ---- graph-level state, in the order the passes fill it ----
    std::vector<NI> ni;
    // (node id, output channel) -> NI index. Multi-output nodes (mc.*, GraphRenderSequence.h:15-24) are planned as one
    // single-output entry per channel; every other node only has channel 0, so an inlet that names another channel of it
    // finds nothing and reads as a missing input, like before.
    FlatIdx idx;
    static int64_t K(int32_t id, uint32_t ch = 0) { return ((int64_t)id << 8) | (int64_t)(ch & 0xFFu); }
    std::vector<std::vector<int>> seqNodes; // per root sequence
    std::vector<Node*> seqRoots;
    std::vector<IslandBuild> ib;            // canonical island list (dense, in order of first appearance)
    std::vector<uint32_t> packCount;        // original islands inside each island
    int numLevels = 0;
    std::vector<int> tapWriter;             // tapIn NI index -> NI index of the tapOut it is paired with
    std::vector<char> islandPairsTaps;
    std::vector<uint32_t> scheduled;        // islands whose program this build made (p.prog holds them, progBegin relative to it)
    std::vector<int> convLevel;             // launch level of p.convs[i]

    // (node, channel) of an inlet -> planner entry (-1: none), through the memo the render-order walk left in the inlet (no
    // hashing): the ~20 questions per inlet the passes ask
    uint32_t buildEpoch = 0;
    int srcOf(const Inlet& in) const {
        const Node* c = in.srcEpoch == e.nodesEpoch ? in.src : nullptr;
        if (c) return (c->planVisited != buildEpoch || in.channel >= c->planChans) ? -1 : c->planIdx + (int)in.channel;
        const FlatIdx::Slot* s = idx.find(K(in.source, in.channel));      // (an inlet of a node the walk did not reach, a missing source)
        return s ? s->second : -1;
    }

    // ---- passes, in build order (plan.cpp) ----
    void traverse(uint32_t epoch, std::vector<Node*>& order, Node* root);
    void renderOrder();
    void foldIntoConvolve();
    void formIslands();
    bool levelIslands();
    void packIslands();
    void assignArena();
    void pairTaps();
    bool planIsland(size_t ii);             // plan_island.cpp
    void emitConvDesc(size_t ii);
    void emitHostDesc(size_t ii);
    bool placePrograms();
    bool levelTables();
    // after the build (Engine::buildPlan)
    static double groupShapes(Engine& e, Plan& p);
    struct Tables { size_t islands, level, roots, taps, convs, convWork, specLists, rest; std::vector<uint8_t> host; };
    static Tables packTables(const Plan& p);

    std::chrono::steady_clock::time_point tPhase;
    int phaseNo = 0;
    void phase(const char* name);           // closes a timed phase (Plan::buildUs, ELEMHIP_PLAN_TIMING)
};

// One island's schedule: lives for one iteration of the island loop (PlanBuilder::planIsland, plan_island.cpp).
struct IslandSchedule {
    PlanBuilder& pb;
    Engine& e;
    Plan& p;
    std::vector<NI>& ni;
    const size_t ii;
    IslandBuild& B;
    Island& I;
    const uint32_t bs, packed;              // block size; original islands inside this one
    const bool pairsTaps;
    const uint32_t streamStart;             // stream buffers handed out before this island
    const std::vector<uint32_t> memberIds;  // {node id, opcode | channel << 16, record, arena buffer} per member (IslandProgram::members)
    IslandSchedule(PlanBuilder& b, size_t island);

    // program cache
    uint64_t ikey = 0, skey = 0;
    std::shared_ptr<IslandProgram> cached;  // exact hit (program on the device already)
    std::vector<uint32_t> canonRecs, canonHbms;   // the island's records / arena buffers in the order its canonical walk meets them
    std::vector<uint32_t> relocated;        // plan_cache = 2: the twin's renamed program, to be compared with the fresh schedule
    uint64_t islandKey(bool structural);
    bool takeFromCache();
    void adoptCached();
    bool relocateTwin(const std::shared_ptr<IslandProgram>& twin);
    std::shared_ptr<IslandProgram> newEntry(std::vector<uint32_t>&& blob);
    void adoptProgram(const std::shared_ptr<IslandProgram>& ent);

    // stages and LDS
    struct Import { uint32_t hbm; int lastUse; uint32_t lds; };
    std::vector<Import> imports;            // imports needed in LDS: external producers (or host inputs) feeding chain members
    int importFor(uint32_t hbm);
    int base = 0, maxStage = 0;
    bool fuseCoef = false;                  // svf with its coefficient pre-pass inside the scan (scan_svf, island_ops.inc): no pre-pass task, no 6-slot scratch
    bool coefFused(uint16_t op) const { return fuseCoef && op == OP_SVF; }
    std::vector<int> slotFreeAt[2];         // per region: stage from which the slot is free again
    static constexpr uint32_t kLongBit = 1u << 31;
    uint32_t takeSlots(int stage, uint32_t count, int lastUse);
    uint32_t slotArea = 0, copies = 1, slotWords = 0;
    bool statelessIsland = true, mixerLike = false;
    bool assignStages();
    void allocateLds();

    // island-local program tables
    std::vector<Task> tasks;
    std::vector<int> taskWave;               // executing wave of tasks[i]
    std::vector<Member> members;
    std::vector<uint32_t> operands;
    std::vector<int> memberNode;             // NI index of members[i] (-1: an import copy)
    std::vector<int> operandSrc;             // operands[i]: NI index of the in-island producer, -2 - import index for an imported buffer, -1 otherwise
    std::vector<ConstCell> cells;            // broadcast cells for const-like producers
    std::unordered_map<uint32_t, uint32_t> cellOf;   // rec -> lds word
    std::vector<uint32_t> recTable;                  // local record index -> global record
    std::unordered_map<uint32_t, uint32_t> localRec;
    uint32_t cellFor(Node* c);
    uint32_t localOf(uint32_t rec);
    Member makeMember(NI& x);
    uint32_t waveLoad[kWaves] = {};          // estimated cycles per block
    uint32_t* loadOut = nullptr;
    int spareWaves = 0;
    void emitRanges(uint16_t op, int stage, uint32_t first, uint32_t count, const std::vector<int>& waves);
    uint32_t constMaskOf(const NI& x) const;
    bool phaseMergeable(const NI& x) const;
    void emitTasks();
    void emitStage(int stage);
    void balanceWaves();
    void orderTasks();

    // stage tables, specialised variant, blob
    uint32_t S = 0, schedRel = 0;
    std::vector<uint32_t> stageTab;
    SpecProgram sp;
    bool specIsland = false;
    void pipelineTables();
    void specVariant();
    void packBlob();
    std::shared_ptr<SpecText> specText();
    void recordProgram();
};

} // namespace elemhip
