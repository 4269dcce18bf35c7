// plan.cpp — render-sequence build: node table -> islands -> device task tables.
//
// Step 1 restates Runtime::buildRenderSequence / traverse (runtime/elem/Runtime.h:502-577):
// roots sorted active-first, DFS post-order per root, children in inlet order, `visited` shared
// across roots.  Any topological order yields identical samples (buffers are never aliased,
// GraphRenderSequence.h:121-124); the order still decides which root's sequence OWNS a shared
// node, and therefore which nodes stop rendering when an inactive root finishes its fade
// (GraphRenderSequence.h:212-219) and in which order tap buffers are promoted.
//
// Steps 2-5 are new: cluster each root sequence into islands (one workgroup, buffers in LDS),
// schedule each island's nodes into barrier-separated stages of wave tasks, allocate LDS slots
// by liveness, and order islands into launch levels. This file holds the graph-level passes (PlanBuilder::build names
// them in order), Engine::buildPlan and Engine::describePlan; plan_island.cpp holds the work on one island.
#include <algorithm>
#include <chrono>
#include <thread>
#include <cstdio>
#include <numeric>

#include <hip/hip_runtime.h>

#include "plan_build.h"

namespace elemhip {

namespace {

struct UF {
    std::vector<int> p;
    int find(int x) { while (p[x] != x) { p[x] = p[p[x]]; x = p[x]; } return x; }
    int add() { p.push_back((int)p.size()); return (int)p.size() - 1; }
};

} // namespace

PlanBuilder::PlanBuilder(Engine& eng, uint32_t packIslands) : e(eng), bs((uint32_t)eng.blockSize) {
    // a dry handle (no device) only generates / compiles kernels when asked to wait for them (cache warming, tests)
    wantSpec = e.specialize != 0 && (!e.dry || e.specialize >= 2);
    packK = packIslands; packMax = (uint32_t)std::max(1, e.packMax); cuCount = (uint32_t)std::max(1, e.cuCount); packRoots = e.packRoots;
}

void PlanBuilder::phase(const char* name) {
    const auto now = std::chrono::steady_clock::now();
    const double us = std::chrono::duration<double, std::micro>(now - tPhase).count();
    if (phaseNo < 4) p.buildUs[phaseNo++] = us;
    if (planTiming()) std::fprintf(stderr, "[elemhip] plan %-18s %7.3f ms\n", name, us * 1e-3);
    tPhase = now;
}

std::shared_ptr<Plan> PlanBuilder::build(uint32_t maxIslandNodes_, uint32_t maxCopies_) {
    maxIslandNodes = maxIslandNodes_; maxCopies = maxCopies_;
    tPhase = std::chrono::steady_clock::now();
    renderOrder();
    foldIntoConvolve();
    phase("render order");
    formIslands();
    if (!levelIslands()) return nullptr;
    packIslands();
    assignArena();
    phase("islands");
    pairTaps();
    // ---- 3/4. per-island schedule, LDS allocation, task emission -------------------------------------
    p.islands.resize(ib.size());
    p.islandProg.assign(ib.size(), nullptr);
    p.islandRoot.assign(ib.size(), 0);
    for (size_t ii = 0; ii < ib.size(); ++ii) if (!planIsland(ii)) return nullptr;
    if (!placePrograms()) return nullptr;
    if (p.heapOverflowDwords) return plan;
    phase("island programs");
    if (!levelTables()) return nullptr;
    phase("levels, roots");
    return plan;
}

void PlanBuilder::traverse(uint32_t epoch, std::vector<Node*>& order, Node* root) {
    // iterative DFS post-order, children in inlet order (Runtime.h:502-518); visited / on-stack are epoch marks in the nodes
    struct Frame { Node* n; size_t next; };
    if (root->planVisited == epoch) return;
    std::vector<Frame> st;
    st.push_back({root, 0});
    root->planOnStack = epoch;
    while (!st.empty()) {
        Frame& f = st.back();
        Node& n = *f.n;
        if (f.next < n.inlets.size()) {
            const Inlet& in = n.inlets[f.next++];
            Node* c = in.srcEpoch == e.nodesEpoch ? in.src : nullptr;
            if (!c) {                                    // (misses are not remembered: the node may be created later)
                auto it = e.nodes.find(in.source);
                if (it == e.nodes.end()) continue;
                c = &it->second; in.src = c; in.srcEpoch = e.nodesEpoch;
            }
            if (c->planVisited == epoch || c->planOnStack == epoch) continue;
            c->planOnStack = epoch;
            st.push_back({c, 0});
        } else {
            order.push_back(f.n);
            n.planVisited = epoch;
            n.planOnStack = 0;
            st.pop_back();
        }
    }
}

// ---- 1. render order ---------------------------------------------------------------------
void PlanBuilder::renderOrder() {
    std::vector<Node*> sortedRoots;   // std::list push_front/push_back in Runtime.h:544-559
    {
        std::vector<Node*> front, back;
        for (int32_t id : e.currentRoots) {
            auto it = e.nodes.find(id);
            if (it == e.nodes.end() || it->second.op != OP_ROOT) continue;
            auto a = it->second.props.find("active");
            const bool active = a != it->second.props.end() && a->second.isBool() && a->second.b;
            if (active) front.push_back(&it->second); else back.push_back(&it->second);
        }
        std::reverse(front.begin(), front.end());
        sortedRoots = front;
        sortedRoots.insert(sortedRoots.end(), back.begin(), back.end());
    }
    if (++e.planEpoch == 0u) { for (auto& kv : e.nodes) kv.second.planVisited = kv.second.planOnStack = 0u; e.planEpoch = 1u; }
    const uint32_t epoch = e.planEpoch;
    buildEpoch = epoch;
    idx.reserve(2 * e.nodes.size() + 64);   // (one entry per node and output channel; the table doubles that again)
    ni.reserve(e.nodes.size() + 16);
    std::vector<int32_t> planNodeIds;
    planNodeIds.reserve(e.nodes.size());
    for (size_t s = 0; s < sortedRoots.size(); ++s) {
        std::vector<Node*> order;
        traverse(epoch, order, sortedRoots[s]);
        seqRoots.push_back(sortedRoots[s]);
        seqNodes.emplace_back();
        for (Node* np : order) {
            Node& node = *np;
            const int32_t id = node.id;
            uint32_t numOuts = 1;                       // getRequiredOutputChannels (GraphRenderSequence.h:15-24)
            if (node.mc) for (auto& o : node.outlets) numOuts = std::max(numOuts, std::min<uint32_t>(o.channel + 1u, 16u));
            node.planIdx = (int32_t)ni.size(); node.planChans = numOuts;
            for (uint32_t ch = 0; ch < numOuts; ++ch) {
                NI x;
                x.n = &node;
                x.seq = (int)s;
                x.pos = (int)ni.size();
                x.kind = kindOf(node.op);
                x.ch = ch;
                if (ch == 0 || !node.mc) x.rec = node.rec;
                else { std::lock_guard<std::mutex> render(e.mu); x.rec = e.channelRec(node, ch); }   // (build runs without `mu`)
                idx[K(id, ch)] = (int)ni.size();
                seqNodes.back().push_back((int)ni.size());
                ni.push_back(x);
            }
            planNodeIds.push_back(id);
            if (node.op == OP_CAPTURE && node.mc) p.mcCaptureIds.push_back(id);
        }
    }
    // (no duplicates: the visit marks are shared by all root sequences, a node belongs to the first sequence that reaches it)
    p.nodeIds.swap(planNodeIds);
}

// ---- 1b. nodes folded into the convolve launch ------------------------------------------------------
// `root(convolve(in))` is the whole graph of a convolution reverb channel: three launch levels for one
// kernel's worth of work. An `in` leaf whose only in-plan consumers are convolvers is read by them straight
// from the host-input arena, and a root whose only input is a convolver owned by the same sequence (and
// consumed by nothing else) has its fade applied by that convolver, which writes the root's buffer.
void PlanBuilder::foldIntoConvolve() {
    for (NI& x : ni) {
        if (x.n->op != OP_IN || !x.n->inlets.empty()) continue;
        bool any = false, all = true;
        for (auto& o : x.n->outlets) {
            auto it = idx.find(K(o.dest));
            if (!it) continue;
            any = true;
            if (ni[it->second].n->op != OP_CONVOLVE) all = false;
        }
        if (any && all) { x.kind = K_CONST; x.elided = true; }
    }
    for (size_t sq = 0; sq < seqRoots.size(); ++sq) {
        Node* r = seqRoots[sq];
        if (r->inlets.size() != 1 || r->inlets[0].channel != 0) continue;
        auto it = idx.find(K(r->inlets[0].source));
        if (!it) continue;
        NI& c = ni[it->second];
        if (c.kind != K_CONV || c.seq != (int)sq) continue;
        size_t consumers = 0;
        for (auto& o : c.n->outlets) if (idx.count(K(o.dest))) ++consumers;
        if (consumers != 1) continue;
        NI& rn = ni[idx.at(K(r->id))];
        rn.kind = K_CONST; rn.elided = true;
        c.fusedRoot = idx.at(K(r->id));
    }
}

// ---- 2. islands ---------------------------------------------------------------------------------
// Union-find over the render order: a node joins the island(s) of its producers when that keeps the island graph acyclic
// and the island under `maxIslandNodes`; what comes out is the dense island list `ib`.
void PlanBuilder::formIslands() {
    UF uf;
    std::vector<uint32_t> weight;            // per island representative
    std::vector<std::vector<int>> succ;      // island DAG (by representative at insertion time; small unsorted sets)
    std::vector<int> ilevel;                 // running estimate of each island's launch level
    std::vector<uint32_t> seenMark;          // reaches(): visit marks by epoch (no hash set per query)
    uint32_t seenEpoch = 0;
    uf.p.reserve(ni.size()); weight.reserve(ni.size()); succ.reserve(ni.size()); ilevel.reserve(ni.size()); seenMark.reserve(ni.size());
    auto rep = [&](int i) { return uf.find(i); };
    auto newIsland = [&]() { int i = uf.add(); weight.push_back(0); succ.emplace_back(); ilevel.push_back(0); seenMark.push_back(0); return i; };
    using Small = std::vector<int>;          // a handful of island ids: linear search beats a tree
    auto has = [](const Small& v, int x) { return std::find(v.begin(), v.end(), x) != v.end(); };
    auto put = [&](Small& v, int x) { if (!has(v, x)) v.push_back(x); };
    auto putSucc = [&](int from, int to) { Small& v = succ[(size_t)from]; if (v.size() >= 64 || !has(v, to)) v.push_back(to); };   // (a duplicate edge is harmless; a fan-out of thousands stays linear)

    auto reaches = [&](const Small& from, const Small& targets, const Small& skip) {
        // is any island of `targets` reachable from `from` without starting inside `skip`?
        std::vector<int> stack;
        ++seenEpoch;
        auto first = [&](int r) { if (seenMark[(size_t)r] == seenEpoch) return false; seenMark[(size_t)r] = seenEpoch; return true; };
        for (int f : from) for (int s : succ[f]) { int r = rep(s); if (!has(skip, r) && first(r)) stack.push_back(r); }
        size_t budget = 20000;
        while (!stack.empty()) {
            if (budget-- == 0) return true;   // give up: treat as unsafe
            int x = stack.back(); stack.pop_back();
            if (has(targets, x)) return true;
            for (int s : succ[x]) { int r = rep(s); if (has(targets, r)) return true; if (first(r)) stack.push_back(r); }
        }
        return false;
    };

    Small deps, foreign, others;
    for (size_t k = 0; k < ni.size(); ++k) {
        NI& x = ni[k];
        if (x.kind == K_CONST) continue;
        const uint32_t w = 1 + scratchSlots(x.n->op);
        deps.clear(); foreign.clear();
        for (auto& in : x.n->inlets) {
            const int si = srcOf(in);
            if (si < 0) continue;
            NI& s = ni[si];
            if (s.kind == K_CONST) continue;
            if (s.seq != x.seq) { put(foreign, rep(s.island)); continue; }
            put(deps, rep(s.island));
        }
        std::sort(deps.begin(), deps.end()); std::sort(foreign.begin(), foreign.end());   // (the order a std::set walked them in)
        int target = -1;
        const bool sealed = x.kind == K_CONV || x.kind == K_HOST;
        if (!deps.empty() && !sealed) {
            uint32_t total = w;
            for (int d : deps) total += weight[d];
            const Small dv(deps);
            if (total <= maxIslandNodes && (deps.size() == 1 || !reaches(dv, deps, deps))) {
                // a foreign (other-sequence) producer must not be downstream of the merged set
                if (foreign.empty() || !reaches(dv, foreign, {})) {
                    target = dv[0];
                    for (size_t j = 1; j < dv.size(); ++j) {
                        int a = rep(target), b = rep(dv[j]);
                        if (a == b) continue;
                        uf.p[b] = a;
                        ilevel[a] = std::max(ilevel[a], ilevel[b]);
                        weight[a] += weight[b];
                        for (int sb : succ[b]) putSucc(a, sb);
                        target = a;
                    }
                    target = rep(target);
                }
            }
            if (target < 0) {
                // join the single producer island that none of the others is downstream of
                // (and only if that does not push the island to a later launch level: a mixer fed
                // by many peer islands gets its own island instead of stalling one of its peers)
                int best = -1;
                for (int d : dv) {
                    if (weight[d] + w > maxIslandNodes) continue;
                    bool raises = false;
                    for (int o : deps) if (o != d && ilevel[o] >= ilevel[d]) { raises = true; break; }
                    if (!raises) for (int o : foreign) if (ilevel[o] >= ilevel[d]) { raises = true; break; }
                    if (raises) continue;
                    others.clear();
                    for (int o : deps) if (o != d) others.push_back(o);
                    for (int f : foreign) put(others, f);
                    if (!others.empty() && reaches({d}, others, {})) continue;
                    if (best < 0 || weight[d] > weight[best]) best = d;
                }
                target = best;
            }
        }
        if (target < 0) {
            target = newIsland();
            for (int d : deps) ilevel[target] = std::max(ilevel[target], ilevel[rep(d)] + 1);
            for (int f : foreign) ilevel[target] = std::max(ilevel[target], ilevel[rep(f)] + 1);
        } else {
            for (int f : foreign) ilevel[target] = std::max(ilevel[target], ilevel[rep(f)] + 1);
        }
        x.island = target;
        weight[target] += w;
        if (sealed) weight[target] += maxIslandNodes;   // nothing joins a convolve island
        for (int d : deps) if (rep(d) != target) putSucc(rep(d), target);
        for (int f : foreign) if (rep(f) != target) putSucc(rep(f), target);
    }

    // canonical island list
    std::vector<int> islandOf(uf.p.size(), -1);   // uf representative -> dense index (in order of first appearance)
    for (size_t k = 0; k < ni.size(); ++k) {
        NI& x = ni[k];
        if (x.kind == K_CONST) continue;
        const int r = rep(x.island);
        if (islandOf[(size_t)r] < 0) { islandOf[(size_t)r] = (int)ib.size(); ib.emplace_back(); ib.back().seq = x.seq; }
        x.island = islandOf[(size_t)r];
        ib[x.island].nodes.push_back((int)k);
    }
}

// exports, in-island consumers, island deps; launch levels. false: the island graph is cyclic
bool PlanBuilder::levelIslands() {
    for (size_t k = 0; k < ni.size(); ++k) {
        NI& x = ni[k];
        if (x.kind == K_CONST) continue;
        if (x.n->op == OP_ROOT || x.kind == K_CONV || x.kind == K_HOST) x.exported = true;
        if (x.kind == K_CHAIN) x.needLds = true;
    }
    for (size_t k = 0; k < ni.size(); ++k) {
        NI& x = ni[k];
        if (x.kind == K_CONST) continue;
        for (auto& in : x.n->inlets) {
            const int si = srcOf(in);
            if (si < 0) continue;
            NI& s = ni[si];
            if (s.kind == K_CONST) continue;
            if (s.island == x.island) s.needLds = true;
            else {
                s.exported = true;
                auto& d = ib[x.island].deps;
                if (std::find(d.begin(), d.end(), s.island) == d.end()) d.push_back(s.island);
            }
        }
    }

    // launch levels (Kahn); a leftover island would mean a cycle slipped through clustering
    {
        std::vector<int> indeg(ib.size(), 0);
        std::vector<std::vector<int>> out(ib.size());
        for (size_t i = 0; i < ib.size(); ++i) for (int d : ib[i].deps) { out[d].push_back((int)i); indeg[i]++; }
        std::vector<int> q;
        for (size_t i = 0; i < ib.size(); ++i) if (!indeg[i]) q.push_back((int)i);
        size_t seen = 0;
        while (seen < q.size()) {
            int i = q[seen++];
            for (int o : out[i]) { ib[o].level = std::max(ib[o].level, ib[i].level + 1); if (--indeg[o] == 0) q.push_back(o); }
        }
        if (seen != ib.size()) { std::fprintf(stderr, "[elemhip] plan: island graph is cyclic\n"); return false; }
    }
    return true;
}

// ---- 2b. lane-packing of isomorphic islands -----------------------------------------------------------------------
// A stateful island is one workgroup, and its float recurrences run one NODE PER LANE: a voice's envelope pole keeps a
// whole wavefront busy with one lane. When a launch level has more such islands than the chip has CUs (512 voices, 1024
// render jobs) the islands of one shape are merged K at a time: the recurrence tasks of the merged island carry K lanes at
// the price of one (same-opcode chain members of a stage share a task anyway), only the sample-parallel work grows K-fold.
// Islands of one launch level never depend on each other, so any such merge keeps the island graph acyclic. Only islands
// of ONE root sequence are merged: an island renders while its root runs (GraphRenderSequence.h:214-219), and two roots
// may stop at different blocks — independent render jobs with a root each (C4) stay one per workgroup.
void PlanBuilder::packIslands() {
    packedIslands = 0;
    packCount.assign(ib.size(), 1u);                       // original islands inside each island
    {   // how many stateful islands does the fullest launch level hold?  packK = 0: as many per island as it takes to fit the CUs
        std::map<int, uint32_t> perLevel;
        for (size_t i = 0; i < ib.size(); ++i) {
            bool stateful = false;
            for (int k : ib[i].nodes) if (ni[k].kind != K_PAR || ni[k].n->op == OP_TAPIN || ni[k].n->op == OP_TAPOUT) stateful = true;
            if (stateful) perLevel[ib[i].level]++;
        }
        statefulIslandsMax = 0;
        for (auto& kv : perLevel) statefulIslandsMax = std::max(statefulIslandsMax, kv.second);
        if (packK == 0) packK = std::max(1u, std::min(packMax, (statefulIslandsMax + cuCount - 1u) / std::max(1u, cuCount)));
    }
    if (packK > 1) {
        struct Key { int level, seq; uint64_t shape; bool operator<(const Key& o) const { return level != o.level ? level < o.level : seq != o.seq ? seq < o.seq : shape < o.shape; } };
        std::map<Key, std::vector<int>> groups;
        // `pack_roots` (opt-in): islands of DIFFERENT root sequences may share a workgroup when every one of those roots is active
        // at plan time — an active root keeps running until the next commit (a change of root targets always arrives with one), so
        // "renders while ITS root runs" (GraphRenderSequence.h:214-219) is the same fact for all members. The other half of that
        // test, root channel < the caller's output count, is a per-call fact: the engine refuses a call that asks for fewer outputs
        // than the packed roots' channels need (Plan::packedRootChannels).
        std::vector<char> seqActive(seqRoots.size(), 0);
        for (size_t sq = 0; sq < seqRoots.size(); ++sq) {
            auto a = seqRoots[sq]->props.find("active");
            seqActive[sq] = (a != seqRoots[sq]->props.end() && a->second.isBool() && a->second.b && seqRoots[sq]->channel >= 0) ? 1 : 0;
        }
        for (size_t i = 0; i < ib.size(); ++i) {
            bool stateful = false, sealed = false;
            uint64_t h = 1469598103934665603ull;
            for (int k : ib[i].nodes) {
                const NI& x = ni[k];
                if (x.kind == K_CONV || x.kind == K_HOST) sealed = true;
                if (x.kind != K_PAR || x.n->op == OP_TAPIN || x.n->op == OP_TAPOUT) stateful = true;
                h ^= (uint64_t)x.n->op | ((uint64_t)x.n->inlets.size() << 16); h *= 1099511628211ull;
            }
            if (sealed || !stateful) continue;
            groups[Key{ib[i].level, (packRoots && seqActive[(size_t)ib[i].seq]) ? -1 : ib[i].seq, h}].push_back((int)i);
        }
        std::vector<int> mergedInto(ib.size(), -1);
        for (auto& kv : groups) {
            std::vector<int>& g = kv.second;
            for (size_t q = 0; q + 1 < g.size(); q += packK) {
                const int head = g[q];
                for (size_t j = q + 1; j < std::min(g.size(), q + (size_t)packK); ++j) {
                    const int from = g[j];
                    ib[head].nodes.insert(ib[head].nodes.end(), ib[from].nodes.begin(), ib[from].nodes.end());
                    for (int d : ib[from].deps) if (std::find(ib[head].deps.begin(), ib[head].deps.end(), d) == ib[head].deps.end()) ib[head].deps.push_back(d);
                    ib[from].nodes.clear(); ib[from].deps.clear();
                    mergedInto[from] = head;
                    packCount[head] += 1u;
                    ++packedIslands;
                    if (ib[from].seq != ib[head].seq)
                        p.packedRootChannels = std::max(p.packedRootChannels, 1 + std::max(seqRoots[(size_t)ib[from].seq]->channel, seqRoots[(size_t)ib[head].seq]->channel));
                }
                std::sort(ib[head].nodes.begin(), ib[head].nodes.end());          // NI indices are render-order positions
            }
        }
        if (packedIslands) {   // compact the island list, renumber
            std::vector<int> newIdx(ib.size(), -1);
            std::vector<IslandBuild> nb;
            std::vector<uint32_t> pc;
            for (size_t i = 0; i < ib.size(); ++i) if (mergedInto[i] < 0) { newIdx[i] = (int)nb.size(); nb.push_back(std::move(ib[i])); pc.push_back(packCount[i]); }
            packCount.swap(pc);
            for (size_t i = 0; i < newIdx.size(); ++i) if (mergedInto[i] >= 0) newIdx[i] = newIdx[mergedInto[i]];
            for (IslandBuild& B : nb) {
                for (int& d : B.deps) d = newIdx[d];
                std::sort(B.deps.begin(), B.deps.end());
                B.deps.erase(std::unique(B.deps.begin(), B.deps.end()), B.deps.end());
            }
            for (NI& x : ni) if (x.kind != K_CONST && x.island >= 0) x.island = newIdx[x.island];
            ib.swap(nb);
        }
    }
}

// HBM arena indices: level-major so one level's exports are contiguous
void PlanBuilder::assignArena() {
    numLevels = 0;
    for (auto& i : ib) numLevels = std::max(numLevels, i.level + 1);
    {
        std::vector<int> order(ib.size());
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ib[a].level < ib[b].level; });
        uint32_t next = kMaxHostIn;
        for (int i : order) for (int k : ib[i].nodes) if (ni[k].exported) ni[k].hbm = next++;
        for (NI& x : ni) if (x.elided && x.n->op == OP_ROOT) x.hbm = next++;   // written by the root's convolver
        p.numHbmBuffers = next;
    }
}

// ---- taps inside launch sets (Feedback.h:90-126, GraphRenderSequence.h:297-308) --------------------
// A tapIn of block b+1 reads what the tapOut of its name received in block b (the end-of-block promotion). A launch
// set renders its blocks level by level, so that hand-over can only happen inside ONE island: the island keeps a single
// block in flight (copies = 1: block b+1 starts when block b has left it), the tapOut sits at least one stage behind its
// tapIns, and a tapIn reads the tapOut's private buffer for every block but the set's first (run_tapin); the batch
// epilogue promotes once, after the set. Anything else — a name written by two tapOuts, or read in another island
// than the one that writes it — keeps the plan on the block-at-a-time path (Engine::batchEligible).
void PlanBuilder::pairTaps() {
    tapWriter.assign(ni.size(), -1);
    islandPairsTaps.assign(ib.size(), 0);
    p.tapsInSets = true;
    p.tapPairs.clear();
    {
        std::map<const void*, std::vector<int>> outs, ins;
        for (size_t k = 0; k < ni.size(); ++k) {
            if (ni[k].island < 0 || !ni[k].n->res) continue;
            if (ni[k].n->op == OP_TAPOUT) outs[ni[k].n->res.get()].push_back((int)k);
            if (ni[k].n->op == OP_TAPIN) ins[ni[k].n->res.get()].push_back((int)k);
        }
        for (auto& kv : outs) {
            std::vector<int> uniq;                   // (a tapOut shared by two roots appears once per NI entry of its id)
            for (int k : kv.second) { bool seen = false; for (int u : uniq) seen = seen || ni[u].n == ni[k].n; if (!seen) uniq.push_back(k); }
            if (uniq.size() > 1) { p.tapsInSets = false; continue; }
            auto it = ins.find(kv.first);
            if (it == ins.end()) continue;
            for (int k : it->second) {
                if (ni[k].island != ni[uniq[0]].island) { p.tapsInSets = false; continue; }
                tapWriter[(size_t)k] = uniq[0];
                islandPairsTaps[(size_t)ni[k].island] = 1;
                ni[(size_t)uniq[0]].needLds = true;   // the hand-over goes through the tapOut's LDS slot (below)
            }
        }
        for (size_t k = 0; k < ni.size(); ++k)
            if (ni[k].island >= 0 && ni[k].n->op == OP_TAPIN) p.tapPairs.push_back({ni[k].n->id, p.tapsInSets && tapWriter[k] >= 0 ? ni[(size_t)tapWriter[k]].n->id : 0});
    }
}

// the scheduled islands' programs go to the heap as one contiguous upload; everything else is there already.
// false: the upload failed. Plan::heapOverflowDwords set: the heap lacks room (Engine::buildPlan starts a bigger one)
bool PlanBuilder::placePrograms() {
    ProgHeap& H = *e.progHeap;
    const size_t need = p.prog.size();
    if (H.usedDwords + need > H.capDwords) { p.heapOverflowDwords = std::max<size_t>(need, 1); return true; }
    const uint32_t base = (uint32_t)H.usedDwords;
    H.usedDwords += need;
    for (uint32_t ii : scheduled) {
        p.islands[ii].progBegin += base;
        p.islandProg[ii]->heap = e.progHeap; p.islandProg[ii]->heapBegin = p.islands[ii].progBegin;
    }
    if (H.dev && need && hipMemcpy(H.dev + base, p.prog.data(), need * 4, hipMemcpyHostToDevice) != hipSuccess) return false;
    p.progHeap = e.progHeap;
    p.prog.clear(); p.prog.shrink_to_fit();
    return true;
}

// ---- 5. launch levels, roots, taps ------------------------------------------------------------------
bool PlanBuilder::levelTables() {
    p.islandLevel.resize(ib.size());
    for (size_t i = 0; i < ib.size(); ++i) p.islandLevel[i] = (uint32_t)ib[i].level;
    p.levelOffsets.assign((size_t)numLevels + 1, 0);
    p.levelLdsBytes.assign((size_t)numLevels, 0);
    for (size_t i = 0; i < ib.size(); ++i) p.levelOffsets[(size_t)ib[i].level + 1] += p.islands[i].split;
    for (int l = 0; l < numLevels; ++l) p.levelOffsets[(size_t)l + 1] += p.levelOffsets[l];
    p.levelIslands.resize(p.levelOffsets.back());
    {
        std::vector<uint32_t> cursor(p.levelOffsets.begin(), p.levelOffsets.end() - 1);
        for (size_t i = 0; i < ib.size(); ++i) {
            for (uint32_t k = 0; k < p.islands[i].split; ++k) p.levelIslands[cursor[ib[i].level]++] = (uint32_t)i | (k << 24);
            p.levelLdsBytes[ib[i].level] = std::max(p.levelLdsBytes[ib[i].level], p.islands[i].ldsWords * 4u);
        }
    }
    if (p.convs.size() > 0xFFFFu) { std::fprintf(stderr, "[elemhip] plan: too many convolve nodes\n"); return false; }
    p.convLevelOffsets.assign((size_t)numLevels + 1, 0);
    for (int l = 0; l < numLevels; ++l) {    // per level: every node's main workgroup first, then the helpers
        for (size_t c = 0; c < p.convs.size(); ++c) if (convLevel[c] == l) p.convWork.push_back((uint32_t)c);
        for (size_t c = 0; c < p.convs.size(); ++c) if (convLevel[c] == l)
            for (uint32_t h = 0; h < conv::kBinGroups * p.convs[c].slices; ++h) p.convWork.push_back((uint32_t)c | ((h + 1u) << 16));
        p.convLevelOffsets[(size_t)l + 1] = (uint32_t)p.convWork.size();
    }
    for (size_t s = 0; s < seqRoots.size(); ++s) {
        Node* r = seqRoots[s];
        NI& x = ni[idx.at(K(r->id))];
        p.roots.push_back(RootEntry{r->rec, x.hbm});
        p.rootIds.push_back(r->id);
        for (int k : seqNodes[s]) if (ni[k].n->op == OP_TAPOUT) p.taps.push_back(TapEntry{ni[k].n->rec, r->rec});
        for (int k : seqNodes[s]) if (ni[k].n->op == OP_METER || ni[k].n->op == OP_SNAPSHOT || ni[k].n->op == OP_SCOPE || ni[k].n->op == OP_CAPTURE || ni[k].n->op == OP_FFT) p.eventNodes.push_back({ni[k].n->id, r->id});
    }
    return true;
}

static size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// ---- specialised kernels: group each level's islands by generated text, queue the shapes for compilation ----
// Returns the time spent waiting for the compiler in ms (`specialize` = 2), -1 when nothing was waited for.
double PlanBuilder::groupShapes(Engine& e, Plan& p) {
    double jitWaitMs = -1.0;
    // Call-out nodes synchronise with the host inside a block: their plans render block at a time through the interpreter kernels.
    // (Plans with tap nodes keep their specialised kernels: a paired tapIn takes its block from the tapOut's LDS slot, an unpaired
    // one from the shared buffer the per-block promotion fills — neither needs anything the specialised kernels lack.)
    if (!p.hosts.empty()) p.specText.clear();
    const size_t L = p.levelOffsets.size() - 1;
    p.restOffsets.assign(L + 1, 0);
    p.restRoots.assign(L, {});
    std::vector<uint8_t> covered(p.islands.size(), 0);
    for (size_t l = 0; l < L; ++l) {
        // one shape per kernel: islands are grouped by the cache key of their text (two cached text objects can carry the same
        // text — the text cache is keyed by a signature that also covers what the text leaves out); a split island appears
        // once per part in levelIslands and once here
        std::map<std::string, std::pair<SpecText*, std::vector<uint32_t>>> byText;
        std::vector<uint8_t> seen(p.islands.size(), 0);
        for (uint32_t q = p.levelOffsets[l]; q < p.levelOffsets[l + 1]; ++q) {
            const uint32_t isl = p.levelIslands[q] & 0xFFFFFFu;
            if (!(isl < p.specText.size() && p.specText[isl]) || covered[isl] || seen[isl]) continue;
            seen[isl] = 1;
            SpecText& tx = *p.specText[isl];
            const uint32_t ldsW = p.islands[isl].ldsWords;
            if (tx.key.empty() || tx.keyLdsWords != ldsW) { tx.key = Jit::get().keyFor(tx.text, ldsW, (uint32_t)e.blockSize); tx.keyLdsWords = ldsW; }
            auto& slot = byText[tx.key];
            slot.first = &tx; slot.second.push_back(isl);
        }
        // the level's shapes, the ones with the most islands first (ties: by key): a level renders at most `max_shape_launches`
        // specialised launches, the biggest shapes — everything behind them in this list is ONE contiguous run the interpreter
        // kernel takes in one launch (Engine::launchLevelBatch). A live graph of structurally different voices used to give every
        // voice whose kernel had been compiled a launch (and a side stream) of its own: 60 launches per level and set, 150 us per block.
        std::vector<std::pair<const std::string*, std::pair<SpecText*, std::vector<uint32_t>>*>> order;
        for (auto& kvk : byText) order.emplace_back(&kvk.first, &kvk.second);
        std::stable_sort(order.begin(), order.end(), [](const auto& a, const auto& b) { return a.second->second.size() > b.second->second.size(); });
        for (auto& ord : order) {
            auto& kv = *ord.second;
            // background mode: a shape only one island has (a voice that is fading out next to its replacement, a
            // one-off graph) is not worth a compile at commit time: its plan may be gone in 30 ms. It gets a DEFERRED entry —
            // known to the kernel cache, not queued — and renders through the interpreter kernel; once this plan has rendered
            // for a while (Engine::promoteDeferredShapes: `spec_lonely_blocks` blocks and `spec_lonely_ms` of wall clock) the
            // shape is queued behind everything else, so a static single-patch graph leaves the interpreter too (r04: never)
            const uint32_t ldsW = p.islands[kv.second[0]].ldsWords;
            SpecText& tx = *kv.first;
            // ... and at once when it keeps coming back: a live graph that replaces a voice per commit meets the same one-off shape
            // (the old voice fading out behind its own mixer and root) in every plan — the second plan that wants it has it compiled
            const bool lonely = e.specialize == 1 && kv.second.size() < 2;
            const bool defer = lonely && !Jit::get().knownKey(tx.key) && Jit::get().sighting(tx.key) < 2u;
            Plan::SpecShape sh;
            sh.optional = lonely;
            sh.deferred = defer;
            sh.entry = Jit::get().requestKey(tx.key, tx.text, ldsW, (uint32_t)e.blockSize, defer);
            if (!e.dry) sh.entry->wantOn(e.device);
            if (defer) p.deferredShapes++;
            sh.level = (uint32_t)l; sh.listBegin = (uint32_t)p.specLists.size();
            sh.stateless = p.islands[kv.second[0]].stateless != 0u;
            // (levelIslands entry format: island | split part << 24 — a split island is one workgroup per part)
            for (uint32_t isl : kv.second) {
                for (uint32_t k = 0; k < std::max(1u, p.islands[isl].split); ++k) p.specLists.push_back(isl | (k << 24));
                covered[isl] = 1;
                if (std::find(sh.roots.begin(), sh.roots.end(), p.islandRoot[isl]) == sh.roots.end()) sh.roots.push_back(p.islandRoot[isl]);
            }
            sh.count = (uint32_t)p.specLists.size() - sh.listBegin;
            p.shapes.push_back(std::move(sh));
        }
        for (uint32_t q = p.levelOffsets[l]; q < p.levelOffsets[l + 1]; ++q) {
            const uint32_t isl = p.levelIslands[q] & 0xFFFFFFu;
            if (covered[isl]) continue;
            p.restIslands.push_back(p.levelIslands[q]);
            auto& rr = p.restRoots[l];
            if (std::find(rr.begin(), rr.end(), p.islandRoot[isl]) == rr.end()) rr.push_back(p.islandRoot[isl]);
        }
        p.restOffsets[l + 1] = (uint32_t)p.restIslands.size();
    }
    p.specText.clear(); p.specText.shrink_to_fit();
    if (e.specialize >= 2) {
        const auto t0 = std::chrono::steady_clock::now();
        for (auto& sh : p.shapes) (void)Jit::get().wait(sh.entry);
        jitWaitMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return jitWaitMs;
}

// the plan's device tables in one host buffer, every table 16-byte aligned
PlanBuilder::Tables PlanBuilder::packTables(const Plan& p) {
    Tables t;
    size_t off = 0;
    auto place = [&](size_t bytes) { size_t o = off; off = align16(off + bytes); return o; };
    t.islands = place(p.islands.size() * sizeof(Island));
    t.level = place(p.levelIslands.size() * 4);
    t.roots = place(p.roots.size() * sizeof(RootEntry));
    t.taps = place(p.taps.size() * sizeof(TapEntry));
    t.convs = place(p.convs.size() * sizeof(ConvDesc));
    t.convWork = place(p.convWork.size() * 4);
    t.specLists = place(p.specLists.size() * 4);
    t.rest = place(p.restIslands.size() * 4);
    t.host.assign(std::max<size_t>(off, 16), 0);
    auto put = [&](size_t o, const void* src, size_t bytes) { if (bytes) std::memcpy(t.host.data() + o, src, bytes); };
    put(t.islands, p.islands.data(), p.islands.size() * sizeof(Island));
    put(t.level, p.levelIslands.data(), p.levelIslands.size() * 4);
    put(t.roots, p.roots.data(), p.roots.size() * sizeof(RootEntry));
    put(t.taps, p.taps.data(), p.taps.size() * sizeof(TapEntry));
    put(t.convs, p.convs.data(), p.convs.size() * sizeof(ConvDesc));
    put(t.convWork, p.convWork.data(), p.convWork.size() * 4);
    put(t.specLists, p.specLists.data(), p.specLists.size() * 4);
    put(t.rest, p.restIslands.data(), p.restIslands.size() * 4);
    return t;
}

std::shared_ptr<Plan> Engine::buildPlan(std::unique_lock<std::mutex>& renderLock) {
    // Planning reads the node table (structure owned by `ctl`, which the caller holds) and writes only the new Plan:
    // it runs WITHOUT the render lock, so process* calls keep rendering the current plan while a commit is planned.
    struct Relock {
        std::unique_lock<std::mutex>& l;
        explicit Relock(std::unique_lock<std::mutex>& l_) : l(l_) { l.unlock(); }
        ~Relock() { if (!l.owns_lock()) l.lock(); }
    } relock(renderLock);
    if (debugBuildDelayMs > 0) std::this_thread::sleep_for(std::chrono::milliseconds(debugBuildDelayMs));
    std::shared_ptr<Plan> plan;
    const uint32_t ldsLimit = 160u * 1024u - 1024u;
    // the text cache is only ever trimmed BETWEEN builds (texts in use stay alive through the shared objects the plan holds)
    if (specTextCache.size() > 4096) specTextCache.clear();
    if (islandCache.size() > 2048) islandCache.clear();      // (entries of replaced islands are never looked up again: ~8 KB each)
    if (islandShapeCache.size() > 512) islandShapeCache.clear();
    // Lane-packing (option "pack_islands": 0 auto, 1 off, K): the first attempt packs as the option says; a packed island
    // that does not fit in LDS, or fits with a single buffer set (no blocks in flight: the stages of a block would run back
    // to back), sends the build back with one island fewer per pack.
    // room in the program heap for this build's new programs: a few islands on a live graph, all of them on a first build
    auto freshHeap = [&](size_t needDwords) -> bool {
        auto h = std::make_shared<ProgHeap>();
        h->capDwords = std::max<size_t>((size_t)4 << 20, 8 * needDwords);       // 16 MB, or eight builds' worth
        if (progHeapCap) h->capDwords = std::max(progHeapCap, needDwords);       // option "prog_heap_dwords" (tests: a heap that keeps running out)
        else if (dry) h->capDwords = (size_t)1 << 30;
        if (dry) {}
        else if (hipMalloc(reinterpret_cast<void**>(&h->dev), h->capDwords * 4) != hipSuccess) return false;
        islandCache.clear();                   // (its entries name offsets of the old heap; plans in flight keep that heap alive)
        progHeap = std::move(h);
        st.progHeaps++;
        return true;
    };
    if (!progHeap || progHeap->capDwords - progHeap->usedDwords < (progHeapCap ? 0 : std::max<size_t>((size_t)1 << 18, 2 * lastPlanProgDwords)))
        if (!freshHeap(lastPlanProgDwords)) return nullptr;
    uint32_t packK = (uint32_t)packIslands;
    for (;;) {
        uint32_t usedK = 1, minCopies = 0;
        for (uint32_t limit = 56; limit >= 4; limit /= 2) {
            PlanBuilder b(*this, packK);
            plan = b.build(limit, (uint32_t)std::max(1, pipelineCopies));
            if (plan && plan->heapOverflowDwords) {        // a graph far bigger than the last one: a heap sized for it, same attempt again
                if (!freshHeap(plan->heapOverflowDwords)) return nullptr;
                PlanBuilder b2(*this, packK);
                plan = b2.build(limit, (uint32_t)std::max(1, pipelineCopies));
                if (plan && plan->heapOverflowDwords) plan.reset();
                if (!plan) return nullptr;
                b.packK = b2.packK; b.minPackedCopies = b2.minPackedCopies; b.packedIslands = b2.packedIslands;
            }
            if (!plan) return nullptr;
            usedK = b.packK; minCopies = b.minPackedCopies;
            plan->packK = b.packedIslands ? usedK : 1u;
            if (plan->maxLdsBytes <= ldsLimit) break;
            plan.reset();
            if (usedK > 1) break;          // (a packed island too big for LDS: pack fewer rather than cut the islands up)
        }
        if (usedK > 1 && (!plan || (minCopies != 0 && minCopies < 2 && pipelineCopies >= 2))) { plan.reset(); packK = usedK - 1; continue; }
        break;
    }
    if (!plan) { std::fprintf(stderr, "[elemhip] plan: could not fit islands into LDS\n"); return nullptr; }
    Plan& p = *plan;
    lastPlanProgDwords = p.progDwordsTotal;


    // group the shapes, pack + upload the tables
    const auto tTables = std::chrono::steady_clock::now();
    const double jitWaitMs = PlanBuilder::groupShapes(*this, p);
    const PlanBuilder::Tables t = PlanBuilder::packTables(p);
    const std::vector<uint8_t>& host = t.host;

    const auto tUpload = std::chrono::steady_clock::now();
    p.buildUs[4] = std::chrono::duration<double, std::micro>(tUpload - tTables).count();
    // The tables go to the device BEFORE the render lock is taken again (r06): nothing a render call touches is involved — the pool
    // has a lock of its own, the copy runs on the null stream, the new plan is not visible to anybody yet — so what a commit still
    // does under `mu` behind a plan build is a handful of stores (the upload was 10 of the ~12 us it held).
    if (!dry) {
        p.pool = tablePool;
        p.dev = tablePool->take(host.size());
        if (!p.dev.ptr) return nullptr;
        if (hipMemcpy(p.dev.ptr, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        const uint8_t* d = static_cast<const uint8_t*>(p.dev.ptr);
        p.view.islands = reinterpret_cast<const Island*>(d + t.islands);
        p.view.levelIslands = reinterpret_cast<const uint32_t*>(d + t.level);
        p.view.prog = p.progHeap->dev;          // island programs live in the engine's program heap (Island::progBegin is relative to it)
        p.view.roots = reinterpret_cast<const RootEntry*>(d + t.roots);
        p.view.taps = reinterpret_cast<const TapEntry*>(d + t.taps);
        p.view.convs = reinterpret_cast<const ConvDesc*>(d + t.convs);
        p.view.convWork = reinterpret_cast<const uint32_t*>(d + t.convWork);
        p.dSpecLists = reinterpret_cast<const uint32_t*>(d + t.specLists);
        p.dRestIslands = reinterpret_cast<const uint32_t*>(d + t.rest);
        p.view.numConvs = (uint32_t)p.convs.size();
        p.view.numRoots = (uint32_t)p.roots.size();
        p.view.numTaps = (uint32_t)p.taps.size();
    }
    p.buildUs[5] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tUpload).count();
    renderLock.lock();   // ---- from here on: render-side state ----
    residentStop();
    st.specShapes = (uint32_t)p.shapes.size(); st.specIslands = (uint32_t)p.specLists.size();
    if (jitWaitMs >= 0.0) st.lastJitWaitMs = jitWaitMs;
    // root records learn whether fade.process() runs on them (Core.h:74-77)
    for (int32_t id : p.rootIds) {
        Node& r = nodes.at(id);
        const uint32_t has = r.inlets.empty() ? 0u : 1u;
        if (shadow[r.rec * kRecDwords + rec::ROOT_HASIN] != has) writeParam(r, rec::ROOT_HASIN, has);
    }
    return plan;
}

} // namespace elemhip

namespace elemhip {

// 64-bit FNV-1a over what the planner produced: island headers and program blobs, the level / convolve / call-out / root / tap
// tables and the text of every specialised shape (tests/plan_corpus.py pins it). Left out: Island::progBegin (a heap offset,
// differs between cache modes) and everything that is a fact of the process rather than of the plan (kernel-cache keys fold in
// the compiler version; the order of equally big shapes of a level follows those keys, so shapes are folded in sorted by hash).
static uint64_t programDigest(const Plan& p) {
    const uint64_t kBasis = 1469598103934665603ull, kPrime = 1099511628211ull;
    uint64_t h = kBasis;
    auto bytes = [&](const void* d, size_t n) { const uint8_t* b = static_cast<const uint8_t*>(d); for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= kPrime; } };
    auto u32 = [&](uint32_t v) { bytes(&v, 4); };
    auto vec = [&](const auto& v) { u32((uint32_t)v.size()); if (!v.empty()) bytes(v.data(), v.size() * sizeof(v[0])); };
    u32((uint32_t)p.islands.size());
    for (size_t i = 0; i < p.islands.size(); ++i) {
        Island I = p.islands[i];
        I.progBegin = 0u;
        bytes(&I, sizeof I);
        if (i < p.islandProg.size() && p.islandProg[i]) vec(p.islandProg[i]->blob); else u32(kNone);
    }
    vec(p.levelIslands); vec(p.levelOffsets); vec(p.convs); vec(p.convWork); vec(p.convLevelOffsets); vec(p.roots); vec(p.taps);
    u32((uint32_t)p.tapPairs.size());
    for (auto& tp : p.tapPairs) { u32((uint32_t)tp.first); u32((uint32_t)tp.second); }
    vec(p.restIslands); vec(p.restOffsets);
    u32((uint32_t)p.hosts.size());
    for (const Plan::HostDesc& d : p.hosts) {
        u32((uint32_t)d.nodeId); u32((uint32_t)d.rootId); u32(d.outHbm); u32(d.level); u32(d.active); u32(d.leaf); u32((uint32_t)d.inputs.size());
        for (auto& in : d.inputs) { u32((uint32_t)in.kind); u32(in.idx); bytes(&in.value, 4); }
    }
    u32(p.numHbmBuffers); u32(p.numStreamBuffers); u32(p.packK);
    std::vector<uint64_t> shapes;       // per specialised shape: its level, kind, kernel text and workgroup list
    for (const Plan::SpecShape& sh : p.shapes) {
        const uint64_t outer = h;
        h = kBasis;
        u32(sh.level); u32(sh.stateless); u32(sh.count);
        bytes(sh.entry->generated.data(), sh.entry->generated.size());
        for (uint32_t k = 0; k < sh.count; ++k) u32(p.specLists[sh.listBegin + k]);
        shapes.push_back(h);
        h = outer;
    }
    std::sort(shapes.begin(), shapes.end());
    vec(shapes);
    return h;
}

// JSON description of the render plan (islands, levels, tasks) for host-logic tests and debugging.
std::string Engine::describePlan() {
    std::lock_guard<std::mutex> lock(mu);
    // the newest plan (pending if a commit has not been rendered yet); nothing is adopted here
    const std::shared_ptr<Plan> shown = pending ? pending : current;
    if (!shown) return "null";
    const Plan& p = *shown;
    std::string s = "{";
    auto kv = [&](const char* k, uint64_t v, bool comma = true) { s += "\"" + std::string(k) + "\":" + std::to_string(v) + (comma ? "," : ""); };
    kv("num_islands", p.islands.size()); kv("num_levels", p.levelOffsets.size() - 1); kv("num_tasks", p.numTasks);
    kv("num_members", p.numMembers); kv("num_operands", p.numOperands); kv("num_nodes", p.nodeIds.size());
    kv("plan_islands_relocated", st.planIslandsRelocated); kv("plan_relocation_mismatches", st.planRelocationMismatches);
    kv("plan_spec_texts", specTextCache.size()); kv("plan_spec_fade_blocks", st.specFadeBlocks); kv("plan_idle_launches_skipped", st.idleLaunchesSkipped); kv("plan_prog_heaps", st.progHeaps); kv("plan_prog_heap_used_dwords", p.progHeap ? p.progHeap->usedDwords : 0);
    kv("plan_islands_reused", st.planIslandsReused); kv("plan_islands_scheduled", st.planIslandsScheduled); kv("plan_cache_mismatches", st.planCacheMismatches);
    kv("num_hbm_buffers", p.numHbmBuffers); kv("num_stream_buffers", p.numStreamBuffers); kv("pack_k", p.packK);
    kv("max_lds_bytes", p.maxLdsBytes); kv("num_roots", p.roots.size());
    { char b[48]; std::snprintf(b, sizeof b, "\"program_digest\":\"%016llx\",", (unsigned long long)programDigest(p)); s += b; }
    s += "\"build_us\":{";
    {
        static const char* names[6] = {"render_order", "islands", "island_programs", "levels_roots", "shapes_tables", "upload"};
        for (int k = 0; k < 6; ++k) { char b[64]; std::snprintf(b, sizeof b, "%s\"%s\":%.1f", k ? "," : "", names[k], p.buildUs[k]); s += b; }
    }
    s += "},";
    {   // which kernels rendered (island x block units since the handle was made), this plan's shapes, the process-wide kernel cache
        const JitStats js = Jit::get().stats();
        const uint64_t tot = islandBlocksSpec + islandBlocksInterp;
        char b[1024];
        uint32_t ready = 0, waiting = 0, deferred = 0;
        for (const Plan::SpecShape& sh : p.shapes) { const int stt = sh.entry->state.load(); if (stt == 1) ++ready; else if (stt == 2) ++deferred; else if (stt == 0) ++waiting; }
        std::snprintf(b, sizeof b, "\"island_blocks_spec\":%llu,\"island_blocks_interp\":%llu,\"interp_block_fraction\":%.6f,"
                      "\"shapes\":{\"total\":%zu,\"ready\":%u,\"compiling\":%u,\"deferred\":%u},"
                      "\"jit\":{\"entries\":%llu,\"entry_cap\":%u,\"modules_loaded\":%llu,\"compiles\":%llu,\"disk_hits\":%llu,\"failed\":%llu,\"evictions\":%llu,"
                      "\"abandoned\":%llu,\"queued\":%llu,\"deferred\":%llu,\"promoted\":%llu,\"compile_ms_mean\":%.1f,\"compile_ms_max\":%.1f,\"compile_ms_last\":%.1f,"
                      "\"text_bytes_held\":%llu,\"code_bytes_held\":%llu,\"disk_bytes\":%llu,\"disk_cap_bytes\":%llu,\"disk_files_removed\":%llu,\"workers\":%u},",
                      (unsigned long long)islandBlocksSpec, (unsigned long long)islandBlocksInterp, tot ? (double)islandBlocksInterp / (double)tot : 0.0,
                      p.shapes.size(), ready, waiting, deferred,
                      (unsigned long long)js.entries, js.entryCap, (unsigned long long)js.modulesLoaded, (unsigned long long)js.compiles, (unsigned long long)js.diskHits,
                      (unsigned long long)js.failed, (unsigned long long)js.evictions, (unsigned long long)js.abandoned, (unsigned long long)js.queued,
                      (unsigned long long)js.deferred, (unsigned long long)js.promoted, js.compiles ? js.compileMsTotal / (double)js.compiles : 0.0, js.compileMsMax, js.compileMsLast,
                      (unsigned long long)js.sourceBytesHeld, (unsigned long long)js.codeBytesHeld, (unsigned long long)js.diskBytes, (unsigned long long)js.diskCapBytes,
                      (unsigned long long)js.diskFilesRemoved, js.workers);
        s += b;
    }
    kv("sync_poll", syncPoll ? 1 : 0); kv("sync_polls", syncPolls); kv("sync_poll_fallbacks", syncPollFallbacks);
    kv("fft_launches", fftLaunches); kv("fft_frames", fftFrames);
    kv("resident", residentOpt ? 1 : 0); kv("resident_launches", st.residentLaunches); kv("resident_blocks", st.residentBlocks);
    kv("conv_direct_io_sets", convDirectSets); kv("conv_long_sets", convLongSets); kv("conv_long", convLong ? 1 : 0); kv("conv_max_long_tap_rows", convMaxQp);
    kv("num_taps", p.taps.size()); kv("taps_in_sets", p.tapsInSets ? 1 : 0); kv("num_tap_nodes", p.taps.size() + p.tapPairs.size()); kv("num_convs", p.convs.size()); kv("conv_workgroups", p.convWork.size());
    s += "\"level_sizes\":[";
    for (size_t l = 0; l + 1 < p.levelOffsets.size(); ++l) { if (l) s += ","; s += std::to_string(p.levelOffsets[l + 1] - p.levelOffsets[l]); }
    s += "],\"root_ids\":[";
    for (size_t i = 0; i < p.rootIds.size(); ++i) { if (i) s += ","; s += std::to_string(p.rootIds[i]); }
    s += "],\"islands\":[";
    for (size_t i = 0; i < p.islands.size(); ++i) {
        const Island& I = p.islands[i];
        if (i) s += ",";
        s += "{\"tasks\":" + std::to_string(I.numTasks) + ",\"stages\":" + std::to_string(I.numStages) +
             ",\"lds_bytes\":" + std::to_string(I.ldsWords * 4) + ",\"consts\":" + std::to_string(I.numCells) +
             ",\"prog_dwords\":" + std::to_string(I.progDwords) + ",\"copies\":" + std::to_string(I.copies) +
             ",\"stateless\":" + std::to_string(I.stateless) + ",\"phases\":[";
        if (p.islandProg[i]) {   // first stage of each pipeline phase (stage tables of the island's program blob)
            const uint32_t* tab = p.islandProg[i]->blob.data() + I.stageOff + 2 * I.numStages + kWaves * (I.numStages + 1);
            for (uint32_t d = 0; d <= I.copies; ++d) { if (d) s += ","; s += std::to_string(tab[d]); }
        }
        s += "],\"waves\":[";
        for (uint32_t w = 0; w < kWaves; ++w) {   // per program wave: [opcode, stage] of its tasks in program order
            if (w) s += ",";
            s += "[";
            for (uint32_t t = I.waveTask[w]; p.islandProg[i] && t < I.waveTask[w + 1]; ++t) {
                const uint32_t d0 = p.islandProg[i]->blob[t * 8u];
                if (t != I.waveTask[w]) s += ",";
                s += "[" + std::to_string(d0 & 0xFFFFu) + "," + std::to_string((d0 >> 16) & 0xFFu) + "]";
            }
            s += "]";
        }
        s += "]}";
        if (i >= 63) break;
    }
    s += "]}";
    return s;
}

} // namespace elemhip
