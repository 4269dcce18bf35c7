// engine_relay.cpp — the event relay: processQueuedEvents and eventWindowBlocks.
#include "engine_impl.h"
#include <functional>

#include "fft_frames.h"
#include "event_replay.h"
#include "event_fold.h"
#include "capture_replay.h"

namespace elemhip {

// ---- the event relay (Runtime.h:437-446, GraphRenderSequence.h:189-198, builtins/Analyzers.h, Capture.h, mc/Capture.h) -------------
//
// The reference drains lock-free queues: its audio thread never notices a relay. Here the readouts live in device memory, so
// the relay (a) takes the render lock only to ENQUEUE a device-side snapshot of the event nodes' records behind the blocks
// already queued (stream order makes it consistent) and, at the end, to queue the read-position updates as parameter patches;
// (b) waits for that snapshot, fetches the ring ranges it names and calls the host back WITHOUT the render lock — a render
// thread that calls process() meanwhile is not held up by a synchronise or a copy (r04 held `mu` across both).
// What a ring range holds cannot change under the copy: kernels only write ahead of the write position the snapshot shows,
// the relay is the only reader, and the rings themselves are freed under `ctl`, which the relay holds throughout.
//
// blockwise = false: the reference's processQueuedEvents — per node the NEWEST readout since the last relay.
// blockwise = true:  what the reference's offline caller produces by relaying after EVERY block (offline-renderer/index.ts:112-120),
//   reconstructed after a whole launch set from the per-block readout logs the kernels keep (device.h EVT_LOG): every block's
//   events in block order, nodes in render order inside a block. Exact while a relay window stays within eventWindowBlocks().
//
// The decisions that need neither HIP nor the engine — host blocks of a sliced window, the meter / snapshot folds, the scope's runs —
// are event_fold.h's (namespace evf), next to event_replay.h's ring replay; the readers below do the fetching and the formatting.
struct RelayCtx {
    bool blockwise = false;
    // A host block longer than the engine's renders as k slices, each an engine block with readouts of its own; the reference's nodes
    // see ONE block: the slices of a host block are put back together — win.sliced, win.hostEnds, win.windowBlocks (event_fold.h).
    evf::Window win;
    uint64_t lastBlock = 0;                    // newest host block of the window
    uint32_t hostFrames = 0;                   // frames of a host block
    hipStream_t stream = nullptr;              // the relay's stream
    struct Item { Node* n; size_t recOff; uint32_t order; };
    std::vector<Item> items;                   // event nodes of active roots, render order; recOff: the node's record in hRelay
    struct Ev { uint64_t block; uint32_t order; const char* type; std::string json; };
    std::vector<Ev> evs;
    struct Wb { Node* n; uint32_t dword; uint32_t value; };
    std::vector<Wb> writeBack;                 // read positions that go back to the device in phase (c)
    struct FftEmit { uint64_t block; size_t outFloat; };
    std::vector<std::vector<FftEmit>> fftEmits;   // per item: the spectra relayFftFrames left in hFft

    // a stretch [from, from + count) of a device ring of `cap` entries of `entryFloats` floats each, wrapped, into `dst`
    // (Async: queued on the relay's stream, the caller synchronises once behind all its stretches)
    bool fetchRingAsync(const float* base, uint32_t cap, uint32_t from, uint32_t count, uint32_t entryFloats, float* dst) const {
        if (!count) return true;
        from %= cap;
        const uint32_t first = std::min(count, cap - from);
        if (hipMemcpyAsync(dst, base + (size_t)from * entryFloats, (size_t)first * entryFloats * 4, hipMemcpyDeviceToHost, stream) != hipSuccess) return false;
        if (count > first && hipMemcpyAsync(dst + (size_t)first * entryFloats, base, (size_t)(count - first) * entryFloats * 4, hipMemcpyDeviceToHost, stream) != hipSuccess) return false;
        return true;
    }
    bool fetchRing(const float* base, uint32_t cap, uint32_t from, uint32_t count, uint32_t entryFloats, float* dst) const {
        return fetchRingAsync(base, cap, from, count, entryFloats, dst) && hipStreamSynchronize(stream) == hipSuccess;
    }
};

static std::string numStr(float v) { char b[64]; std::snprintf(b, sizeof b, "%.17g", (double)v); return std::string(b); }
static void numList(std::string& j, const float* v, size_t count) { for (size_t i = 0; i < count; ++i) { if (i) j += ", "; j += numStr(v[i]); } }
static std::string srcOf(const Node& n) {
    std::string src = "null";
    auto nm = n.props.find("name");
    if (nm != n.props.end() && nm->second.isString()) { src = "\""; for (char ch : nm->second.str) { if (ch == '"' || ch == '\\') src += '\\'; src += ch; } src += "\""; }
    return src;
}

// ---- scope / fft rings: the reads of this relay (event_replay.h). emit(host block of the window, absolute index of the frame's
// first sample); the frame's samples sit at that index, wrapped, in the device ring of n.ringFrames frames per channel. ----
// plain relay: ONE read at the positions the device kept — no relay came in between, so its overrun nudges are the reference's.
// blockwise:   the device's read position is NOT what a relay after every block would have left (the kernel never saw the reads in
//   between): the window is replayed from the positions the previous relay established, kept on the host per node — write rule,
//   then the read comparison, per HOST block — and the final read position goes back to the device. A frame the device ring no
//   longer holds (a window longer than eventWindowBlocks()) is dropped rather than handed on with newer samples in it.
static void ringReads(RelayCtx& c, Node& n, const uint32_t* rc_, uint32_t size, evr::Cmp cmp, const std::function<void(uint64_t, uint64_t)>& emit) {
    const uint32_t fresh = rc_[rec::SCP_ABS] - (uint32_t)n.ringWritten;      // frames written since the last relay
    const uint64_t writtenEnd = n.ringWritten + fresh;
    evr::Pos p;
    if (!c.blockwise) {
        p.written = writtenEnd; p.read = rc_[rec::SCP_READ];
        uint64_t first;
        if (evr::read_frame(p, size, cmp, first) && emit) emit(c.lastBlock, first);
    } else {
        p.written = n.ringWritten; p.read = n.ringRead;
        // whole host blocks; what does not fit the window's count (blocks rendered while the node's root was off, a short first
        // call) was written with no relay behind it
        uint64_t blocks = fresh / c.hostFrames;
        if (fresh % c.hostFrames) evr::write_block(p, fresh % c.hostFrames);
        for (; blocks > std::max<uint64_t>(1, c.win.hostBlocks()); --blocks) evr::write_block(p, c.hostFrames);
        const uint64_t firstBlock = c.lastBlock + 1 >= blocks ? c.lastBlock + 1 - blocks : 0;
        p = evr::replay(p, c.hostFrames, size, cmp, (uint32_t)blocks, [&](uint32_t b, uint64_t first) {
            if (emit && writtenEnd - first <= (uint64_t)n.ringFrames) emit(std::min<uint64_t>(c.lastBlock, firstBlock + b), first);
        });
    }
    n.ringWritten = p.written; n.ringRead = p.read;
    if (p.read != rc_[rec::SCP_READ]) c.writeBack.push_back({&n, rec::SCP_READ, p.read});
}

// ---- fft nodes (wasm/FFT.h:92-132): what every node hands on in this window, then ONE launch for all frames ----
// A relay emits at most one frame per node (`ringBuffer.size() >= size`, where scope has `>`); the blockwise relay replays that
// comparison after every host block of the window (ringReads), as relayScope does: up to a frame per node and block,
// all of them in ONE launch. The kernel reads the rings where the replay says the frames are and writes into the relay's own
// buffer, on the relay's stream: the render thread is not involved.
int Engine::relayFftFrames(RelayCtx& c) {
    c.fftEmits.assign(c.items.size(), {});
    std::vector<FftFrame> frames;
    size_t outFloats = 0;
    uint32_t maxSize = 0;
    for (size_t ix = 0; ix < c.items.size(); ++ix) {
        Node& n = *c.items[ix].n;
        if (n.op != OP_FFT) continue;
        const uint32_t* rc_ = reinterpret_cast<const uint32_t*>(hRelay + c.items[ix].recOff);
        const uint32_t size = (uint32_t)analyzerSize(n);
        uint32_t lg = 0;
        while ((1u << lg) < size) ++lg;
        // (the ring never holds more than 8191 frames: size 8192 never fires, FFT.h:96 with MultiChannelRingBuffer.h:99-110)
        if (!n.ring.ptr || !ffr::size_ok(size) || !dFftTables[lg]) { ringReads(c, n, rc_, size, evr::kAtLeast, nullptr); continue; }
        const double* tab = static_cast<const double*>(dFftTables[lg]);
        ringReads(c, n, rc_, size, evr::kAtLeast, [&](uint64_t block, uint64_t first) {
            frames.push_back(FftFrame{static_cast<const float*>(n.ring.ptr), tab, tab + size, nullptr, (uint32_t)(first & (n.ringFrames - 1u)), size, n.ringFrames - 1u, 0u});
            c.fftEmits[ix].push_back({block, outFloats});
            outFloats += (size_t)size + 2u;
            maxSize = std::max(maxSize, size);
        });
    }
    if (frames.empty()) return kOk;
    const size_t descBytes = (frames.size() * sizeof(FftFrame) + 255u) & ~(size_t)255u, need = descBytes + outFloats * 4u;
    if (need > fftBytes) {                                   // (only this relay and its stream, idle here, ever touch the pair)
        const size_t capB = std::max<size_t>(need * 2, 65536);
        uint8_t* d = nullptr; uint8_t* h = nullptr;
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&d), capB));
        HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&h), capB, hipHostMallocDefault));
        if (dFft) (void)hipFree(dFft);
        if (hFft) (void)hipHostFree(hFft);
        dFft = d; hFft = h; fftBytes = capB;
    }
    size_t at = 0;
    for (FftFrame& f : frames) { f.out = reinterpret_cast<float*>(dFft + descBytes) + at; at += (size_t)f.size + 2u; }
    std::memcpy(hFft, frames.data(), frames.size() * sizeof(FftFrame));
    HIP_OK(hipMemcpyAsync(dFft, hFft, frames.size() * sizeof(FftFrame), hipMemcpyHostToDevice, c.stream));
    HIP_OK(launch_fft_frames(c.stream, reinterpret_cast<const FftFrame*>(dFft), (uint32_t)frames.size(), maxSize));
    HIP_OK(hipMemcpyAsync(hFft + descBytes, dFft + descBytes, outFloats * 4u, hipMemcpyDeviceToHost, c.stream));
    HIP_OK(hipStreamSynchronize(c.stream));
    fftLaunches++; fftFrames += frames.size();
    for (auto& v : c.fftEmits) for (RelayCtx::FftEmit& e : v) e.outFloat += descBytes / 4u;
    return kOk;
}

// ... and the events of item `ix`, from the spectra that launch left in hFft
void Engine::relayFft(RelayCtx& c, size_t ix) {
    const Node& n = *c.items[ix].n;
    if (c.fftEmits[ix].empty()) return;
    const size_t bins = (size_t)analyzerSize(n) / 2u + 1u;
    const std::string src = srcOf(n);
    for (const RelayCtx::FftEmit& e : c.fftEmits[ix]) {
        const float* sp = reinterpret_cast<const float*>(hFft) + e.outFloat;
        std::string j = "{\"source\": " + src + ", \"data\": {\"real\": [";
        numList(j, sp, bins);
        j += "], \"imag\": [";
        numList(j, sp + bins, bins);
        j += "]}}";
        c.evs.push_back({e.block, c.items[ix].order, "fft", std::move(j)});
    }
}

int Engine::relayScope(RelayCtx& c, Node& n, const uint32_t* rc_, uint32_t order) {   // Analyzers.h:192-245, MultiChannelRingBuffer.h:61-86
    auto ch = n.props.find("channels");
    const size_t size = (size_t)analyzerSize(n), channels = std::min<size_t>(4, (size_t)((ch != n.props.end() && ch->second.isNumber()) ? ch->second.num : 1.0));
    if (!n.ring.ptr || size == 0) return kOk;
    if (size >= evr::kRefRing) { ringReads(c, n, rc_, (uint32_t)size, evr::kMoreThan, nullptr); return kOk; }   // (never fires: the ring holds 8191 at most)
    evf::ScopeRuns sr;       // the frames to fetch, as runs of absolute frame indices (event_fold.h)
    ringReads(c, n, rc_, (uint32_t)size, evr::kMoreThan, [&](uint64_t block, uint64_t first) { sr.add(block, first, size); });
    if (sr.emits.empty()) return kOk;
    sr.layout();
    std::vector<float> host((size_t)channels * sr.span);
    const uint32_t cap = n.ringFrames;
    bool ok = true;
    for (size_t k = 0; k < channels && ok; ++k)
        for (const evf::ScopeRuns::Run& run : sr.runs)
            if (!(ok = c.fetchRingAsync((const float*)n.ring.ptr + k * cap, cap, (uint32_t)(run.first & (cap - 1u)), (uint32_t)run.frames, 1, host.data() + k * sr.span + run.at))) break;
    if (!ok || hipStreamSynchronize(c.stream) != hipSuccess) return kHipError;
    const std::string src = srcOf(n);
    for (const evf::ScopeRuns::Emit& e : sr.emits) {
        const size_t at = sr.offset(e);
        std::string j = "{\"source\": " + src + ", \"data\": [";
        for (size_t k = 0; k < channels; ++k) {
            j += k ? ", [" : "[";
            numList(j, host.data() + k * sr.span + at, size);
            j += "]";
        }
        j += "]}";
        c.evs.push_back({e.block, order, "scope", std::move(j)});
    }
    return kOk;
}

// Capture.h:60-95 / mc/Capture.h:107-146: drain the ring(s) into the relay, emit once the gate fell
// A node made with history (option "capture_history_blocks") under the blockwise relay: the per-block log says what a relay after every
// block would have drained and when it would have emitted (capture_replay.h) — the window's frames come over in ONE stretch per
// channel and are cut into those takes; the device's positions are left as such a relay would have left them. Its ring is addressed
// by CAP_ABS, so the plain relay fetches the `avail` frames the reference's positions name from behind that count.
int Engine::relayCapture(RelayCtx& c, Node& n, const uint32_t* rc_, uint32_t order) {
    const uint32_t* sh = shadow.data() + (size_t)n.rec * kRecDwords;
    const uint32_t mask = sh[rec::CAP_REFMASK], cap = sh[rec::CAP_MASK] + 1u;       // the reference's positions; frames of the device ring
    const uint32_t chans = n.mc ? sh[rec::CAP_CHANS] : 1u;
    const uint32_t w = rc_[rec::CAP_WRITE], r = rc_[rec::CAP_READ], ready = rc_[rec::CAP_READY];
    // `count` frames of every channel from ring index `from` to the end of the relay buffer(s)
    auto drain = [&](uint32_t from, uint32_t count) {
        if (n.mc) { if (n.relayCh.size() != chans) n.relayCh.resize(chans); }      // (pendingEventData.resize(numChansToRead))
        for (uint32_t k = 0; k < chans; ++k) {
            std::vector<float>& dst = n.mc ? n.relayCh[k] : n.relay;
            const size_t at = dst.size();
            dst.resize(at + count);
            if (!c.fetchRingAsync((const float*)n.ring.ptr + (size_t)k * cap, cap, from, count, 1, dst.data() + at)) return false;
        }
        return hipStreamSynchronize(c.stream) == hipSuccess;
    };
    // the event of a take after host block `block`: the relay buffer(s) but for their newest `keep` frames, which belong to a later take
    auto emit = [&](uint64_t block, size_t keep) {
        std::string j = "{\"source\": " + srcOf(n) + ", \"data\": [";
        auto cut = [&](std::vector<float>& v) { const size_t m = v.size() - std::min(keep, v.size()); numList(j, v.data(), m); v.erase(v.begin(), v.begin() + (std::ptrdiff_t)m); };
        if (n.mc) for (size_t k = 0; k < n.relayCh.size(); ++k) { j += k ? ", [" : "["; cut(n.relayCh[k]); j += "]"; }
        else cut(n.relay);
        j += "]}";
        c.evs.push_back({block, order, n.mc ? "mc.capture" : "capture", std::move(j)});
    };
    if (c.blockwise && n.captureHistoryBlocks && n.ring.ptr && chans > 0) {
        const uint32_t lcap = sh[rec::CAP_LOGMASK] + 1u, blk = rc_[rec::CAP_BLK], take = std::min(blk - n.logRelayed, lcap);
        std::vector<uint32_t> e((size_t)take * 4);
        if (take && !c.fetchRing((const float*)n.ring.ptr + (size_t)chans * cap, lcap, blk - take, take, 4, reinterpret_cast<float*>(e.data()))) return kHipError;
        std::vector<cpr::Entry> blocks = cpr::fold(c.win, e.data(), take);
        if (blocks.empty()) blocks.push_back({c.lastBlock, rc_[rec::CAP_ABS], false});   // (nothing rendered since: a pending flag still goes out)
        bool pending = ready != 0u;
        for (const cpr::Entry& b : blocks) if (b.fell) pending = false;
        std::vector<cpr::Take> takes;
        const uint64_t end = cpr::replay(blocks.data(), blocks.size(), n.capRelayed, pending, takes);
        // (a window longer than eventWindowBlocks(): the ring holds the newest frames only — 128 of it may be the scratch ahead)
        const uint64_t from = std::max(n.capRelayed, end - std::min<uint64_t>(end, cap - 128u));
        if (end > from && !drain((uint32_t)from, (uint32_t)(end - from))) return kHipError;
        for (const cpr::Take& t : takes) emit(t.block, (size_t)(end - std::max(t.end, from)));
        n.capRelayed = end; n.logRelayed = blk;
        if (r != w) c.writeBack.push_back({&n, rec::CAP_READ, w});
        if (ready) c.writeBack.push_back({&n, rec::CAP_READY, 0u});
        return kOk;
    }
    const uint32_t avail = evf::capture_avail(w, r, mask);
    if (avail > 0 && n.ring.ptr && chans > 0) {
        // (without history CAP_ABS - avail IS the read position, mod the ring)
        if (!drain(n.captureHistoryBlocks ? rc_[rec::CAP_ABS] - avail : r, avail)) return kHipError;
        c.writeBack.push_back({&n, rec::CAP_READ, (r + avail) & mask});
    }
    n.capRelayed = cpr::unwrap(n.capRelayed, rc_[rec::CAP_ABS]); n.logRelayed = rc_[rec::CAP_BLK];
    if (!ready) return kOk;
    c.writeBack.push_back({&n, rec::CAP_READY, 0u});
    emit(c.lastBlock, 0);
    return kOk;
}

int Engine::relayMeter(RelayCtx& c, Node& n, const uint32_t* rc_, uint32_t order) {   // Analyzers.h:23-62
    const uint32_t count = rc_[rec::EVT_COUNT], fresh = count - n.eventCount;
    const uint32_t lcap = shadow[(size_t)n.rec * kRecDwords + rec::EVT_LOGMASK] + 1u;
    if (!fresh) return kOk;
    auto emit = [&](uint64_t block, float mn, float mx) { c.evs.push_back({block, order, "meter", "{\"min\": " + numStr(mn) + ", \"max\": " + numStr(mx) + ", \"source\": " + srcOf(n) + "}"}); };
    if (n.ring.ptr && (c.win.sliced || (c.blockwise && fresh > 1u))) {
        const uint32_t take = std::min(fresh, lcap);
        std::vector<uint32_t> e((size_t)take * 4);
        if (!c.fetchRing((const float*)n.ring.ptr, lcap, count - take, take, 4, reinterpret_cast<float*>(e.data()))) return kHipError;
        for (const evf::MeterOut& g : evf::fold_meter(c.win, e.data(), take, c.blockwise)) emit(g.block, g.mn, g.mx);
    } else if (!evf::wraps_to_empty(fresh)) emit(c.lastBlock, evf::as_float(rc_[rec::EVT_A]), evf::as_float(rc_[rec::EVT_B]));
    n.eventCount = count;
    return kOk;
}

int Engine::relaySnapshot(RelayCtx& c, Node& n, const uint32_t* rc_, uint32_t order) {   // Analyzers.h:83-131
    const uint32_t count = rc_[rec::EVT_COUNT], blk = rc_[rec::EVT_BLK], logn = rc_[rec::EVT_LOGN];
    const uint32_t lcap = shadow[(size_t)n.rec * kRecDwords + rec::EVT_LOGMASK] + 1u;
    if (count == n.eventCount) { n.logRelayed = logn; return kOk; }
    const uint32_t fresh = logn - n.logRelayed;
    auto emit = [&](uint64_t block, float v) { c.evs.push_back({block, order, "snapshot", "{\"source\": " + srcOf(n) + ", \"data\": " + numStr(v) + "}"}); };
    if (c.blockwise && n.ring.ptr && fresh >= 1u) {
        const uint32_t take = std::min(fresh, lcap);
        std::vector<uint32_t> e((size_t)take * 4);
        if (!c.fetchRing((const float*)n.ring.ptr, lcap, logn - take, take, 4, reinterpret_cast<float*>(e.data()))) return kHipError;
        for (const evf::SnapshotOut& s : evf::fold_snapshot(c.win, e.data(), take, blk)) emit(s.block, s.value);
    } else if (!evf::wraps_to_empty(count - n.eventCount)) emit(c.lastBlock, evf::as_float(rc_[rec::EVT_B]));
    n.eventCount = count; n.logRelayed = logn;
    return kOk;
}

int Engine::processQueuedEvents(void (*cb)(const char*, const char*, void*), void* user, bool blockwise) {
    std::lock_guard<std::mutex> control(ctl);
    if (dry || !cb) return kOk;
    RelayCtx c;
    c.blockwise = blockwise; c.win.sliced = hostBlockSize != blockSize; c.hostFrames = (uint32_t)hostBlockSize;
    std::shared_ptr<Plan> plan;
    uint64_t blocksNow = 0;
    {   // ---- (a) under the render lock: snapshot of the records, stream-ordered behind everything rendered so far ----
        RenderGuard lock(*this);
        if (!current) return kOk;
        if (hipSetDevice(device) != hipSuccess) return kHipError;
        plan = current;
        uint32_t order = 0;
        for (auto& en : plan->eventNodes) {
            auto nit = nodes.find(en.first), rit = nodes.find(en.second);
            if (nit == nodes.end() || rit == nodes.end()) continue;
            auto a = rit->second.props.find("active");                       // GraphRenderSequence.h:192
            if (a == rit->second.props.end() || !a->second.isBool() || !a->second.b) continue;
            bool seen = false;                                              // (an mc.* node is one plan entry per output channel: relayed once)
            for (const RelayCtx::Item& it : c.items) if (it.n == &nit->second) { seen = true; break; }
            if (seen) continue;
            c.items.push_back({&nit->second, c.items.size() * kRecDwords * 4, order++});
        }
        blocksNow = st.blocksRendered;
        c.win.windowBlocks = blocksNow - relayBlocksMark;
        if (c.win.sliced) {
            std::vector<uint64_t>& hostEnds = c.win.hostEnds;
            for (uint64_t e : hostBlockEnds) if (e > relayBlocksMark && e <= blocksNow) hostEnds.push_back(e - relayBlocksMark);
            if (c.win.windowBlocks && (hostEnds.empty() || hostEnds.back() != c.win.windowBlocks)) hostEnds.push_back(c.win.windowBlocks);
        }
        if (c.items.empty()) { relayBlocksMark = blocksNow; hostBlockEnds.clear(); return kOk; }
        const size_t need = c.items.size() * kRecDwords * 4;
        if (need > relayBytes) {
            const size_t cap = std::max<size_t>(need * 2, 16384);
            uint8_t* d = nullptr; uint8_t* h = nullptr;
            HIP_OK(hipMalloc(reinterpret_cast<void**>(&d), cap));
            HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&h), cap, hipHostMallocDefault));
            if (dRelay) deferredFree.push_back(dRelay);
            if (hRelay) (void)hipHostFree(hRelay);
            dRelay = d; hRelay = h; relayBytes = cap;
        }
        if (!relayStream) {
            HIP_OK(hipStreamCreateWithFlags(&relayStream, hipStreamNonBlocking));
            HIP_OK(hipEventCreateWithFlags(&evRelay, hipEventDisableTiming));
        }
        // (parameter patches still waiting for the next block — a read position written by the previous relay — go first)
        int rc = flushPending();
        if (rc != kOk) return rc;
        for (const RelayCtx::Item& it : c.items)
            HIP_OK(hipMemcpyAsync(dRelay + it.recOff, dRecs + (size_t)it.n->rec * kRecDwords, kRecDwords * 4, hipMemcpyDeviceToDevice, stream));
        HIP_OK(hipEventRecord(evRelay, stream));
    }
    // ---- (b) without the render lock: wait for the snapshot, fetch what it names — the fft nodes' one launch, then a reader per node ----
    HIP_OK(hipStreamWaitEvent(relayStream, evRelay, 0));
    HIP_OK(hipMemcpyAsync(hRelay, dRelay, c.items.size() * kRecDwords * 4, hipMemcpyDeviceToHost, relayStream));
    HIP_OK(hipStreamSynchronize(relayStream));
    c.stream = relayStream; c.lastBlock = c.win.lastBlock();
    int rc = relayFftFrames(c);
    for (size_t ix = 0; ix < c.items.size() && rc == kOk; ++ix) {
        Node& n = *c.items[ix].n;
        const uint32_t* rc_ = reinterpret_cast<const uint32_t*>(hRelay + c.items[ix].recOff);
        const uint32_t order = c.items[ix].order;
        if (n.op == OP_FFT) relayFft(c, ix);
        else if (n.op == OP_SCOPE) rc = relayScope(c, n, rc_, order);
        else if (n.op == OP_CAPTURE) rc = relayCapture(c, n, rc_, order);
        else if (n.op == OP_METER) rc = relayMeter(c, n, rc_, order);
        else rc = relaySnapshot(c, n, rc_, order);
    }
    if (rc != kOk) return rc;
    {   // ---- (c) read positions back to the device: parameter patches, applied in stream order at once (no synchronise) ----
        RenderGuard lock(*this);
        for (const RelayCtx::Wb& w : c.writeBack) writeParam(*w.n, w.dword, w.value);
        relayBlocksMark = blocksNow;
        while (!hostBlockEnds.empty() && hostBlockEnds.front() <= blocksNow) hostBlockEnds.pop_front();
        if (!c.writeBack.empty()) { const int rc2 = flushPending(); if (rc2 != kOk) return rc2; }
    }
    // ---- (d) the host's callbacks, in block order (stable: nodes stay in render order inside a block) ----
    if (blockwise) std::stable_sort(c.evs.begin(), c.evs.end(), [](const RelayCtx::Ev& a, const RelayCtx::Ev& b) { return a.block != b.block ? a.block < b.block : a.order < b.order; });
    for (const RelayCtx::Ev& e : c.evs) cb(e.type, e.json.c_str(), user);
    return kOk;
}

// How many blocks may pass between two blockwise relays for their result to be exactly the per-block relay's: the per-block
// readout logs hold 1024 blocks; a scope or fft ring of 8192 frames (`size` of them per event) must not overrun inside a window — one
// made with history (option "event_history_blocks" = W) serves W blocks; a capture node's take is placed by the relay that sees its
// gate fall, so it wants a relay per block — unless it was made with a history and a per-block log of its own ("capture_history_blocks").
uint32_t Engine::eventWindowBlocks() {
    std::lock_guard<std::mutex> control(ctl);
    RenderGuard lock(*this);
    const std::shared_ptr<Plan> pl = pending ? pending : current;
    // in HOST blocks (what the caller counts in): a host block of k slices fills k entries of the per-block readout logs
    const uint32_t perHost = (uint32_t)((hostBlockSize + blockSize - 1) / blockSize);
    uint32_t w = std::max(1u, kEventLogEntries / std::max(1u, perHost));
    if (!pl) return w;
    for (auto& en : pl->eventNodes) {
        auto nit = nodes.find(en.first);
        if (nit == nodes.end()) continue;
        const Node& n = nit->second;
        // a capture ring with history (option "capture_history_blocks") keeps that many blocks of takes and the per-block log the relay
        // places them by (capture_replay.h); without it the take is placed by the relay that sees the gate fall: a relay per block
        if (n.op == OP_CAPTURE) { if (!n.captureHistoryBlocks) return 1u; w = std::min(w, n.captureHistoryBlocks); continue; }
        // a ring with history (option "event_history_blocks") holds every frame a per-block relay hands on over that many blocks, and
        // the relay replays the reads: whatever `size`, overruns included
        if ((n.op == OP_SCOPE || n.op == OP_FFT) && n.historyBlocks) { w = std::min(w, n.historyBlocks); continue; }
        const double size = analyzerSize(n);
        if (n.op == OP_SCOPE) {
            // a scope whose `size` is below the block hands on less per relay than a block brings: its ring overruns under a per-block
            // relay too, and where it does depends on every single relay — only a relay per block reproduces that
            if (size < (double)hostBlockSize) return 1u;
            const double room = 8192.0 - 1.0 - std::max(1.0, size);
            w = std::min<uint32_t>(w, (uint32_t)std::max(1.0, std::floor(room / (double)hostBlockSize)));
        }
        if (n.op == OP_FFT) {
            // as the scope, with `>=` where the scope compares with `>`: under a per-block relay the ring holds at most size - 1 frames
            // when a window begins, so w blocks fit without an overrun while size - 1 + w * block <= 8191
            if (size < (double)hostBlockSize) return 1u;
            w = std::min<uint32_t>(w, (uint32_t)std::max(1.0, std::floor((8192.0 - size) / (double)hostBlockSize)));
        }
    }
    return w;
}

} // namespace elemhip
