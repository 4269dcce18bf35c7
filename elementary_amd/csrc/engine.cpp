// engine.cpp — the engine's construction and teardown, its device-resident node records, rings and resources, gc and options.
// See engine.h for the mapping onto runtime/elem/Runtime.h. The other units behind engine.h: engine_nodes.cpp (instruction
// interpreter and node table), engine_relay.cpp (event relay), engine_render.cpp (the per-block launch sequence and launch sets).
#include "engine_impl.h"
#include "flac_encode.h"
#include "fft_frames.h"

namespace elemhip {

const char* describe(int c) {
    switch (c) {   // 0..8: runtime/elem/Types.h:62-85
        case 0: return "Ok";
        case 1: return "Node type not recognized";
        case 2: return "Node not found";
        case 3: return "Attempting to create a node that already exists";
        case 4: return "Attempting to create a node type that already exists";
        case 5: return "Invalid value type for the given node property";
        case 6: return "Invalid value for the given node property";
        case 7: return "Invariant violation";
        case 8: return "Invalid instruction format";
        case kHipError: return "HIP runtime error";
        case kNoDevice: return "No HIP device available";
        case kBlockTooLarge: return "numSamples exceeds the block size the runtime was created with";
        case kTooManyChannels: return "Too many host channels";
        case kUnsupportedGraph: return "Graph uses a construct the HIP engine does not support";
        case kJsonParseError: return "Failed to parse json string";
        case kFlacInput: return "A FLAC input frame does not decode";
        default: return "Return code not recognized";
    }
}

ProgHeap::~ProgHeap() { if (dev) (void)hipFree(dev); }

Plan::~Plan() {
    if (graphExec) (void)hipGraphExecDestroy(graphExec);
    if (dev.ptr) { if (pool) pool->give(dev); else (void)hipFree(dev.ptr); }
}

DevBuf TablePool::take(size_t bytes) {
    {
        std::lock_guard<std::mutex> lock(m);
        size_t best = free.size();
        for (size_t k = 0; k < free.size(); ++k)
            if (free[k].bytes >= bytes && free[k].bytes <= 4 * bytes && (best == free.size() || free[k].bytes < free[best].bytes)) best = k;
        if (best != free.size()) { DevBuf b = free[best]; free.erase(free.begin() + (long)best); return b; }
    }
    DevBuf b;
    b.bytes = bytes + bytes / 4 + 4096;    // (the next plan of a live graph is a little bigger or smaller)
    if (hipMalloc(&b.ptr, b.bytes) != hipSuccess) { b.ptr = nullptr; b.bytes = 0; }
    return b;
}

void TablePool::give(DevBuf b) {
    std::lock_guard<std::mutex> lock(m);
    free.push_back(b);
    if (free.size() > 8) { (void)hipFree(free.front().ptr); free.erase(free.begin()); }
}

TablePool::~TablePool() { for (DevBuf& b : free) (void)hipFree(b.ptr); }

// ---------------------------------------------------------------------------------------------
Engine::Engine(double sr, int bs, int dev) : sampleRate(sr), blockSize(bs), device(dev) {
    auto fail = [&](int code) { initErr = code; };
    // A block's buffers are LDS slots of at most kMaxBlock frames. A longer host block is rendered as k equal slices — the smallest k
    // that divides it into slices of 64 .. kMaxBlock frames (1024 -> 2 x 512, 700 -> 2 x 350, 1023 -> 3 x 341; r04 took multiples of
    // 512 only) — the sample-rate nodes cannot tell; taps, whose delay IS the host's block (Feedback.h:29-31, 66-67, 103-104), keep
    // shared buffers of the HOST's block size and every slice reads / writes its own stretch of them (setTapSlice): the engine's own
    // block size is the slice, the host's the limit of a process() call. A size no such k divides (a prime above 512: 521, 1031) is
    // rendered as slices of kMaxBlock frames and a shorter last one — to the kernels the same as a host that calls process() with
    // fewer frames than the block size (r04 / early r05 refused such sizes).
    hostBlockSize = bs;
    if (bs > (int)kMaxBlock && bs <= 64 * (int)kMaxBlock) {
        bool equal = false;
        for (int k = (bs + (int)kMaxBlock - 1) / (int)kMaxBlock; k <= bs / 64; ++k)
            if (bs % k == 0) { bs /= k; blockSize = bs; equal = true; break; }
        if (!equal) { bs = (int)kMaxBlock; blockSize = bs; }
    }
    if (const char* e = std::getenv("ELEMHIP_SPECIALIZE")) specialize = std::max(0, std::min(2, std::atoi(e)));
    if (const char* e = std::getenv("ELEMHIP_SYNC_POLL")) syncPoll = std::atoi(e) != 0;
    if (const char* e = std::getenv("ELEMHIP_RESIDENT")) residentOpt = std::atoi(e) != 0;   // (a native host without access to the options)
    if (const char* e = std::getenv("ELEMHIP_PLAN_CACHE")) planCache = std::max(0, std::min(2, std::atoi(e)));   // 2: verify mode (tests)
    if (bs <= 0 || bs > (int)kMaxBlock) { fail(kBlockTooLarge); return; }
    if (dev == -1) {
        // "dry" engine: host logic only (instruction decode, graph mutation, plan build, gc) with
        // no device behind it. It cannot render: process() returns kNoDevice. Used by CPU-only tests.
        dry = true;
        hGlobals = Globals{};
        hGlobals.numSamples = (uint32_t)bs; hGlobals.ringSlots = 1; hGlobals.blockStride = (uint32_t)bs;
        hGlobals.sampleRateF = (float)sr; hGlobals.sampleRate = sr;
        return;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { fail(kNoDevice); return; }
    if (dev < 0 || dev >= count) { fail(kNoDevice); return; }
    if (hipSetDevice(dev) != hipSuccess) { fail(kHipError); return; }
    if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) { fail(kHipError); return; }
    ownStream = true;
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) cuCount = cus; }

    recCapacity = 8192;
    if (hipMalloc(&dRecs, (size_t)recCapacity * kRecDwords * 4) != hipSuccess) { fail(kHipError); return; }
    (void)hipMemsetAsync(dRecs, 0, (size_t)recCapacity * kRecDwords * 4, stream);
    (void)hipStreamSynchronize(stream);
    shadow.reserve((size_t)recCapacity * kRecDwords);

    patchCap = 1u << 16;
    if (hipHostMalloc((void**)&hPatches, sizeof(Patch) * patchCap, hipHostMallocDefault) != hipSuccess) { fail(kHipError); return; }

    hGlobals = Globals{};
    hGlobals.sampleTime = 0;
    hGlobals.numSamples = (uint32_t)bs;
    hGlobals.ringSlots = 1;
    hGlobals.blockStride = (uint32_t)bs;
    hGlobals.sampleRateF = (float)sr;
    hGlobals.sampleRate = sr;
    if (hipMalloc(&dGlobals, sizeof(Globals)) != hipSuccess) { fail(kHipError); return; }
    (void)hipMemcpy(dGlobals, &hGlobals, sizeof(Globals), hipMemcpyHostToDevice);

    {   // FFT twiddles for `convolve` (conv.hip): cis(-2 pi k / 1024) rounded from double
        std::vector<float> tw(2 * conv::kFft);
        for (uint32_t k = 0; k < conv::kFft; ++k) {
            const double a = -2.0 * 3.14159265358979323846 * (double)k / (double)conv::kFft;
            tw[2 * k] = (float)std::cos(a); tw[2 * k + 1] = (float)std::sin(a);
        }
        std::vector<float> tw8(2 * 8192);     // ... and cis(-2 pi j / 8192) for the long-partition transforms (conv_long.inc, fft4096.h)
        for (uint32_t k = 0; k < 8192; ++k) {
            const double a = -2.0 * 3.14159265358979323846 * (double)k / 8192.0;
            tw8[2 * k] = (float)std::cos(a); tw8[2 * k + 1] = (float)std::sin(a);
        }
        if (upload_convolve_tables(tw.data(), tw8.data()) != hipSuccess) { fail(kHipError); return; }
    }
    // LCG jump-ahead table for `rand` (Noise.h:28-32): s_k = A[k]*s_0 + C[k] (mod 2^32)
    std::vector<uint32_t> lcg(2 * (kMaxBlock + 1));
    uint32_t A = 1, Cc = 0;
    for (uint32_t k = 0; k <= kMaxBlock; ++k) {
        lcg[2 * k] = A; lcg[2 * k + 1] = Cc;
        A = 214013u * A; Cc = 214013u * Cc + 2531011u;
    }
    if (hipMalloc(&dLcg, lcg.size() * 4) != hipSuccess) { fail(kHipError); return; }
    (void)hipMemcpy(dLcg, lcg.data(), lcg.size() * 4, hipMemcpyHostToDevice);

    if (ensureHbm(kMaxHostIn + 64) != kOk) { fail(kHipError); return; }
    if (ensureOutRing((size_t)8 * bs) != kOk) { fail(kHipError); return; }
    if (const char* e = std::getenv("ELEMHIP_NO_GRAPH")) useGraph = !(e[0] == '1');
}

Engine::~Engine() {
    for (auto& kv : nodes) if (kv.second.hostInst && kv.second.hostVt && kv.second.hostVt->destroy) kv.second.hostVt->destroy(kv.second.hostInst, kv.second.hostVt->user);
    if (dry) {
        for (auto& kv : nodes) std::free(kv.second.ring.ptr);
        for (auto& kv : resources) { std::free(kv.second->dev.ptr); for (DevBuf& d : kv.second->devCh) std::free(d.ptr); }
        return;
    }
    residentStop();
    if (stream) (void)hipStreamSynchronize(stream);
    if (hResident) (void)hipHostFree(hResident);
    if (hDone) (void)hipHostFree(hDone);
    if (hResIn) (void)hipHostFree(hResIn);
    if (hResOut) (void)hipHostFree(hResOut);
    if (dResidentSync) (void)hipFree(dResidentSync);
    current.reset(); pending.reset();
    for (auto& kv : nodes) if (kv.second.ring.ptr) (void)hipFree(kv.second.ring.ptr);
    for (auto& kv : resources) { if (kv.second->dev.ptr) (void)hipFree(kv.second->dev.ptr); for (DevBuf& d : kv.second->devCh) if (d.ptr) (void)hipFree(d.ptr); }
    freeDeferred();
    if (dRecs) (void)hipFree(dRecs);
    if (dGlobals) (void)hipFree(dGlobals);
    if (dLcg) (void)hipFree(dLcg);
    if (dConvScratch) (void)hipFree(dConvScratch);
    if (dHbm) (void)hipFree(dHbm);
    if (dOutRing) (void)hipFree(dOutRing);
    for (hipEvent_t e : profEvents) (void)hipEventDestroy(e);
    for (hipEvent_t e : auxDone) (void)hipEventDestroy(e);
    for (hipStream_t s2 : auxStreams) (void)hipStreamDestroy(s2);
    if (forkEvent) (void)hipEventDestroy(forkEvent);
    if (hPatches) (void)hipHostFree(hPatches);
    if (hOut) (void)hipHostFree(hOut);
    if (hIn) (void)hipHostFree(hIn);
    if (ioStream) (void)hipStreamSynchronize(ioStream);
    for (int k = 0; k < 2; ++k) {
        if (hStageOut[k]) (void)hipHostFree(hStageOut[k]);
        if (hStageIn[k]) (void)hipHostFree(hStageIn[k]);
        if (dStageOut[k]) (void)hipFree(dStageOut[k]);
        if (dStageIn[k]) (void)hipFree(dStageIn[k]);
        if (evIn[k]) (void)hipEventDestroy(evIn[k]);
        if (evRendered[k]) (void)hipEventDestroy(evRendered[k]);
        if (evOut[k]) (void)hipEventDestroy(evOut[k]);
    }
    for (int k = 0; k < 2; ++k) { if (hPcm[k]) (void)hipHostFree(hPcm[k]); if (dPcm[k]) (void)hipFree(dPcm[k]); }
    if (dPcmRowBase) (void)hipFree(dPcmRowBase);
    for (int k = 0; k < 2; ++k) { if (hPcmIn[k]) (void)hipHostFree(hPcmIn[k]); if (dPcmIn[k]) (void)hipFree(dPcmIn[k]); }
    if (dPcmInRowBase) (void)hipFree(dPcmInRowBase);
    loudnessFree();
    resampleFree();
    inputResampleFree();
    limiterFree();
    noiseShapeFree();
    spectrumFree(true);
    qcFree();
    flacFree();
    flacInFree();
    if (ioStream) (void)hipStreamDestroy(ioStream);
    if (relayStream) { (void)hipStreamSynchronize(relayStream); (void)hipStreamDestroy(relayStream); }
    if (evRelay) (void)hipEventDestroy(evRelay);
    if (dRelay) (void)hipFree(dRelay);
    if (hRelay) (void)hipHostFree(hRelay);
    if (dFft) (void)hipFree(dFft);
    if (hFft) (void)hipHostFree(hFft);
    for (void* t : dFftTables) if (t) (void)hipFree(t);
    resourceLoadFree();
    if (ownStream && stream) (void)hipStreamDestroy(stream);
}

void Engine::setStream(hipStream_t s) {
    RenderGuard lock(*this);
    if (dry) return;
    if (stream) (void)hipStreamSynchronize(stream);
    if (ownStream && stream) (void)hipStreamDestroy(stream);
    stream = s; ownStream = false;
    dropGraphs();
}

uint32_t Engine::allocRec() {
    uint32_t r;
    if (!freeRecs.empty()) { r = freeRecs.back(); freeRecs.pop_back(); }
    else r = nextRec++;
    if (shadow.size() < (size_t)(r + 1) * kRecDwords) shadow.resize((size_t)(r + 1) * kRecDwords, 0u);
    std::fill(shadow.begin() + (size_t)r * kRecDwords, shadow.begin() + (size_t)(r + 1) * kRecDwords, 0u);
    if (freshFlag.size() <= r) freshFlag.resize((size_t)r + 1, 0);
    freshFlag[r] = 1;
    freshRecs.push_back(r);
    return r;
}

// Channel `ch` of a shared resource on the device (channel 0 is Resource::dev). A channel the resource does not have
// reads as an empty buffer (AudioBufferResource.h:32-40).
int Engine::ensureResourceChannelOnDevice(const ResourcePtr& r, uint32_t ch, const void** ptr, uint32_t* len) {
    *ptr = nullptr; *len = 0;
    if (!r || ch >= r->numChannels()) return kOk;
    *len = (uint32_t)r->frames(ch);
    if (ch == 0) { int rc = ensureResourceOnDevice(r); *ptr = r->dev.ptr; return rc; }
    if (r->devCh.size() <= ch) r->devCh.resize(ch + 1);
    DevBuf& d = r->devCh[ch];
    if (!d.ptr) {                                   // (a resource made on the device has every row already)
        const size_t floats = std::max<size_t>(r->frames(ch), (size_t)blockSize);
        if (dry) { d.ptr = std::calloc(floats, sizeof(float)); std::memcpy(d.ptr, r->channels[ch].data(), r->channels[ch].size() * 4); }
        else {
            HIP_OK(hipMalloc(&d.ptr, floats * sizeof(float)));
            HIP_OK(hipMemsetAsync(d.ptr, 0, floats * sizeof(float), stream));
            HIP_OK(hipStreamSynchronize(stream));
            if (*len) HIP_OK(hipMemcpy(d.ptr, r->channels[ch].data(), (size_t)*len * sizeof(float), hipMemcpyHostToDevice));
        }
        d.bytes = floats * sizeof(float);
    }
    *ptr = d.ptr;
    return kOk;
}

// mc.table (mc/Table.h:12-85): output channel j is TableNode's lookup (Table.h:35-71) into channel j of the resource
void Engine::writeTableChannel(Node& n, uint32_t ch, uint32_t rec) {
    const void* ptr = nullptr; uint32_t len = 0;
    if (n.res) (void)ensureResourceChannelOnDevice(n.res, ch, &ptr, &len);
    const uint64_t v = (uint64_t)reinterpret_cast<uintptr_t>(ptr);
    writeRec(rec, rec::TBL_BUF, (uint32_t)(v & 0xFFFFFFFFu));
    writeRec(rec, rec::TBL_BUF + 1, (uint32_t)(v >> 32));
    writeRec(rec, rec::TBL_LEN, len);
}

// The record of output channel `ch` of a multi-output node. Every channel renders the node's algorithm on its own copy of
// the state (the reference keeps ONE state and loops over the channels inside process(): reader positions and fades
// evolve identically for every channel) and differs only in the resource channel it reads.
uint32_t Engine::channelRec(Node& n, uint32_t ch) {
    if (ch == 0 || !n.mc) return n.rec;
    while (n.chanRecs.size() < ch) {
        const uint32_t r = allocRec();
        n.chanRecs.push_back(r);
        // parameters and INITIAL state as the host last wrote them for channel 0 (pending-buffer flags included)
        std::memcpy(shadow.data() + (size_t)r * kRecDwords, shadow.data() + (size_t)n.rec * kRecDwords, kRecDwords * 4);
        if (n.op == OP_CAPTURE) shadow[(size_t)r * kRecDwords + rec::CAP_CH] = (uint32_t)n.chanRecs.size();   // mc.capture: passes input ch + 1 through (channel 0 records)
        else writeChannelBuffer(n, (uint32_t)n.chanRecs.size(), r);
        // channel 0 has been on the device already (it may be mid-playback): the new channel continues from channel 0's
        // LIVE reader state and consumed flags — the reference keeps one state for all channels (mc/Sample.h, mc/SampleSeq.h)
        // (mc.capture channels > 0 only pass an input through: they have no state to take over, and the clone — dwords P3.. of
        //  channel 0's LIVE record — would overwrite the CAP_CH just set with channel 0's: the new channel would pass input 1 through
        //  and record every block into the shared ring a second time)
        if (!freshFlag[n.rec] && n.op != OP_CAPTURE) recClones.push_back({n.rec, r});
    }
    return n.chanRecs[ch - 1];
}

// buffer pointer / length of resource channel `ch` into record `rec` (table, mc.sample, mc.sampleseq share the slots P0-P2)
void Engine::writeChannelBuffer(Node& n, uint32_t ch, uint32_t rec) {
    static_assert(rec::TBL_BUF == rec::SMP_BUF && rec::TBL_BUF == rec::SSQ_BUF && rec::TBL_LEN == rec::SMP_LEN && rec::TBL_LEN == rec::SSQ_BUFLEN, "shared buffer slots");
    writeTableChannel(n, ch, rec);
}

int Engine::allocRing(Node& n, size_t floats) {
    void* p = nullptr;
    const size_t bytes = std::max<size_t>(floats, 1) * sizeof(float);
    if (dry) {
        p = std::calloc(1, bytes);
        std::free(n.ring.ptr);
        n.ring.ptr = p; n.ring.bytes = bytes;
        return kOk;
    }
    HIP_OK(hipMalloc(&p, bytes));
    HIP_OK(hipMemsetAsync(p, 0, bytes, stream));
    HIP_OK(hipStreamSynchronize(stream));   // callers follow up with blocking hipMemcpy's into the buffer
    if (n.ring.ptr) deferredFree.push_back(n.ring.ptr);
    n.ring.ptr = p; n.ring.bytes = bytes;
    return kOk;
}

// The fft node's tables of one size (fft_frames.h): Blackman-Harris window and transform twiddles, made in double, uploaded once.
int Engine::ensureFftTables(uint32_t size) {
    if (dry || !ffr::size_ok(size)) return kOk;          // (8192 is accepted and never fires: no transform, no tables)
    uint32_t lg = 0;
    while ((1u << lg) < size) ++lg;
    if (dFftTables[lg]) return kOk;
    std::vector<double> host((size_t)size * 3u);
    ffr::make_window(size, host.data());
    ffr::make_twiddles(size, reinterpret_cast<ffr::c2*>(host.data() + size));
    void* d = nullptr;
    HIP_OK(hipMalloc(&d, host.size() * sizeof(double)));
    HIP_OK(hipMemcpy(d, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice));
    dFftTables[lg] = d;
    return kOk;
}

int Engine::ensureResourceOnDevice(const ResourcePtr& r) {
    if (r->dev.ptr) return kOk;
    const size_t have = r->frames(0);
    const size_t floats = std::max<size_t>(have, (size_t)blockSize);
    void* p = nullptr;
    if (dry) { r->dev.ptr = std::calloc(floats, sizeof(float)); r->dev.bytes = floats * sizeof(float); return kOk; }
    HIP_OK(hipMalloc(&p, floats * sizeof(float)));
    HIP_OK(hipMemsetAsync(p, 0, floats * sizeof(float), stream));
    HIP_OK(hipStreamSynchronize(stream));
    if (have) HIP_OK(hipMemcpy(p, r->channels[0].data(), have * sizeof(float), hipMemcpyHostToDevice));
    r->dev.ptr = p; r->dev.bytes = floats * sizeof(float);
    return kOk;
}

// SharedResourceMap::getTapResource (SharedResource.h:79-92)
ResourcePtr Engine::tapResource(const std::string& name) {
    auto it = resources.find(name);
    if (it != resources.end()) return it->second;
    auto r = std::make_shared<Resource>();
    r->channels.emplace_back((size_t)hostBlockSize, 0.0f);      // AudioBufferResource(1, getBlockSize()) (Feedback.h:29-31): the HOST's block
    r->isTap = true;
    resources.emplace(name, r);
    return r;
}

// GainFade::updateCurrentStep (helpers/GainFade.h:107-109)
void Engine::rootUpdateStep(Node& n) {
    n.step = (n.gain > n.target) ? n.outStep : n.inStep;
    writeParamF(n, rec::ROOT_TARGET, n.target);
    writeParamF(n, rec::ROOT_STEP, n.step);
}

// ---- gc / resources -------------------------------------------------------------------------------
void Engine::freeRec(uint32_t r) {   // drop queued writes aimed at the record before it is recycled
    const uint32_t lo = r * kRecDwords, hi = lo + kRecDwords;
    patches.erase(std::remove_if(patches.begin(), patches.end(), [&](const Patch& p) { return p.kind != 2 && p.index >= lo && p.index < hi; }), patches.end());
    if (freshFlag[r]) { freshRecs.erase(std::remove(freshRecs.begin(), freshRecs.end(), r), freshRecs.end()); freshFlag[r] = 0; }
    freeRecs.push_back(r);
}

size_t Engine::gc(int32_t* out, size_t cap) {   // Runtime.h:220-272
    std::lock_guard<std::mutex> control(ctl);
    RenderGuard lock(*this);
    if (!dry) (void)hipSetDevice(device);
    std::vector<int32_t> pruned;
    for (auto it = nodes.begin(); it != nodes.end(); ++it) {
        const int32_t id = it->first;
        const bool held = (current && current->holdsNode(id)) || (pending && pending->holdsNode(id));
        if (!held) pruned.push_back(id);
    }
    std::set<int32_t> prunedSet(pruned.begin(), pruned.end());
    for (int32_t id : pruned) {
        Node& n = nodes.at(id);
        for (auto& inlet : n.inlets) {
            auto c = nodes.find(inlet.source);
            if (c == nodes.end() || prunedSet.count(inlet.source)) continue;
            auto& o = c->second.outlets;
            o.erase(std::remove_if(o.begin(), o.end(), [&](const Outlet& x) { return x.dest == id; }), o.end());
        }
    }
    for (int32_t id : pruned) {
        Node& n = nodes.at(id);
        // (`mu` free does NOT mean the device is idle: elemhip_process_blocks_host drops it between launch sets while one renders.
        //  Device memory is released after the next synchronize — freeDeferred — never under a kernel that may still read it.)
        if (n.ring.ptr) { if (dry) std::free(n.ring.ptr); else deferredFree.push_back(n.ring.ptr); }
        if (n.hostInst && n.hostVt && n.hostVt->destroy) n.hostVt->destroy(n.hostInst, n.hostVt->user);
        recClones.erase(std::remove_if(recClones.begin(), recClones.end(), [&](const std::pair<uint32_t, uint32_t>& c) { return c.first == n.rec; }), recClones.end());
        freeRec(n.rec);
        for (uint32_t cr : n.chanRecs) freeRec(cr);
        if (n.op == OP_TAPIN || n.op == OP_TAPOUT) tapNodeIds.erase(std::remove(tapNodeIds.begin(), tapNodeIds.end(), id), tapNodeIds.end());
        convStaleNodes.erase(id);
        nodes.erase(id);
    }
    if (!pruned.empty()) { if (++nodesEpoch == 0u) nodesEpoch = 1u; }      // (Inlet::src memos name erased nodes now)
    std::sort(pruned.begin(), pruned.end());
    size_t k = 0;
    for (int32_t id : pruned) { if (out && k < cap) out[k] = id; ++k; }
    lastPruned.swap(pruned);
    return k;
}

size_t Engine::lastGc(int32_t* out, size_t cap) {
    std::lock_guard<std::mutex> control(ctl);
    RenderGuard lock(*this);
    size_t k = 0;
    for (int32_t id : lastPruned) { if (out && k < cap) out[k] = id; ++k; }
    return k;
}

bool Engine::hasNode(int32_t id) {
    std::lock_guard<std::mutex> control(ctl);
    RenderGuard lock(*this);
    return nodes.find(id) != nodes.end();
}

// Runtime::reset (Runtime.h:448-458) forwards to every node; of the built-ins only SampleNode reacts: both readers get
// noteOff(), i.e. target gain 0 (Sample.h:78-81, 174-177). The reader state lives in the node record.
void Engine::reset() {
    std::lock_guard<std::mutex> control(ctl);
    RenderGuard lock(*this);
    for (auto& kv : nodes) {
        Node& n = kv.second;
        if (n.op == OP_SAMPLE) {
            writeParamF(n, rec::SMP_READER0, 0.0f);
            writeParamF(n, rec::SMP_READER0 + rec::SMP_READER_DWORDS, 0.0f);
        } else if (n.op == OP_MCSAMPLE) {
            writeParam(n, rec::MCS_RESET, 1u);          // both readers noteOff() at the next block (mc/Sample.h:78-81)
        } else if (n.op == OP_HOST && n.hostVt && n.hostVt->reset) {
            n.hostVt->reset(n.hostInst, n.hostVt->user);
        }
    }
}

static std::string idToHex(int32_t id) {   // Types.h:16-27
    char b[16]; std::snprintf(b, sizeof b, "%08x", (uint32_t)id);
    return b;
}

std::string Engine::snapshotJson() {   // Runtime.h:489-498: { nodeIdToHex(id): node.getProperties() }
    std::lock_guard<std::mutex> control(ctl);
    RenderGuard lock(*this);
    std::map<std::string, const Node*> sorted;
    for (auto& kv : nodes) sorted.emplace(idToHex(kv.first), &kv.second);
    std::string out = "{";
    bool first = true;
    for (auto& kv : sorted) {
        if (!first) out += ',';
        first = false;
        out += '"' + kv.first + "\":{";
        bool f2 = true;
        for (auto& pr : kv.second->props) {
            if (!f2) out += ',';
            f2 = false;
            toJson(Value::string(pr.first), out); out += ':'; toJson(pr.second, out);
        }
        out += '}';
    }
    out += '}';
    return out;
}

std::string Engine::sharedResourceKeysJson() {   // SharedResourceMap::keys (SharedResource.h)
    std::lock_guard<std::mutex> control(ctl);
    RenderGuard lock(*this);
    std::vector<std::string> keys;
    for (auto& kv : resources) keys.push_back(kv.first);
    std::sort(keys.begin(), keys.end());
    std::string out = "[";
    for (size_t i = 0; i < keys.size(); ++i) { if (i) out += ','; toJson(Value::string(keys[i]), out); }
    out += ']';
    return out;
}

bool Engine::addSharedResource(const std::string& name, const float* const* ch, size_t nCh, size_t nSamples) {
    std::lock_guard<std::mutex> control(ctl);
    RenderGuard lock(*this);
    if (resources.count(name)) return false;                 // insert-only (SharedResource.h:61-63)
    auto r = std::make_shared<Resource>();
    for (size_t c = 0; c < nCh; ++c) r->channels.emplace_back(ch[c], ch[c] + nSamples);
    resources.emplace(name, r);
    return true;
}

void Engine::pruneSharedResources() {   // SharedResource.h:94-102
    std::lock_guard<std::mutex> control(ctl);
    RenderGuard lock(*this);
    if (!dry) (void)hipSetDevice(device);
    for (auto it = resources.begin(); it != resources.end();) {
        if (it->second.use_count() == 1) {
            if (it->second->dev.ptr) { if (dry) std::free(it->second->dev.ptr); else deferredFree.push_back(it->second->dev.ptr); }
            for (DevBuf& d : it->second->devCh) if (d.ptr) { if (dry) std::free(d.ptr); else deferredFree.push_back(d.ptr); }
            it->second->dev.ptr = nullptr;
            for (DevBuf& d : it->second->devCh) d.ptr = nullptr;
            it->second->onDevice = false;
            it = resources.erase(it);
        } else ++it;
    }
}

int Engine::setOption(const std::string& key, double value) {
    std::lock_guard<std::mutex> control(ctl);
    RenderGuard lock(*this);
    if (key == "use_graph") { useGraph = value != 0.0; return kOk; }
    if (key == "sync_poll") { syncPoll = value != 0.0; return kOk; }   // elemhip_process: wait for the epilogue's word in mapped host memory (1) or synchronise the stream (0)
    // elemhip_process through a kernel that stays on the GPU between calls (resident.hip): opt-in, the GPU spins while the host is away
    if (key == "resident") { residentOpt = value != 0.0; residentStreak = 0; return kOk; }
    if (key == "resident_idle_us") { residentIdleUs = (uint32_t)std::max(10.0, std::min(5e6, value)); return kOk; }
    if (key == "resident_after") { residentAfter = (uint32_t)std::max(1.0, std::min(1e6, value)); return kOk; }
    if (key == "host_out_direct") { hostOutDirect = value != 0; return kOk; }   // elemhip_process: epilogue writes the pinned host block itself
    if (key == "conv_direct_io") { convDirectIo = value != 0; return kOk; }
    if (key == "conv_long") { convLong = value != 0; return kOk; }   // IRs set from now on get (or do not get) long-partition spectra; sets of older IRs keep theirs
    if (key == "conv_mfma") { convMfma = std::max(0, std::min(1, (int)value)); return kOk; }   // partition MAC of launch sets: 1 matrix cores (default), 0 packed vector FMAs
    if (key == "skip_idle_launches") { skipIdleLaunches = value != 0; dropGraphs(); return kOk; }
    if (key == "spec_blocks") { specBlocks = value != 0; return kOk; }      // elemhip_process through the specialised kernels when it can
    // relay window (host blocks) the device rings of scope / fft nodes made FROM NOW ON keep: their blockwise relay stays exact over that
    // many blocks, ring overruns included (0: the reference's 8192 frames, windows as short as one block). Older nodes keep their ring.
    if (key == "event_history_blocks") { eventHistoryBlocks = (uint32_t)std::max(0, std::min((int)kEventLogEntries, (int)value)); return kOk; }
    // the same for capture / mc.capture nodes made FROM NOW ON: a ring that keeps that many blocks of takes and a per-block log of what a
    // relay after every block would have seen (capture_replay.h). 0: the reference's bitceil(sr) frames and a relay window of one block.
    if (key == "capture_history_blocks") { captureHistoryBlocks = (uint32_t)std::max(0, std::min((int)kEventLogEntries, (int)value)); return kOk; }
    // loudness.h: BS.1770 sub-block mean squares and true peak of every launch set of the host-buffer render calls, on the GPU. Turning
    // it on resets the meter; off (the default) not one launch or byte differs.
    if (key == "loudness_meter") {
        const bool on = value != 0.0;
        if (on && !dry) { loudness::make_plan(deliveryRate(), loudPlan); const int rc = loudnessResetLocked(0); if (rc != kOk) return rc; }      // (it meters what is delivered)
        loudnessOn = on;
        return kOk;
    }
    // resample.h: the host-buffer render calls deliver at this rate (Hz, integral like the engine's; 0 or the engine's rate: off),
    // converted on the GPU behind every launch set. Setting it starts a new programme — the meter's too, at the delivery rate.
    if (key == "resample_rate") return setResampleRate(value);
    // resample.h, the input side: the host-buffer render calls take their inputs at this rate (Hz, integral; 0 or the engine's rate: off),
    // converted to the engine's on the GPU in front of every launch set. Setting it starts a new input programme; nothing else changes.
    if (key == "input_rate") return setInputRate(value);
    // limiter.h: a static gain and a look-ahead true-peak limiter on what those calls deliver, behind the converter. Turning it on, or
    // changing a parameter while it is on, starts a new programme; off (the default) not one launch, allocation or byte differs.
    if (key.compare(0, 7, "limiter") == 0) return setLimiterOption(key, value);
    // flac_encode.h: the block size (256, 512, 1024, 2048, 4096) and the sample size (16, 24) of FLAC delivery. A programme keeps the
    // values it started with: while one is open another value is refused (flacReset first). No other call is touched.
    // flac_lpc.h: the LPC order P (0 .. 12; 0, the default: none — not one byte, launch or allocation differs). The programme keeps it too.
    if (key == "flac_lpc_order") {
        if (!(value >= 0.0) || value > (double)flac_encode::kLpcMaxOrder || value != std::floor(value)) return kInvalidPropertyValue;
        if (flacStreams != 0u && (uint32_t)value != flacLpc) return kInvalidPropertyValue;
        flacLpcOpt = (uint32_t)value;
        return kOk;
    }
    // flac_md5.h: 1 — every stream of a FLAC programme carries its STREAMINFO MD5 on the device; 0, the default: not one launch, allocation
    // or byte differs. The programme keeps the value it started with.
    if (key == "flac_md5") {
        if (value != 0.0 && value != 1.0) return kInvalidPropertyValue;
        if (flacStreams != 0u && (uint32_t)value != flacMd5) return kInvalidPropertyValue;
        flacMd5Opt = (uint32_t)value;
        return kOk;
    }
    // flac_in_md5.h: 1 — the samples decoded from FLAC inputs and FLAC resources enter their stream's STREAMINFO MD5 on the device; 0, the
    // default: not one launch, allocation or byte differs. Another value than the option has resets the input slots.
    if (key == "flac_in_md5") {
        if (value != 0.0 && value != 1.0) return kInvalidPropertyValue;
        if ((uint32_t)value != flacInMd5Opt) { const int rc = flacInMd5ResetLocked(); if (rc != kOk) return rc; }
        flacInMd5Opt = (uint32_t)value;
        return kOk;
    }
    if (key == "flac_frame" || key == "flac_bits") {
        const bool frame = key == "flac_frame";
        const uint32_t v = value >= 0.0 && value <= 65536.0 && value == std::floor(value) ? (uint32_t)value : 0u;
        if (frame ? !flac_encode::frame_ok(v) : !flac_encode::bits_ok(v)) return kInvalidPropertyValue;
        if (frame && flacStreams != 0u && v != flacFF) return kInvalidPropertyValue;
        (frame ? flacFrameOpt : flacBitsOpt) = v;
        return kOk;
    }
    // resource_load.h: source frames per staged piece of addSharedResourcePcm (64 .. 2^24, default 2^20). The resource's bits do not depend on it.
    if (key == "resource_load_frames") {
        if (!(value >= (double)resource_load::kMinPiece) || value > (double)resource_load::kMaxPiece || value != std::floor(value)) return kInvalidPropertyValue;
        resourceLoadFramesOpt = (uint32_t)value;
        return kOk;
    }
    if (key == "batch_blocks") { batchBlocks = std::max(1, std::min(1024, (int)value)); return kOk; }      // blocks per multi-block launch (1 = off)
    if (key == "debug_build_delay_ms") { debugBuildDelayMs = std::max(0, (int)value); return kOk; }   // tests: stretches the unlocked part of a plan build
    if (key == "plan_cache") { planCache = std::max(0, std::min(2, (int)value)); islandCache.clear(); islandShapeCache.clear(); return kOk; }
    if (key == "plan_relocate") { relocatePrograms = value != 0; islandShapeCache.clear(); return kOk; }   // programs of structural twins renamed instead of scheduled again
    if (key == "fuse_svf_coef") { fuseSvfCoef = (uint32_t)std::max(0, std::min(2, (int)value)); planStale = true; return kOk; }
    if (key == "mixer_split") { const int v = (int)value; mixerSplit = (v == 2 || v == 4 || v == 8) ? (uint32_t)v : 1u; planStale = true; return kOk; }
    if (key == "stateless_rows") { statelessRows = (uint32_t)std::max(1, std::min(64, (int)value)); return kOk; }   // gridDim.y of a multi-block launch: blocks that stateless islands render side by side
    if (key == "pipeline_copies") { pipelineCopies = std::max(1, std::min(6, (int)value)); planStale = true; return kOk; }   // next commit re-plans
    if (key == "pack_islands") { packIslands = std::max(0, std::min(16, (int)value)); planStale = true; return kOk; }   // next commit re-plans
    if (key == "prog_heap_dwords") { progHeapCap = (size_t)std::max(0.0, value); progHeap.reset(); islandCache.clear(); planStale = true; return kOk; }   // 0: sized by the engine
    if (key == "pack_roots") { packRoots = value != 0; planStale = true; return kOk; }   // islands of different active roots may share a workgroup (C4: a root per render job)
    if (key == "pack_max") { packMax = std::max(1, std::min(16, (int)value)); planStale = true; return kOk; }
    if (key == "cu_count") { cuCount = std::max(1, (int)value); planStale = true; return kOk; }      // (dry handles / tests: the CU count the auto mode plans for)
    if (key == "merge_phases") { mergePhases = value != 0.0; planStale = true; return kOk; }   // next commit re-plans
    if (key == "specialize") { specialize = std::max(0, std::min(2, (int)value)); planStale = true; return kOk; }   // next commit re-plans
    if (key == "profile_launches") {
        // 1: a HIP event pair around every launch of every launch set; N > 1: around those of every N-th set only (r06: an event record
        // costs ~4 us of stream time — 8.5 of an 80 us C3 set; the per-set mean is over the sampled sets, still inside the timed region)
        profileLaunches = value != 0.0;
        profileEvery = (uint32_t)std::max(1.0, std::min(1024.0, value));
        if (profileLaunches) { profMs.clear(); profSets = 0; profBlocks = 0; profSetCounter = 0; }
        return kOk;
    }
    if (key == "max_shape_launches") { maxShapeLaunches = std::max(1, std::min(64, (int)value)); dropGraphs(); return kOk; }
    if (key == "spec_lonely_blocks") { lonelyBlocks = std::max(0, (int)value); return kOk; }   // background mode: a one-off shape is queued for compilation once its
    if (key == "spec_lonely_ms") { lonelyMs = std::max(0, (int)value); return kOk; }           // plan has rendered this many blocks and been current this long
    if (key == "jit_cache_entries") { Jit::get().setEntryCap((uint32_t)std::max(0.0, value)); return kOk; }   // PROCESS-wide: compiled shapes kept in memory (0: default 256)
    if (key == "time_batch") { timeBatch = std::max(1, std::min(256, (int)value)); return kOk; }
    if (key == "graph_blocks") { graphBlocks = std::max(1, (int)value); dropGraphs(); return kOk; }
    return kInvalidPropertyValue;
}

} // namespace elemhip
