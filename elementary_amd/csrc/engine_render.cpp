// engine_render.cpp — the per-block launch sequence (process), launch sets (processBlocks / processBlocksHost), the resident
// kernel's host side and the measurement calls. Everything a render call reaches lives in this unit or inline in engine.h, but for the
// block-by-block host render (engine_host_blocks.cpp).
#include "engine_impl.h"
#include "flac_encode.h"
#include <functional>
#include <thread>

namespace elemhip {

// ---- block rendering ----------------------------------------------------------------------------------
void Engine::dropGraphs() {
    if (!current) return;
    if (current->graphExec) { (void)hipGraphExecDestroy(current->graphExec); current->graphExec = nullptr; }
}

void Engine::freeDeferred() {   // called right after a synchronize of every stream the engine renders on (`mu` held)
    patchCursor = 0;
    for (void* p : deferredFree) (void)hipFree(p);
    deferredFree.clear();
    retiredPlans.clear();         // plans replaced since the last synchronize: their tables / hipGraphs are idle now (~Plan frees them)
}

int Engine::ensureHbm(size_t buffers) {
    if (buffers <= hbmBuffers) return kOk;
    size_t want = std::max(buffers, hbmBuffers * 2);
    float* nb = nullptr;
    // + slack: vector loads of a 64*V-frame task may read (never write) past a short block's buffer
    const size_t floats = want * blockSize + 1024;
    HIP_OK(hipMalloc(&nb, floats * sizeof(float)));
    HIP_OK(hipMemsetAsync(nb, 0, floats * sizeof(float), stream));   // ordered with the kernels: they run on `stream` (non-blocking w.r.t. the null stream)
    if (dHbm) deferredFree.push_back(dHbm);
    dHbm = nb; hbmBuffers = want;
    dropGraphs();
    return kOk;
}

// Arena buffers a launch set of `blocks` blocks of plan `p` needs: one slice (host inputs + exports) per block, then the
// stream ring of the specialised kernels, one slice per buffer set an island may keep in flight.
size_t Engine::arenaBuffers(const Plan& p, size_t blocks) const {
    return (size_t)p.numHbmBuffers * blocks + (size_t)p.numStreamBuffers * (size_t)p.maxCopies;
}
// The recurrence loops of the specialised kernels address the whole arena through 32-bit buffer offsets with the top bit
// reserved as "out of range": a launch set stays under 2 GB of arena (C2: 0.6 MB per block).
size_t Engine::maxSetBlocks(const Plan& p) const {
    const size_t cap = ((size_t)1 << 29) / (size_t)blockSize;                       // buffers of blockSize floats in 2 GB
    const size_t ring = (size_t)p.numStreamBuffers * p.maxCopies + 2;
    return cap > ring ? std::max<size_t>(1, (cap - ring) / std::max<uint32_t>(1u, p.numHbmBuffers)) : 1;
}

int Engine::ensureOutRing(size_t floats) {
    if (floats <= outRingFloats) return kOk;
    float* nb = nullptr;
    HIP_OK(hipMalloc(&nb, floats * sizeof(float)));
    HIP_OK(hipMemsetAsync(nb, 0, floats * sizeof(float), stream));
    if (dOutRing) deferredFree.push_back(dOutRing);
    dOutRing = nb; outRingFloats = floats;
    dropGraphs();
    return kOk;
}

int Engine::flushPending() {
    residentStop();
    if (nextRec > recCapacity) {   // grow the record arena (device idle: we hold `mu` and sync every call)
        uint32_t cap = recCapacity;
        while (cap < nextRec) cap *= 2;
        uint32_t* nr = nullptr;
        HIP_OK(hipStreamSynchronize(stream));
        HIP_OK(hipMalloc(&nr, (size_t)cap * kRecDwords * 4));
        HIP_OK(hipMemsetAsync(nr, 0, (size_t)cap * kRecDwords * 4, stream));
        HIP_OK(hipMemcpyAsync(nr, dRecs, (size_t)recCapacity * kRecDwords * 4, hipMemcpyDeviceToDevice, stream));
        HIP_OK(hipStreamSynchronize(stream));
        (void)hipFree(dRecs);
        dRecs = nr; recCapacity = cap;
        dropGraphs();
    }
    if (!freshRecs.empty()) {
        std::sort(freshRecs.begin(), freshRecs.end());
        size_t i = 0;
        while (i < freshRecs.size()) {
            size_t j = i + 1;
            while (j < freshRecs.size() && freshRecs[j] == freshRecs[j - 1] + 1) ++j;
            const uint32_t first = freshRecs[i];
            const size_t count = j - i;
            // through the pinned staging area the patches use (`shadow` is pageable and changes under the copy otherwise): a new
            // voice's records reach the device without waiting for the blocks that are still rendering
            constexpr size_t slotsPerRec = (kRecDwords * 4 + sizeof(Patch) - 1) / sizeof(Patch);
            size_t done = 0;
            while (done < count) {
                if (patchCursor + slotsPerRec > patchCap) { HIP_WARN(hipStreamSynchronize(stream)); patchCursor = 0; }
                const size_t fit = std::min(count - done, (patchCap - patchCursor) / slotsPerRec);
                std::memcpy(hPatches + patchCursor, shadow.data() + ((size_t)first + done) * kRecDwords, fit * kRecDwords * 4);
                HIP_WARN(hipMemcpyAsync(dRecs + ((size_t)first + done) * kRecDwords, hPatches + patchCursor, fit * kRecDwords * 4, hipMemcpyHostToDevice, stream));
                patchCursor += fit * slotsPerRec;
                done += fit;
            }
            i = j;
        }
        for (uint32_t r : freshRecs) freshFlag[r] = 0;
        freshRecs.clear();
    }
    if (deviceClockBehind && !nextSetDirect) {      // (enqueueBatch: direct-I/O convolver sets leave the device's sample clock to be caught up here)
        const uint64_t t = (uint64_t)hGlobals.sampleTime;
        patches.push_back(Patch{2u, (uint32_t)(offsetof(Globals, sampleTime) / 4), (uint32_t)(t & 0xFFFFFFFFu), 0u});
        patches.push_back(Patch{2u, (uint32_t)(offsetof(Globals, sampleTime) / 4 + 1), (uint32_t)(t >> 32), 0u});
        deviceClockBehind = false;
    }
    size_t off = 0;
    while (off < patches.size()) {
        // the patch kernel reads the pinned staging area when it RUNS: hand every launch its own
        // stretch of it and only rewind once the stream has drained
        if (patchCursor >= patchCap) { HIP_WARN(hipStreamSynchronize(stream)); patchCursor = 0; }
        const size_t cnt = std::min<size_t>(patchCap - patchCursor, patches.size() - off);
        std::memcpy(hPatches + patchCursor, patches.data() + off, cnt * sizeof(Patch));
        launch_patches(stream, hPatches + patchCursor, (uint32_t)cnt, dRecs, reinterpret_cast<uint32_t*>(dGlobals));
        debugSync("patches", (unsigned)cnt);
        patchCursor += cnt;
        off += cnt;
    }
    patches.clear();
    // new channel records of multi-output nodes that are already rendering: everything but the buffer slots, AFTER the
    // patches (a pending-buffer flag the host has just queued for channel 0 reaches the new channel with this copy)
    for (auto& cl : recClones)
        HIP_WARN(hipMemcpyAsync(dRecs + (size_t)cl.second * kRecDwords + rec::P3, dRecs + (size_t)cl.first * kRecDwords + rec::P3,
                                (kRecDwords - rec::P3) * 4, hipMemcpyDeviceToDevice, stream));
    recClones.clear();
    return kOk;
}

int Engine::setGlobalsFor(size_t nIn, size_t nOut, size_t n, int64_t sampleTime) {
    auto patchG = [&](size_t byteOff, uint32_t v) { patches.push_back(Patch{2u, (uint32_t)(byteOff / 4), v, 0u}); };
    if (hGlobals.numSamples != (uint32_t)n) { hGlobals.numSamples = (uint32_t)n; patchG(offsetof(Globals, numSamples), (uint32_t)n); }
    if (hGlobals.numIn != (uint32_t)nIn) { hGlobals.numIn = (uint32_t)nIn; patchG(offsetof(Globals, numIn), (uint32_t)nIn); }
    if (hGlobals.numOut != (uint32_t)nOut) { hGlobals.numOut = (uint32_t)nOut; patchG(offsetof(Globals, numOut), (uint32_t)nOut); }
    if (hGlobals.sampleTime != sampleTime) {
        hGlobals.sampleTime = sampleTime;
        patchG(offsetof(Globals, sampleTime), (uint32_t)((uint64_t)sampleTime & 0xFFFFFFFFu));
        patchG(offsetof(Globals, sampleTime) + 4, (uint32_t)((uint64_t)sampleTime >> 32));
    }
    return kOk;
}

void Engine::setInRing(const float* ring, uint32_t blocks) {
    const uint64_t v = (uint64_t)(uintptr_t)ring;
    if (hGlobals.inRing != v) {
        hGlobals.inRing = v;
        patches.push_back(Patch{2u, (uint32_t)(offsetof(Globals, inRing) / 4), (uint32_t)(v & 0xFFFFFFFFu), 0u});
        patches.push_back(Patch{2u, (uint32_t)(offsetof(Globals, inRing) / 4 + 1), (uint32_t)(v >> 32), 0u});
    }
    if (hGlobals.inBlocks != blocks) {
        hGlobals.inBlocks = blocks;
        patches.push_back(Patch{2u, (uint32_t)(offsetof(Globals, inBlocks) / 4), blocks, 0u});
    }
}

int Engine::swapInPending() {   // Runtime.h:277-285: newest sequence wins
    if (pending) {
        if (current && !dry) retiredPlans.push_back(std::move(current));   // its kernels may still be queued (host path): freed after the next synchronize
        current = pending;
        pending.reset();
        current->blocksAtAdoption = st.blocksRendered;
        current->adopted = std::chrono::steady_clock::now();
        st.numIslands = (uint32_t)current->islands.size();
        st.numLevels = (uint32_t)current->levelOffsets.size() - 1;
        st.numTasks = current->numTasks;
        st.numNodesInPlan = (uint32_t)current->nodeIds.size();
        st.maxLdsBytes = current->maxLdsBytes;
        st.numHbmBuffers = current->numHbmBuffers;
    }
    if (!current) return kOk;
    int rc = ensureHbm(arenaBuffers(*current, 1));
    if (rc != kOk) return rc;
    if (current->maxLdsBytes > maxLdsConfigured) {
        HIP_OK(configure_kernels(current->maxLdsBytes));
        maxLdsConfigured = current->maxLdsBytes;
    }
    return kOk;
}

void Engine::enqueueBlock(const Plan& p, float* outRing) {
    if (!outRing) outRing = dOutRing;
    const size_t L = p.levelOffsets.size() - 1;
    for (size_t l = 0; l < L; ++l) {
        const uint32_t b = p.levelOffsets[l], e = p.levelOffsets[l + 1];
        if (e > b) { launch_level(stream, p.view, dRecs, dHbm, dGlobals, dLcg, b, e - b, p.levelLdsBytes[l]); islandBlocksInterp += e - b; }
        debugSync("block: interpreter level", (unsigned)l, e - b);
        const uint32_t cb = p.convLevelOffsets[l], ce = p.convLevelOffsets[l + 1];
        if (ce > cb) launch_convolve(stream, p.view, dRecs, dHbm, dGlobals, cb, ce - cb);
        if (!p.hosts.empty()) (void)renderHostNodes(p, l);
    }
    launch_epilogue(stream, p.view, dRecs, dHbm, dGlobals, outRing, armFlag, armValue);
    if (armFlag) flagArmed = true;
    debugSync("block: epilogue");
}

// Call-out nodes of launch level `l` (GraphNode::process on the CPU, GraphNode.h:72): drain the stream, bring each node's
// input buffers to the host, run the user's process(), put its output block back into the arena. Slow by construction
// (two PCIe round trips and a pipeline drain per node and block) — the price of keeping custom CPU nodes usable.
int Engine::renderHostNodes(const Plan& p, size_t l) {
    bool any = false;
    for (const Plan::HostDesc& h : p.hosts) if (h.level == (uint32_t)l) { any = true; break; }
    if (!any) return kOk;
    HIP_OK(hipStreamSynchronize(stream));
    const size_t bs = (size_t)blockSize, n = hGlobals.numSamples, nInHost = hGlobals.numIn;
    for (const Plan::HostDesc& h : p.hosts) {
        if (h.level != (uint32_t)l) continue;
        auto nit = nodes.find(h.nodeId), rit = nodes.find(h.rootId);
        if (nit == nodes.end() || rit == nodes.end() || !nit->second.hostVt) continue;
        const Node& r = rit->second;
        const bool on = r.target > 0.5f, settled = std::fabs(r.target - r.gain) <= 1e-6f;
        if (!((on || !settled) && r.channel >= 0 && (uint32_t)r.channel < hGlobals.numOut)) continue;   // GraphRenderSequence.h:214-219
        const size_t k = h.leaf ? nInHost : h.inputs.size();
        hostIn.assign(std::max<size_t>(k, 1) * bs, 0.0f);
        hostOut.assign(bs, 0.0f);
        for (size_t j = 0; j < k; ++j) {
            float* dst = hostIn.data() + j * bs;
            if (h.leaf) { HIP_OK(hipMemcpyAsync(dst, dHbm + j * bs, n * sizeof(float), hipMemcpyDeviceToHost, stream)); continue; }
            const Plan::HostDesc::In& in = h.inputs[j];
            if (in.kind == 1) HIP_OK(hipMemcpyAsync(dst, dHbm + (size_t)in.idx * bs, n * sizeof(float), hipMemcpyDeviceToHost, stream));
            else if (in.kind == 2) { float v; std::memcpy(&v, &shadow[(size_t)in.idx * kRecDwords + rec::P0], 4); std::fill(dst, dst + n, v); }
            else if (in.kind == 3) {
                const uint32_t ch = shadow[(size_t)in.idx * kRecDwords + rec::P0];
                if (ch < nInHost) HIP_OK(hipMemcpyAsync(dst, dHbm + (size_t)ch * bs, n * sizeof(float), hipMemcpyDeviceToHost, stream));
            }
        }
        HIP_OK(hipStreamSynchronize(stream));
        std::vector<const float*> ptrs(std::max<size_t>(k, 1));
        for (size_t j = 0; j < k; ++j) ptrs[j] = hostIn.data() + j * bs;
        const Node& hn = nit->second;
        hn.hostVt->process(hn.hostInst, ptrs.data(), k, hostOut.data(), n, curBlockTime, h.active ? 1 : 0, hn.hostVt->user);
        HIP_OK(hipMemcpyAsync(dHbm + (size_t)h.outHbm * bs, hostOut.data(), n * sizeof(float), hipMemcpyHostToDevice, stream));
        HIP_OK(hipStreamSynchronize(stream));
    }
    return kOk;
}

// Host mirror of what the epilogue kernel does to each root's fade (GainFade.h:56-72), so that
// activateRoots()/gc() can evaluate stillRunning() without a device read-back.
void Engine::mirrorRootFades(const Plan& p, uint32_t n, uint32_t nOut, uint32_t nIn) {
    for (int32_t id : p.rootIds) {
        auto it = nodes.find(id);
        if (it == nodes.end()) continue;
        Node& r = it->second;
        const bool on = r.target > 0.5f;
        const bool settled = std::fabs(r.target - r.gain) <= 1e-6f;
        if (!((on || !settled) && r.channel >= 0 && (uint32_t)r.channel < nOut)) continue;
        if (r.gain != r.target && (!r.inlets.empty() || nIn > 0))
            r.gain = clampf(r.gain + r.step * (float)(int)n, 0.0f, 1.0f);
    }
}

// A host block longer than the engine's: slice `off / blockSize` of it renders the frames [off, off + blockSize) — and a tap's delay
// is the HOST's block (TapOutNode::promoteTapBuffers copies numSamples frames of its delay buffer to the shared one, TapInNode copies
// numSamples frames back out: Feedback.h:88-109, 40-54), so the slice reads and promotes ITS stretch of the shared buffers: the tap
// records' shared-buffer pointers move with the slice (parameter patches, applied in front of the slice's kernels).
void Engine::setTapSlice(size_t off) {
    if (off == tapSliceOff) return;
    tapSliceOff = off;
    if (dry) return;
    for (int32_t id : tapNodeIds) {
        auto it = nodes.find(id);
        if (it == nodes.end() || !it->second.res || !it->second.res->dev.ptr) continue;
        writeParamPtr(it->second, rec::TAP_SHARED, reinterpret_cast<const float*>(it->second.res->dev.ptr) + off);
    }
}

int Engine::process(const float* const* in, size_t nIn, float* const* out, size_t nOut, size_t n, int64_t sampleTime) {
    if (hostBlockSize == blockSize) return processSlice(in, nIn, out, nOut, n, sampleTime);
    if (n > (size_t)hostBlockSize) return kBlockTooLarge;
    if (nIn > kMaxHostIn || nOut > kMaxOutBus) return kTooManyChannels;
    // a host block longer than the engine's: slice by slice (each slice is a block of its own to the kernels), the render lock held
    // and the newest sequence adopted ONCE for the whole host block — a commit, gc or event relay from another thread lands between
    // two host blocks, never inside one
    std::vector<const float*> ip(nIn);
    std::vector<float*> op(nOut);
    std::lock_guard<std::mutex> lock(mu);
    for (size_t off = 0; off < n || off == 0; off += (size_t)blockSize) {
        for (size_t c = 0; c < nIn; ++c) ip[c] = in[c] + off;
        for (size_t c = 0; c < nOut; ++c) op[c] = out[c] + off;
        if (!tapNodeIds.empty()) setTapSlice(off);
        const int rc = processSliceLocked(ip.data(), nIn, op.data(), nOut, std::min((size_t)blockSize, n - off), sampleTime + (int64_t)off, off == 0);
        if (rc != kOk) return rc;
    }
    noteHostBlockEnd();
    return kOk;
}

int Engine::processSlice(const float* const* in, size_t nIn, float* const* out, size_t nOut, size_t n, int64_t sampleTime) {
    std::lock_guard<std::mutex> lock(mu);
    return processSliceLocked(in, nIn, out, nOut, n, sampleTime, true);
}

// (`mu` held.) `adopt`: take the newest render sequence — once per HOST block (Runtime.h:277-285): the later slices of a host block
// longer than the engine's render the sequence its first slice adopted, under the same hold of the lock.
int Engine::processSliceLocked(const float* const* in, size_t nIn, float* const* out, size_t nOut, size_t n, int64_t sampleTime, bool adopt) {
    if (dry) return kNoDevice;
    if (hipSetDevice(device) != hipSuccess) return kHipError;
    if (n > (size_t)blockSize) return kBlockTooLarge;
    if (nIn > kMaxHostIn || nOut > kMaxOutBus) return kTooManyChannels;
    if (n != conv::kBlock) convAligned = false;   // a convolver's input block may now be partly filled at a call boundary
    if (residentLive && (pending || !residentOpt)) residentStop();
    int rc = adopt ? swapInPending() : kOk;
    if (rc != kOk) return rc;
    if (!current) return kOk;   // no render sequence yet: outputs untouched (Runtime.h:287-289)
    Plan& p = *current;
    if (p.packedRootChannels > 0 && nOut < (size_t)p.packedRootChannels) return kInvalidPropertyValue;   // (`pack_roots`, plan.cpp)

    if (hGlobals.ringSlots != 1 || hGlobals.blockSlot != 0) {
        hGlobals.ringSlots = 1; hGlobals.blockSlot = 0;
        patches.push_back(Patch{2u, (uint32_t)(offsetof(Globals, ringSlots) / 4), 1u, 0u});
        patches.push_back(Patch{2u, (uint32_t)(offsetof(Globals, blockSlot) / 4), 0u, 0u});
    }
    setGlobalsFor(nIn, nOut, n, sampleTime);
    setInRing(nullptr, 0);
    rc = ensureOutRing(std::max<size_t>(nOut, 1) * blockSize);
    if (rc != kOk) return rc;
    // option "resident": a run of plain blocks (nothing to flush, every fade settled, the same plan and channel counts) is handed
    // to the resident kernel through mapped host memory — no launch, no stream synchronise
    {
        const bool plain = residentOpt && n == (size_t)blockSize && residentEligible(p, nIn, nOut);
        if (residentLive && (!plain || residentPlan != &p || residentNIn != nIn || residentNOut != nOut)) residentStop();
        if (!plain) residentStreak = 0;
        else if (!residentLive && ++residentStreak > residentAfter) {
            rc = residentStart(p, nIn, nOut);
            if (rc != kOk) return rc;
        }
        if (residentLive) {
            rc = residentBlock(in, nIn, out, nOut, n);
            if (rc != kResidentGone) return rc;
        }
    }
    // A whole block of a settled sequence whose island shapes are all compiled goes through the specialised kernels as a
    // launch set of one (stages pipelined inside the workgroup, no interpreter image); everything else block by block.
    const bool specLevels = n == (size_t)blockSize && specBlockOk(p);
    const bool specBlock = specLevels && batchEligible(p, nOut, true);
    const bool specFade = specLevels && !specBlock;      // root fades running: same level launches, the per-block epilogue behind them
    if (specLevels) {
        rc = ensureHbm(arenaBuffers(p, 1));
        if (rc != kOk) return rc;
    }

    if (nIn > 0) {
        const size_t floats = nIn * (size_t)blockSize;
        if (floats > hInFloats) {
            if (hIn) (void)hipHostFree(hIn);
            HIP_OK(hipHostMalloc((void**)&hIn, floats * sizeof(float), hipHostMallocDefault));
            hInFloats = floats;
        }
        for (size_t c = 0; c < nIn; ++c) {
            std::memcpy(hIn + c * blockSize, in[c], n * sizeof(float));
            if (n < (size_t)blockSize) std::memset(hIn + c * blockSize + n, 0, (blockSize - n) * sizeof(float));
        }
        HIP_OK(hipMemcpyAsync(dHbm, hIn, floats * sizeof(float), hipMemcpyHostToDevice, stream));
    }
    rc = flushPending();
    if (rc != kOk) return rc;
    curBlockTime = sampleTime;
    // the epilogue writes the output block straight into the pinned host buffer (mapped into the device's address space): one
    // launch and one PCIe write burst less than rendering into HBM and copying back
    float* outDev = nullptr;
    if (nOut > 0) {
        const size_t floats = std::max<size_t>(nOut, 1) * (size_t)blockSize;
        if (floats > hOutFloats) {
            HIP_OK(hipStreamSynchronize(stream));
            if (hOut) (void)hipHostFree(hOut);
            hOut = nullptr; hOutFloats = 0; hOutDev = nullptr;
            // mapped AND coherent, said out loud: with `sync_poll` the host reads this block when the epilogue's word arrives, before the
            // kernel has ended — no kernel-end release stands behind the samples, only the epilogue's own system-scope fence
            HIP_OK(hipHostMalloc((void**)&hOut, floats * sizeof(float), hipHostMallocMapped | hipHostMallocCoherent));
            hOutFloats = floats;
            if (hipHostGetDevicePointer((void**)&hOutDev, hOut, 0) != hipSuccess) hOutDev = nullptr;
        }
        outDev = hostOutDirect ? hOutDev : nullptr;
    }
    // the call ends when the epilogue's word arrives (sync_poll): only when the epilogue writes the host's block itself and nothing is
    // being profiled
    flagArmed = false; armFlag = nullptr;
    if (syncPoll && outDev && !profileLaunches && !debugSyncOn() && p.hosts.empty()) {
        if (!hDone) {
            HIP_OK(hipHostMalloc((void**)&hDone, 64, hipHostMallocMapped | hipHostMallocCoherent));
            *hDone = 0;
            HIP_OK(hipHostGetDevicePointer((void**)&dDone, hDone, 0));
        }
        armFlag = dDone; armValue = ++doneSeq;
    }
    if (specBlock) enqueueBatch(p, 1u, outDev);
    else if (specFade) enqueueSpecBlock(p, outDev);
    else { fixConvOverlaps(p); enqueueBlock(p, outDev); }
    if (nOut > 0 && !outDev) HIP_OK(hipMemcpyAsync(hOut, dOutRing, nOut * (size_t)blockSize * sizeof(float), hipMemcpyDeviceToHost, stream));
    armFlag = nullptr;
    bool arrived = false;
    if (flagArmed) {
        // spin on the epilogue's word (2 ms at most: a graph that takes longer gains nothing from it; a kernel that faulted never
        // publishes — the synchronise below reports it)
        const uint32_t want = armValue;
        uint32_t spins = 0;
        std::chrono::steady_clock::time_point t0;
        for (;;) {
            if (__atomic_load_n(hDone, __ATOMIC_ACQUIRE) == want) { arrived = true; break; }
            __builtin_ia32_pause();
            if ((++spins & 0x3FFu) == 0u) {
                const auto now = std::chrono::steady_clock::now();
                if (spins == 0x400u) t0 = now;
                else if (now - t0 > std::chrono::milliseconds(2)) break;
            }
        }
        flagArmed = false;
        syncPolls++;
        if (!arrived) syncPollFallbacks++;
    }
    // (every 256th call still synchronises: the runtime retires its launch bookkeeping there; so does a call with plans / buffers
    //  waiting to be released — freeDeferred's contract is a REAL synchronise of the stream, not the polled word)
    bool synced = false;
    if (!arrived || !deferredFree.empty() || !retiredPlans.empty() || (++unsyncedCalls & 255u) == 0u) {
        HIP_OK(hipStreamSynchronize(stream));
        HIP_OK(hipGetLastError());
        synced = true;
    }
    if (profUsed) profCollect();
    for (size_t c = 0; c < nOut; ++c) std::memcpy(out[c], hOut + c * blockSize, n * sizeof(float));
    mirrorRootFades(p, (uint32_t)n, (uint32_t)nOut, (uint32_t)nIn);
    hGlobals.sampleTime += (int64_t)n;
    st.blocksRendered++;
    promoteDeferredShapes();
    // the word arrived: the armed epilogue is the last work of this call on `stream`, which is in order and joined every side stream
    // in front of it — the patch uploads of this call have been consumed, so the staging cursor may start over; nothing is freed
    if (synced) freeDeferred(); else patchCursor = 0;
    return kOk;
}

// ---- option "resident" (resident.hip) -------------------------------------------------------------------------------------------
bool Engine::residentEligible(const Plan& p, size_t nIn, size_t nOut) const {
    if (!p.convs.empty() || !p.hosts.empty() || profileLaunches || debugSyncOn() || hGlobals.trace) return false;
    if (!patches.empty() || !freshRecs.empty() || !recClones.empty() || deviceClockBehind) return false;   // (something flushPending still has to bring to the device)
    if (p.view.numRoots > kResidentMaxRoots || p.levelOffsets.size() < 2 || p.levelOffsets.size() - 1 > kResidentMaxLevels) return false;
    if (p.levelOffsets.back() == 0u) return false;
    return batchEligible(p, nOut, true);      // every running root's fade settled: the epilogue has no per-root state to advance
}

int Engine::residentStart(const Plan& p, size_t nIn, size_t nOut) {
    if (!hResident) {
        HIP_OK(hipHostMalloc((void**)&hResident, sizeof(ResidentCtl), hipHostMallocMapped | hipHostMallocCoherent));
        HIP_OK(hipHostGetDevicePointer((void**)&dResidentCtl, hResident, 0));
        HIP_OK(hipMalloc((void**)&dResidentSync, 64));
    }
    const size_t inF = std::max<size_t>(nIn, 1) * (size_t)blockSize, outF = std::max<size_t>(nOut, 1) * (size_t)blockSize;
    if (inF > resInFloats) {
        if (hResIn) (void)hipHostFree(hResIn);
        hResIn = nullptr; resInFloats = 0;
        HIP_OK(hipHostMalloc((void**)&hResIn, inF * sizeof(float), hipHostMallocMapped | hipHostMallocCoherent));
        HIP_OK(hipHostGetDevicePointer((void**)&dResIn, hResIn, 0));
        resInFloats = inF;
    }
    if (outF > resOutFloats) {
        if (hResOut) (void)hipHostFree(hResOut);
        hResOut = nullptr; resOutFloats = 0;
        HIP_OK(hipHostMalloc((void**)&hResOut, outF * sizeof(float), hipHostMallocMapped | hipHostMallocCoherent));
        HIP_OK(hipHostGetDevicePointer((void**)&dResOut, hResOut, 0));
        resOutFloats = outF;
    }
    ResidentLevels lv{};
    lv.count = (uint32_t)p.levelOffsets.size() - 1;
    uint32_t widest = 1;
    for (uint32_t l = 0; l <= lv.count; ++l) lv.offset[l] = p.levelOffsets[l];
    for (uint32_t l = 0; l < lv.count; ++l) widest = std::max(widest, lv.offset[l + 1] - lv.offset[l]);
    // one workgroup per compute unit at most: every workgroup has to be ON the device for the barriers between the levels to complete
    const uint32_t groups = std::min<uint32_t>(widest, (uint32_t)std::max(1, cuCount));
    if (p.maxLdsBytes > residentLdsConfigured) {
        HIP_OK(configure_resident(p.maxLdsBytes));
        residentLdsConfigured = p.maxLdsBytes;
    }
    std::memset(hResident, 0, sizeof(ResidentCtl));
    HIP_OK(hipMemsetAsync(dResidentSync, 0, 64, stream));
    const uint64_t idleTicks = (uint64_t)residentIdleUs * 100ull, hangTicks = 5ull * 100000000ull;   // s_memrealtime: 100 MHz
    HIP_OK(launch_resident(stream, p.view, dRecs, dHbm, dGlobals, dLcg, lv, groups, std::max<uint32_t>(p.maxLdsBytes, 1024u), dResidentCtl, dResIn, dResOut,
                           dResidentSync, idleTicks, hangTicks));
    residentTicksBody = residentTicksEpilogue = 0;
    residentLive = true; residentSeq = 0; residentPlan = &p; residentNIn = nIn; residentNOut = nOut;
    st.residentLaunches++;
    return kOk;
}

void Engine::residentStop() {
    if (!residentLive) return;
    __atomic_store_n(&hResident->seq, kResidentQuit, __ATOMIC_RELEASE);
    HIP_WARN(hipStreamSynchronize(stream));
    if (__atomic_load_n(&hResident->exited, __ATOMIC_ACQUIRE) == 2u)
        std::fprintf(stderr, "[elemhip] resident kernel: a device-wide barrier timed out; the block it was rendering is lost\n");
    residentLive = false; residentStreak = 0; residentPlan = nullptr;
    static const bool trace = std::getenv("ELEMHIP_RESIDENT_TRACE") != nullptr;
    if (trace && residentSeq)
        std::fprintf(stderr, "[elemhip] resident kernel left after %u blocks: levels %.2f us, epilogue %.2f us per block (device clock, from the block number's arrival)\n",
                     residentSeq, 0.01 * (double)residentTicksBody / residentSeq, 0.01 * (double)residentTicksEpilogue / residentSeq);
}

int Engine::residentBlock(const float* const* in, size_t nIn, float* const* out, size_t nOut, size_t n) {
    for (size_t c = 0; c < nIn; ++c) std::memcpy(hResIn + c * blockSize, in[c], n * sizeof(float));
    const uint32_t seq = ++residentSeq;
    __atomic_store_n(&hResident->seq, seq, __ATOMIC_RELEASE);
    uint32_t spins = 0;
    std::chrono::steady_clock::time_point t0;
    for (;;) {
        if (__atomic_load_n(&hResident->done, __ATOMIC_ACQUIRE) == seq) break;
        if (__atomic_load_n(&hResident->exited, __ATOMIC_ACQUIRE) != 0u) {
            // it left: by itself (idle) before it saw this block, or on a barrier time-out
            const bool rendered = __atomic_load_n(&hResident->done, __ATOMIC_ACQUIRE) == seq;
            const uint32_t code = hResident->exited;
            HIP_WARN(hipStreamSynchronize(stream));
            residentLive = false; residentStreak = 0; residentPlan = nullptr;
            if (rendered) break;
            if (code == 2u) return kHipError;
            return kResidentGone;
        }
        __builtin_ia32_pause();
        if ((++spins & 0xFFFu) == 0u) {
            const auto now = std::chrono::steady_clock::now();
            if (spins == 0x1000u) t0 = now;
            else if (now - t0 > std::chrono::seconds(10)) {      // (the kernel's own time-outs are 5 s: this is a kernel that never started)
                __atomic_store_n(&hResident->seq, kResidentQuit, __ATOMIC_RELEASE);
                HIP_WARN(hipStreamSynchronize(stream));
                residentLive = false; residentStreak = 0; residentPlan = nullptr;
                return kHipError;
            }
        }
    }
    for (size_t c = 0; c < nOut; ++c) std::memcpy(out[c], hResOut + c * blockSize, n * sizeof(float));
    residentTicksBody += hResident->ticksBody; residentTicksEpilogue += hResident->ticksEpilogue;
    curBlockTime = hGlobals.sampleTime;
    hGlobals.sampleTime += (int64_t)n;
    st.blocksRendered++; st.residentBlocks++;
    islandBlocksInterp += current->levelOffsets.back();
    return kOk;
}

int Engine::timeLaunches(size_t nOut, size_t numBlocks, float* msOut, size_t cap) {
    RenderGuard lock(*this);
    if (dry) return -kNoDevice;
    if (hipSetDevice(device) != hipSuccess) return -kHipError;
    int rc = swapInPending();
    if (rc != kOk) return -rc;
    if (!current) return 0;
    const Plan& p = *current;
    const size_t L = p.levelOffsets.size() - 1;
    if (cap < L + 1) return -kInvalidPropertyValue;
    rc = ensureOutRing(std::max<size_t>(nOut, 1) * blockSize);
    if (rc != kOk) return -rc;
    if (hGlobals.ringSlots != 1 || hGlobals.blockSlot != 0) {
        hGlobals.ringSlots = 1; hGlobals.blockSlot = 0;
        patches.push_back(Patch{2u, (uint32_t)(offsetof(Globals, ringSlots) / 4), 1u, 0u});
        patches.push_back(Patch{2u, (uint32_t)(offsetof(Globals, blockSlot) / 4), 0u, 0u});
    }
    setGlobalsFor(0, nOut, (size_t)blockSize, hGlobals.sampleTime);
    setInRing(nullptr, 0);
    rc = flushPending();
    if (rc != kOk) return -rc;
    std::vector<hipEvent_t> ev(2 * (L + 2));   // + one empty pair: the cost of the event pair itself
    for (auto& e : ev) if (hipEventCreate(&e) != hipSuccess) return -kHipError;
    std::vector<double> acc(L + 2, 0.0);
    // timeBatch > 1: time the multi-block launches elemhip_process_blocks issues (msOut = per LAUNCH of `batch` blocks)
    const uint32_t batch = (timeBatch > 1 && p.convs.empty() && batchEligible(p, nOut)) ? (uint32_t)std::min<size_t>((size_t)timeBatch, maxSetBlocks(p)) : 1u;
    const uint32_t arenaFloats = batch > 1 ? p.numHbmBuffers * (uint32_t)blockSize : 0u;
    if (batch > 1) {
        rc = ensureHbm(arenaBuffers(p, batch)); if (rc != kOk) return -rc;
        rc = ensureOutRing(std::max<size_t>(nOut, 1) * blockSize * batch); if (rc != kOk) return -rc;
    }
    lastTimeBatch = batch;
    fixConvOverlaps(p);
    for (size_t b = 0; b < numBlocks; ++b) {
        for (size_t l = 0; l < L; ++l) {
            const uint32_t lb = p.levelOffsets[l], le = p.levelOffsets[l + 1];
            (void)hipEventRecord(ev[2 * l], stream);
            if (le > lb) { if (batch > 1) launchLevelBatch(p, l, batch, arenaFloats); else launch_level(stream, p.view, dRecs, dHbm, dGlobals, dLcg, lb, le - lb, p.levelLdsBytes[l], batch, arenaFloats, statelessRows); }
            if (p.convLevelOffsets[l + 1] > p.convLevelOffsets[l])
                launch_convolve(stream, p.view, dRecs, dHbm, dGlobals, p.convLevelOffsets[l], p.convLevelOffsets[l + 1] - p.convLevelOffsets[l]);
            (void)hipEventRecord(ev[2 * l + 1], stream);
        }
        (void)hipEventRecord(ev[2 * L], stream);
        if (batch > 1) launch_epilogue_batch(stream, p.view, dRecs, dHbm, dGlobals, dOutRing, batch, arenaFloats);
        else launch_epilogue(stream, p.view, dRecs, dHbm, dGlobals, dOutRing);
        (void)hipEventRecord(ev[2 * L + 1], stream);
        (void)hipEventRecord(ev[2 * L + 2], stream);
        (void)hipEventRecord(ev[2 * L + 3], stream);
        if (hipStreamSynchronize(stream) != hipSuccess) return -kHipError;
        for (size_t l = 0; l <= L + 1; ++l) { float ms = 0; (void)hipEventElapsedTime(&ms, ev[2 * l], ev[2 * l + 1]); acc[l] += ms; }
        for (uint32_t k = 0; k < batch; ++k) mirrorRootFades(p, (uint32_t)blockSize, (uint32_t)nOut, 0);
        hGlobals.sampleTime += (int64_t)blockSize * batch;
        st.blocksRendered += batch;
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    // an empty event pair measures the marker-to-marker cost that every timed launch also pays
    const double empty = acc[L + 1] / (double)std::max<size_t>(numBlocks, 1);
    for (size_t l = 0; l <= L; ++l) msOut[l] = (float)std::max(0.0, acc[l] / (double)std::max<size_t>(numBlocks, 1) - empty);
    if (cap > L + 1) msOut[L + 1] = (float)empty;
    if (cap > L + 2) msOut[L + 2] = (float)batch;   // blocks per timed launch
    return (int)(L + 1);
}

int Engine::traceLevel(size_t nOut, uint32_t level, unsigned long long* out, size_t cap) {
    RenderGuard lock(*this);
    if (dry) return kNoDevice;
    if (hipSetDevice(device) != hipSuccess) return kHipError;
    int rc = swapInPending();
    if (rc != kOk) return rc;
    if (!current || cap < kWaves * 192) return kInvalidPropertyValue;
    const Plan& p = *current;
    const size_t L = p.levelOffsets.size() - 1;
    rc = ensureOutRing(std::max<size_t>(nOut, 1) * blockSize);
    if (rc != kOk) return rc;
    unsigned long long* dTrace = nullptr;
    HIP_OK(hipMalloc(&dTrace, kWaves * 192 * 8));
    HIP_OK(hipMemset(dTrace, 0, kWaves * 192 * 8));
    if (hGlobals.ringSlots != 1 || hGlobals.blockSlot != 0) {
        hGlobals.ringSlots = 1; hGlobals.blockSlot = 0;
        patches.push_back(Patch{2u, (uint32_t)(offsetof(Globals, ringSlots) / 4), 1u, 0u});
        patches.push_back(Patch{2u, (uint32_t)(offsetof(Globals, blockSlot) / 4), 0u, 0u});
    }
    setGlobalsFor(0, nOut, (size_t)blockSize, hGlobals.sampleTime);
    setInRing(nullptr, 0);
    rc = flushPending();
    if (rc != kOk) return rc;
    const uint64_t tp = (uint64_t)reinterpret_cast<uintptr_t>(dTrace);
    const uint32_t batch = (timeBatch > 1 && p.convs.empty() && batchEligible(p, nOut)) ? (uint32_t)std::min<size_t>((size_t)timeBatch, maxSetBlocks(p)) : 1u;
    const uint32_t arenaFloats = batch > 1 ? p.numHbmBuffers * (uint32_t)blockSize : 0u;
    if (batch > 1) {
        rc = ensureHbm(arenaBuffers(p, batch)); if (rc != kOk) return rc;
        rc = ensureOutRing(std::max<size_t>(nOut, 1) * blockSize * batch); if (rc != kOk) return rc;
    }
    for (size_t l = 0; l < L; ++l) {
        const uint32_t lb = p.levelOffsets[l], le = p.levelOffsets[l + 1];
        const uint64_t v = (l == level) ? tp : 0;
        HIP_OK(hipMemcpyAsync(reinterpret_cast<char*>(dGlobals) + offsetof(Globals, trace), &v, 8, hipMemcpyHostToDevice, stream));
        if (le > lb) { if (batch > 1) launchLevelBatch(p, l, batch, arenaFloats); else launch_level(stream, p.view, dRecs, dHbm, dGlobals, dLcg, lb, le - lb, p.levelLdsBytes[l], batch, arenaFloats, statelessRows); }
    }
    const uint64_t zero = 0;
    HIP_OK(hipMemcpyAsync(reinterpret_cast<char*>(dGlobals) + offsetof(Globals, trace), &zero, 8, hipMemcpyHostToDevice, stream));
    if (batch > 1) launch_epilogue_batch(stream, p.view, dRecs, dHbm, dGlobals, dOutRing, batch, arenaFloats);
    else launch_epilogue(stream, p.view, dRecs, dHbm, dGlobals, dOutRing);
    HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(hipMemcpy(out, dTrace, kWaves * 192 * 8, hipMemcpyDeviceToHost));
    (void)hipFree(dTrace);
    for (uint32_t k = 0; k < batch; ++k) mirrorRootFades(p, (uint32_t)blockSize, (uint32_t)nOut, 0);
    hGlobals.sampleTime += (int64_t)blockSize * batch;
    st.blocksRendered += batch;
    return kOk;
}

// A multi-block launch carries no per-block root/tap/convolver bookkeeping: it is used only while every
// running root's fade is settled (Core.h:28-31) and the plan has neither taps nor convolvers.
// every island shape of the sequence has its kernel loaded on this device (stateless islands stay with the interpreter kernel)
bool Engine::specReady(const Plan& p) const {
    if (specialize == 0 || p.shapes.empty()) return false;
    bool any = false;
    for (const Plan::SpecShape& sh : p.shapes) {
        if (sh.entry->function(device)) any = true;
        else if (!sh.optional) return false;
    }
    return any;
}

void Engine::promoteDeferredShapes() {
    Plan* p = current.get();
    if (!p || !p->deferredShapes) return;
    if (st.blocksRendered - p->blocksAtAdoption < (uint64_t)std::max(0, lonelyBlocks)) return;
    if (std::chrono::steady_clock::now() - p->adopted < std::chrono::milliseconds(std::max(0, lonelyMs))) return;
    for (Plan::SpecShape& sh : p->shapes)
        if (sh.deferred) { Jit::get().promote(sh.entry); sh.deferred = false; }
    p->deferredShapes = 0;
}

bool Engine::anyRootRuns(const std::vector<int32_t>& rootIds, size_t nOut) const {
    for (int32_t id : rootIds) {
        auto it = nodes.find(id);
        if (it == nodes.end()) return true;          // (cannot tell: launch)
        const Node& r = it->second;
        const bool on = r.target > 0.5f, settled = std::fabs(r.target - r.gain) <= 1e-6f;
        if ((on || !settled) && r.channel >= 0 && (uint32_t)r.channel < nOut) return true;
    }
    return false;
}

// (oneBlock: a launch set of ONE — the batch epilogue promotes the taps after it like the per-block epilogue does, so tap
// pairs that do not sit in one island are no obstacle)
bool Engine::batchEligible(const Plan& p, size_t nOut, bool oneBlock) const {
    if ((!oneBlock && !p.taps.empty() && !p.tapsInSets) || !p.hosts.empty()) return false;
    // convolvers: the multi-block kernels (conv.hip) assume every node's 512-frame input block is empty at the start of a
    // launch set, i.e. that every call so far rendered whole 512-frame blocks
    if (!p.convs.empty() && !(convAligned && blockSize == (int)conv::kBlock)) return false;
    for (int32_t id : p.rootIds) {
        auto it = nodes.find(id);
        if (it == nodes.end()) return false;
        const Node& r = it->second;
        const bool on = r.target > 0.5f;
        const bool settled = std::fabs(r.target - r.gain) <= 1e-6f;
        const bool running = (on || !settled) && r.channel >= 0 && (uint32_t)r.channel < nOut;
        if (running && r.gain != r.target) return false;
    }
    return true;
}

hipEvent_t Engine::profEvent() {
    if (profUsed == profEvents.size()) { hipEvent_t e = nullptr; (void)hipEventCreate(&e); profEvents.push_back(e); }
    return profEvents[profUsed++];
}

// after a stream synchronize: fold the event pairs of this call into the per-level sums
void Engine::profCollect() {
    for (size_t k = 0; k + 1 < profUsed; k += 2) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, profEvents[k], profEvents[k + 1]) != hipSuccess) continue;
        const uint32_t slot = profSlots[k / 2];
        if (profMs.size() <= slot) profMs.resize(slot + 1, 0.0);
        profMs[slot] += ms;
    }
    profUsed = 0; profSlots.clear();
}

// debug / tests: program text and compile state of the k-th specialised shape of the newest plan
int Engine::specInfo(size_t k, std::string* source, std::string* log, int* state, uint32_t* islands) {
    std::lock_guard<std::mutex> control(ctl);
    RenderGuard lock(*this);
    const std::shared_ptr<Plan> pl = pending ? pending : current;
    if (!pl || k >= pl->shapes.size()) return -1;
    const Plan::SpecShape& sh = pl->shapes[k];
    if (source) *source = sh.entry->fullText();
    if (log) *log = sh.entry->log;
    if (state) *state = sh.entry->state.load();
    if (islands) *islands = sh.count;
    return (int)pl->shapes.size();
}

int Engine::launchProfile(double* msOut, size_t cap, uint64_t* launchSets, uint64_t* blocks) {
    RenderGuard lock(*this);
    if (launchSets) *launchSets = profSets;
    if (blocks) *blocks = profBlocks;
    const size_t n = std::min(cap, profMs.size());
    for (size_t i = 0; i < n; ++i) msOut[i] = profMs[i];
    return (int)profMs.size();
}

// One launch level of a multi-block launch. When every island shape of the level has its specialised kernel compiled
// (jit.cpp) the level runs as one launch per shape plus an interpreter launch for the islands no shape covers
// (stateless mixers and roots); until then the whole level goes through the interpreter kernel.
void Engine::launchLevelBatch(const Plan& p, size_t l, uint32_t batch, uint32_t arenaFloats) {
    const uint32_t b = p.levelOffsets[l], e = p.levelOffsets[l + 1];
    if (e <= b) return;
    bool spec = specialize != 0 && !p.shapes.empty();
    std::vector<std::pair<hipFunction_t, const Plan::SpecShape*>> fns;   // function null: the shape is not compiled (yet)
    struct InterpRun { uint32_t begin, count; };                          // contiguous stretches of specLists the interpreter kernel renders
    std::vector<InterpRun> interpRuns;
    if (spec) {
        bool any = false;
        int specTaken = 0;
        for (const Plan::SpecShape& sh : p.shapes) {
            if (sh.level != (uint32_t)l) continue;
            // (the level's shapes are listed biggest first, plan.cpp: the first `maxShapeLaunches` compiled ones get their kernels)
            hipFunction_t fn = specTaken < maxShapeLaunches ? sh.entry->function(device) : nullptr;
            if (fn) ++specTaken;
            any = any || fn != nullptr;
            // A launch whose islands all belong to roots that do not run (a replaced root once its fade-out has settled stays in
            // the plan until the next commit) would start workgroups that return at once — and, as a second launch of its
            // level, cost a fork to a side stream and a join. The host mirrors the root fades (mirrorRootFades), and launch
            // sets are only rendered while every running root's fade is settled: what runs does not change inside a set.
            if (skipIdleLaunches && !anyRootRuns(sh.roots, hGlobals.numOut)) { st.idleLaunchesSkipped++; continue; }
            if (fn) { fns.emplace_back(fn, &sh); continue; }
            // not compiled (yet), or beyond the launch cap: joins the interpreter run that ends where its list begins, or starts one
            if (!interpRuns.empty() && interpRuns.back().begin + interpRuns.back().count == sh.listBegin) interpRuns.back().count += sh.count;
            else interpRuns.push_back({sh.listBegin, sh.count});
        }
        if (!any) spec = false;
    }
    if (!spec) { launch_level(stream, p.view, dRecs, dHbm, dGlobals, dLcg, b, e - b, p.levelLdsBytes[l], batch, arenaFloats, statelessRows); islandBlocksInterp += (uint64_t)(e - b) * batch; debugSync("set: interpreter level", (unsigned)l, batch); return; }
    // The launches of one level are independent of each other (different islands): with more than one they go to side
    // streams forked from / joined to the engine's stream, so two shapes of 64 islands each fill 128 CUs at once
    // instead of 64 CUs twice.
    uint32_t rb = p.restOffsets[l], re = p.restOffsets[l + 1];
    if (re > rb && skipIdleLaunches && l < p.restRoots.size() && !anyRootRuns(p.restRoots[l], hGlobals.numOut)) { re = rb; st.idleLaunchesSkipped++; }
    const size_t launches = fns.size() + interpRuns.size() + (re > rb ? 1 : 0);
    if (launches == 0) return;
    const bool fork = launches > 1;
    if (fork) {
        while (auxStreams.size() < launches - 1) {
            hipStream_t s2 = nullptr; hipEvent_t ev = nullptr;
            // a side stream must not share a hardware queue with the engine's stream (the runtime hands queues out round-robin
            // per priority class; in a process with many streams two shapes of C4 landed on one queue and ran back to back,
            // 12.9 -> 25 us per block): side streams alternate between the two other priority classes
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            const int prio = (auxStreams.size() % 2 == 0) ? greatest : least;
            if (least == greatest || hipStreamCreateWithPriority(&s2, hipStreamNonBlocking, prio) != hipSuccess)
                HIP_WARN(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
            HIP_WARN(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            auxStreams.push_back(s2); auxDone.push_back(ev);
        }
        if (!forkEvent) HIP_WARN(hipEventCreateWithFlags(&forkEvent, hipEventDisableTiming));
        HIP_WARN(hipEventRecord(forkEvent, stream));
    }
    size_t k = 0;
    auto streamFor = [&](size_t idx) -> hipStream_t {
        if (!fork || idx == 0) return stream;
        hipStream_t s2 = auxStreams[idx - 1];
        HIP_WARN(hipStreamWaitEvent(s2, forkEvent, 0));
        return s2;
    };
    for (const InterpRun& r : interpRuns) {   // these shapes' islands go through the interpreter kernel (their lists have the levelIslands entry format)
        PlanView pv = p.view;
        pv.levelIslands = p.dSpecLists;
        launch_level(streamFor(k++), pv, dRecs, dHbm, dGlobals, dLcg, r.begin, r.count, p.levelLdsBytes[l], batch, arenaFloats, statelessRows);
        islandBlocksInterp += (uint64_t)r.count * batch;
    }
    for (auto& f : fns) {
        hipStream_t st_ = streamFor(k++);
        PlanView pv = p.view;
        uint32_t* recs = dRecs; float* hbm = dHbm; const Globals* g = dGlobals; const uint32_t* lcg = dLcg;
        const uint32_t* list = p.dSpecLists + f.second->listBegin;
        // the stream ring sits behind the `batch` block slices of this launch set
        uint32_t bt = batch, af = arenaFloats, sb = batch * arenaFloats, ss = p.numStreamBuffers * (uint32_t)blockSize;
        void* args[] = {&pv, &recs, &hbm, &g, &lcg, &list, &bt, &af, &sb, &ss};
        const uint32_t gy = f.second->stateless ? std::max(1u, std::min(batch, statelessRows)) : 1u;
        HIP_WARN(hipModuleLaunchKernel(f.first, f.second->count, gy, 1, kThreads, 1, 1, 0, st_, args, nullptr));
        st.specLaunches++;
        islandBlocksSpec += (uint64_t)f.second->count * batch;
        debugSync("set: specialised shape", f.second->count, batch);
    }
    if (re > rb) {
        PlanView pv = p.view;
        pv.levelIslands = p.dRestIslands;
        launch_level(streamFor(k++), pv, dRecs, dHbm, dGlobals, dLcg, rb, re - rb, p.levelLdsBytes[l], batch, arenaFloats, statelessRows);
        islandBlocksInterp += (uint64_t)(re - rb) * batch;
        debugSync("set: interpreter rest", re - rb, batch);
    }
    if (fork) {
        for (size_t i = 1; i < launches; ++i) {
            HIP_WARN(hipEventRecord(auxDone[i - 1], auxStreams[i - 1]));
            HIP_WARN(hipStreamWaitEvent(stream, auxDone[i - 1], 0));
        }
    }
}

// the convolve nodes of level l over a whole launch set: four launches (fft, mac, ifft, finish: conv.hip, "multi-block launches")
void Engine::launchConvolveBatch(const Plan& p, size_t l, uint32_t batch, uint32_t arenaFloats) {
    const uint32_t cb = p.convLevelOffsets[l], ce = p.convLevelOffsets[l + 1];
    uint32_t mains = 0;
    while (cb + mains < ce && (p.convWork[cb + mains] >> 16) == 0u) ++mains;   // main entries lead a level's work list
    if (!mains) return;
    // which nodes of the level have long-partition spectra (an IR can be replaced without a re-plan: looked up per launch set)
    bool anyShortPath = false;
    uint32_t stateBlocks = 1;
    for (uint32_t k = 0; k < mains; ++k) {
        const uint32_t ci = p.convWork[cb + k] & 0xFFFFu;
        auto it = ci < p.convNodeIds.size() ? nodes.find(p.convNodeIds[ci]) : nodes.end();
        if (it == nodes.end() || it->second.convQp == 0u) { anyShortPath = true; continue; }
        stateBlocks = std::max(stateBlocks, std::max(it->second.convHistBlocks, it->second.convP));
    }
    const uint32_t longRows = (convLong && convMaxQp) ? convMaxQp - 1u : 0u;
    const bool longSet = longRows && batch >= 8u && (batch & 7u) == 0u;
    {   // the scratch holds per-node headers (which convolver's spectra its ring carries from set to set, conv_long.inc): they mean
        // something only under the layout they were written for — a new allocation or another set geometry starts from zeroed scratch
        const uint64_t key = ((uint64_t)(uint32_t)batchBlocks << 32) | longRows;
        if (key != convScratchKey && dConvScratch) { HIP_WARN(hipMemsetAsync(dConvScratch, 0, convScratchFloats * sizeof(float), stream)); convScratchKey = key; }
    }
    if (longSet && stateBlocks > 1u) {
        convLongSets++;
        // staleness is a fact of a NODE (its header's H_OVL_STALE), not of the engine: a plan without this node may render
        // block-at-a-time in between, and the node must still be repaired when a later plan brings it back
        for (uint32_t k = 0; k < mains; ++k) {
            const uint32_t ci = p.convWork[cb + k] & 0xFFFFu;
            if (ci < p.convNodeIds.size()) convStaleNodes.insert(p.convNodeIds[ci]);
        }
    }
    if (!longSet) fixConvOverlaps(p);
    launch_convolve_batch(stream, p.view, dRecs, dHbm, dGlobals, cb, mains, batch, arenaFloats, dConvScratch, (uint32_t)batchBlocks, (uint32_t)convMfma,
                          convMinP <= convolve_mfma_max_partitions(), convMaxP > convolve_mfma_max_partitions(), longRows, anyShortPath, stateBlocks,
                          longSet ? setInDirect : nullptr, setNumIn, longSet ? setOutDirect : nullptr, setNumOut);
}

// A plan that consists of long-partition convolvers only (BASELINE configs[2]: root(convolve(in)) per channel — in and root folded into
// the node's launches) needs neither the copy of the caller's input blocks into the arenas nor the bus-sum epilogue of a launch set:
// the long-partition kernels read the [block][channel][frame] input where it lies, and when every output channel of the call is the
// folded root of exactly one running convolver they write the caller's output buffer themselves (r05: 8.4 + 9.5 us of a 118 us C3 set).
void Engine::chooseConvDirectIo(const Plan& p, size_t nIn, size_t nOut, uint32_t batch, bool haveIn, bool& dIn, bool& dOut) {
    dIn = dOut = false;
    if (!convDirectIo || !convLong || !convMaxQp || p.convs.empty() || !p.levelIslands.empty() || !p.hosts.empty() || !p.taps.empty()) return;
    if (batch < 8u || (batch & 7u) != 0u) return;
    std::vector<uint32_t> fused;
    for (size_t ci = 0; ci < p.convs.size(); ++ci) {
        auto it = ci < p.convNodeIds.size() ? nodes.find(p.convNodeIds[ci]) : nodes.end();
        if (it == nodes.end() || it->second.convQp == 0u) return;            // a node without long-partition spectra: the 512-partition kernels read the arenas
        if (p.convs[ci].fuseRootRec != kNone) fused.push_back(p.convs[ci].fuseRootRec);
    }
    dIn = haveIn;
    std::vector<uint8_t> seen(nOut, 0);
    size_t covered = 0;
    for (int32_t id : p.rootIds) {
        auto it = nodes.find(id);
        if (it == nodes.end()) return;
        const Node& r = it->second;
        const bool on = r.target > 0.5f, settled = std::fabs(r.target - r.gain) <= 1e-6f;
        if (!((on || !settled) && r.channel >= 0 && (size_t)r.channel < nOut)) continue;   // not running (or a channel the call does not ask for)
        if (std::find(fused.begin(), fused.end(), r.rec) == fused.end() || seen[(size_t)r.channel]) return;
        seen[(size_t)r.channel] = 1; ++covered;
    }
    dOut = covered == nOut && nOut > 0;
}

void Engine::fixConvOverlaps(const Plan& p) {
    if (convStaleNodes.empty() || p.convs.empty() || !dConvScratch) return;
    bool any = false;
    for (int32_t id : p.convNodeIds) any = convStaleNodes.erase(id) > 0 || any;      // (the kernels return early for nodes whose header is not stale)
    if (!any) return;
    launch_convolve_fix_overlap(stream, p.view, dRecs, dHbm, dGlobals, 0u, (uint32_t)p.convWork.size(), dConvScratch, (uint32_t)batchBlocks,
                                (convLong && convMaxQp) ? convMaxQp - 1u : 0u, convMaxP);
}

void Engine::enqueueBatch(const Plan& p, uint32_t batch, float* outRing) {
    if (!outRing) outRing = dOutRing;
    const uint32_t arenaFloats = p.numHbmBuffers * (uint32_t)blockSize;
    const size_t L = p.levelOffsets.size() - 1;
    const bool prof = profileLaunches && (profSetCounter++ % profileEvery) == 0u;
    for (size_t l = 0; l < L; ++l) {
        const uint32_t b = p.levelOffsets[l], e = p.levelOffsets[l + 1];
        if (e <= b && p.convLevelOffsets[l + 1] <= p.convLevelOffsets[l]) continue;
        if (prof) (void)hipEventRecord(profEvent(), stream);
        launchLevelBatch(p, l, batch, arenaFloats);
        launchConvolveBatch(p, l, batch, arenaFloats);
        if (prof) { (void)hipEventRecord(profEvent(), stream); profSlots.push_back((uint32_t)l); }
    }
    if (prof && !setOutDirect) (void)hipEventRecord(profEvent(), stream);      // (a direct-I/O set has no epilogue to bracket: two stream operations less per set)
    if (setOutDirect) {
        // the convolvers wrote the caller's buffer themselves (chooseConvDirectIo): what is left of the epilogue is the device's sample
        // clock, moved on by a parameter patch (applied in stream order with the next call's patches)
        // (r06: ... and only once something is about to READ it — a stream of such sets has no island, no epilogue and no other
        //  reader of the clock, and a patch launch per set was 4 us of kernel plus its launch gap in front of every 70 us of work:
        //  flushPending brings the device's clock up to the host's before the first launch that is not another direct set)
        deviceClockBehind = true;
    } else {
        launch_epilogue_batch(stream, p.view, dRecs, dHbm, dGlobals, outRing, batch, arenaFloats, armFlag, armValue);
        if (armFlag && batch == 1u) flagArmed = true;
    }
    debugSync("set: epilogue", batch);
    if (prof && !setOutDirect) { (void)hipEventRecord(profEvent(), stream); profSlots.push_back((uint32_t)L); }
    if (prof) { profSets++; profBlocks += batch; if (profMs.size() <= L) profMs.resize(L + 1, 0.0); }     // (slot L = the epilogue, 0 for direct sets)
}

bool Engine::specBlockOk(const Plan& p) const { return specBlocks && p.convs.empty() && p.hosts.empty() && specReady(p); }

void Engine::enqueueSpecBlock(const Plan& p, float* outRing) {
    if (!outRing) outRing = dOutRing;
    const uint32_t arenaFloats = p.numHbmBuffers * (uint32_t)blockSize;
    const size_t L = p.levelOffsets.size() - 1;
    for (size_t l = 0; l < L; ++l) launchLevelBatch(p, l, 1u, arenaFloats);
    launch_epilogue(stream, p.view, dRecs, dHbm, dGlobals, outRing, armFlag, armValue);
    if (armFlag) flagArmed = true;
    debugSync("block: specialised levels + epilogue");
    st.specFadeBlocks++;
}

int Engine::processBlocks(const float* inDev, size_t nIn, float* outDev, size_t nOut, size_t numBlocks, int64_t sampleTime) {
    RenderGuard lock(*this);
    if (dry) return kNoDevice;
    if (hostBlockSize != blockSize) return kBlockTooLarge;     // (the device-resident layout is [block][channel][blockSize <= 512])
    if (hipSetDevice(device) != hipSuccess) return kHipError;
    int rc = enqueueBlocks(inDev, nIn, outDev, nOut, numBlocks, sampleTime);
    if (rc != kOk) return rc;
    HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(hipGetLastError());
    if (profUsed) profCollect();
    freeDeferred();
    return kOk;
}

// `mu` held, device current. Everything is enqueued on `stream`; the caller synchronises.
int Engine::enqueueBlocks(const float* inDev, size_t nIn, float* outDev, size_t nOut, size_t numBlocks, int64_t sampleTime) {
    if (nIn > kMaxHostIn || nOut > kMaxOutBus) return kTooManyChannels;
    armFlag = nullptr; flagArmed = false;      // (no launch set publishes elemhip_process' completion word)
    int rc = swapInPending();
    if (rc != kOk) return rc;
    if (!current || numBlocks == 0) return kOk;
    Plan& p = *current;
    if (p.packedRootChannels > 0 && nOut < (size_t)p.packedRootChannels) {      // (plan.cpp `pack_roots`: a packed root would not run in the reference)
        std::fprintf(stderr, "[elemhip] pack_roots: this plan needs calls with at least %d output channels\n", p.packedRootChannels);
        return kInvalidPropertyValue;
    }
    const size_t bs = (size_t)blockSize;
    const bool graphOk = useGraph && p.hosts.empty() && !debugSyncOn();   // call-out nodes synchronise inside a block: nothing to capture
    const bool haveIn = nIn > 0 && inDev != nullptr;
    const size_t G = graphOk ? (size_t)graphBlocks : 1;
    rc = ensureOutRing(std::max<size_t>(nOut, 1) * bs * G);
    if (rc != kOk) return rc;

    setGlobalsFor(nIn, nOut, bs, sampleTime);
    size_t done = 0;
    while (done < numBlocks) {
        if (batchBlocks > 1 && numBlocks - done > 1 && batchEligible(p, nOut)) {
            // ---- multi-block launches: one kernel per level renders `chunk` blocks (kernels.hip) ----
            const size_t setCap = std::min((size_t)batchBlocks, maxSetBlocks(p));
            const size_t chunk = std::min(setCap, numBlocks - done);
            rc = ensureHbm(arenaBuffers(p, setCap));
            if (rc != kOk) return rc;
            rc = ensureOutRing(std::max<size_t>(nOut, 1) * bs * (size_t)batchBlocks);
            if (rc != kOk) return rc;
            if (!p.convs.empty()) {
                const size_t need = p.convs.size() * convolve_batch_scratch_floats((uint32_t)batchBlocks, (convLong && convMaxQp) ? convMaxQp - 1u : 0u);
                if (need > convScratchFloats) {
                    HIP_OK(hipStreamSynchronize(stream));
                    if (dConvScratch) (void)hipFree(dConvScratch);
                    dConvScratch = nullptr; convScratchFloats = 0;
                    HIP_OK(hipMalloc(&dConvScratch, need * sizeof(float)));
                    convScratchFloats = need;
                    convScratchKey = ~0ull;        // (its per-node headers are garbage: zeroed before the first launch that reads them)
                }
            }
            setInRing(nullptr, 0);
            hGlobals.blockSlot = 0;
            bool dIn = false, dOut = false;
            chooseConvDirectIo(p, nIn, nOut, (uint32_t)chunk, haveIn, dIn, dOut);
            float* const outTarget = (outDev && nOut > 0) ? outDev + done * nOut * bs : nullptr;
            setInDirect = dIn ? inDev + done * nIn * bs : nullptr; setNumIn = (uint32_t)nIn;
            setOutDirect = dOut ? (outTarget ? outTarget : dOutRing) : nullptr; setNumOut = (uint32_t)nOut;
            if (dIn || dOut) convDirectSets++;
            nextSetDirect = dOut;
            if (haveIn && !dIn)   // host inputs of block b -> arena buffers 0..nIn-1 of block b's arena
                HIP_OK(hipMemcpy2DAsync(dHbm, (size_t)p.numHbmBuffers * bs * sizeof(float), inDev + done * nIn * bs, nIn * bs * sizeof(float),
                                        nIn * bs * sizeof(float), chunk, hipMemcpyDeviceToDevice, stream));
            rc = flushPending();
            nextSetDirect = false;
            if (rc != kOk) return rc;
            // the set's epilogue sums the roots straight into the caller's [block][channel][frame] buffer (r04: into the engine's ring and
            // a device-to-device copy behind it — 5.6 us of a 135 us C3 set, 100 us of a C4 set)
            enqueueBatch(p, (uint32_t)chunk, outTarget);
            setInDirect = nullptr; setOutDirect = nullptr;
            hGlobals.sampleTime += (int64_t)(chunk * bs);
            done += chunk;
            st.blocksRendered += chunk;
            promoteDeferredShapes();
            st.batchLaunches++;
            continue;
        }
        if (specBlockOk(p)) {
            // ---- one block through the specialised kernels (root fades running, or a call of one block) ----
            rc = ensureHbm(arenaBuffers(p, 1));
            if (rc != kOk) return rc;
            if (hGlobals.ringSlots != 1u || hGlobals.blockSlot != 0u) {
                hGlobals.ringSlots = 1u; hGlobals.blockSlot = 0u;
                patches.push_back(Patch{2u, (uint32_t)(offsetof(Globals, ringSlots) / 4), 1u, 0u});
                patches.push_back(Patch{2u, (uint32_t)(offsetof(Globals, blockSlot) / 4), 0u, 0u});
            }
            setInRing(nullptr, 0);
            if (haveIn) HIP_OK(hipMemcpyAsync(dHbm, inDev + done * nIn * bs, nIn * bs * sizeof(float), hipMemcpyDeviceToDevice, stream));
            rc = flushPending();
            if (rc != kOk) return rc;
            curBlockTime = hGlobals.sampleTime;
            if (batchEligible(p, nOut, true)) enqueueBatch(p, 1u); else enqueueSpecBlock(p);
            if (outDev && nOut > 0)
                HIP_OK(hipMemcpyAsync(outDev + done * nOut * bs, dOutRing, nOut * bs * sizeof(float), hipMemcpyDeviceToDevice, stream));
            mirrorRootFades(p, (uint32_t)bs, (uint32_t)nOut, (uint32_t)nIn);
            hGlobals.sampleTime += (int64_t)bs;
            done += 1;
            st.blocksRendered += 1;
            promoteDeferredShapes();
            continue;
        }
        const size_t chunk = std::min(G, numBlocks - done);
        // ring geometry for this chunk
        if (hGlobals.ringSlots != (uint32_t)G || hGlobals.blockSlot != 0) {
            hGlobals.ringSlots = (uint32_t)G; hGlobals.blockSlot = 0;
            patches.push_back(Patch{2u, (uint32_t)(offsetof(Globals, ringSlots) / 4), (uint32_t)G, 0u});
            patches.push_back(Patch{2u, (uint32_t)(offsetof(Globals, blockSlot) / 4), 0u, 0u});
        }
        // host inputs: block 0 of the chunk is copied here, the epilogue of block k stages block k + 1
        setInRing(haveIn ? inDev + done * nIn * bs : nullptr, haveIn ? (uint32_t)chunk : 0u);
        if (haveIn) HIP_OK(hipMemcpyAsync(dHbm, inDev + done * nIn * bs, nIn * bs * sizeof(float), hipMemcpyDeviceToDevice, stream));
        rc = flushPending();
        if (rc != kOk) return rc;
        fixConvOverlaps(p);      // (convolve nodes a long-partition set rendered last: their overlap, before block-at-a-time launches read it)
        // (a plan is captured at its third block-at-a-time chunk: a live graph's plan renders the two blocks of its root fades this
        //  way, then launch sets take over and the next commit replaces it — a capture would be made and thrown away every time)
        if (graphOk && chunk == G && (p.graphExec || ++p.blockChunks > 2u)) {
            if (!p.graphExec || p.graphBlocks != (int)G) {
                if (p.graphExec) { (void)hipGraphExecDestroy(p.graphExec); p.graphExec = nullptr; }
                hipGraph_t graph = nullptr;
                HIP_OK(hipStreamSynchronize(stream));
                const auto tc0 = std::chrono::steady_clock::now();
                const uint64_t ibi = islandBlocksInterp;
                HIP_OK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
                for (size_t b = 0; b < G; ++b) enqueueBlock(p);
                HIP_OK(hipStreamEndCapture(stream, &graph));
                islandBlocksInterp = ibi;                                   // (counted per replay below)
                HIP_OK(hipGraphInstantiate(&p.graphExec, graph, nullptr, nullptr, 0));
                (void)hipGraphDestroy(graph);
                p.graphBlocks = (int)G;
                st.graphCaptures++;
                st.lastGraphCaptureMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc0).count();
            }
            HIP_OK(hipGraphLaunch(p.graphExec, stream));
            st.graphReplays++;
            islandBlocksInterp += (uint64_t)G * p.levelIslands.size();
        } else {
            for (size_t b = 0; b < chunk; ++b) { curBlockTime = hGlobals.sampleTime + (int64_t)(b * bs); enqueueBlock(p); }
        }
        if (outDev && nOut > 0)
            HIP_OK(hipMemcpyAsync(outDev + done * nOut * bs, dOutRing, chunk * nOut * bs * sizeof(float), hipMemcpyDeviceToDevice, stream));
        // host mirrors of device-side block state
        for (size_t b = 0; b < chunk; ++b) mirrorRootFades(p, (uint32_t)bs, (uint32_t)nOut, (uint32_t)nIn);
        hGlobals.sampleTime += (int64_t)(chunk * bs);
        hGlobals.blockSlot = (uint32_t)((hGlobals.blockSlot + chunk) % G);
        done += chunk;
        st.blocksRendered += chunk;
        promoteDeferredShapes();
    }
    return kOk;
}

int Engine::ensureHostStaging(size_t outFloats, size_t inFloats) {
    if (!ioStream) {
        HIP_OK(hipStreamCreateWithFlags(&ioStream, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) {
            HIP_OK(hipEventCreateWithFlags(&evIn[k], hipEventDisableTiming));
            HIP_OK(hipEventCreateWithFlags(&evRendered[k], hipEventDisableTiming));
            HIP_OK(hipEventCreateWithFlags(&evOut[k], hipEventDisableTiming));
        }
    }
    const int rc = growHalves(hStageOut, dStageOut, stageOutFloats, outFloats);
    return rc != kOk ? rc : growHalves(hStageIn, dStageIn, stageInFloats, inFloats);
}

int Engine::ensureRowTable(uint16_t*& dev, uint32_t& haveGroup, uint32_t& dwords, uint32_t group) {
    if (group == haveGroup) return kOk;
    // (the device is idle between calls: every host-path call ends with both streams synchronised)
    if (!dev) HIP_OK(hipMalloc((void**)&dev, pcm_pack::kMaxGroup * sizeof(uint16_t)));
    std::vector<uint16_t> table(group);
    const uint32_t n = pcm_pack_row_table(group, table.data());
    HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(hipMemcpy(dev, table.data(), group * sizeof(uint16_t), hipMemcpyHostToDevice));
    haveGroup = group; dwords = n;
    return kOk;
}

// a pinned and a device pair of staging halves, grown to `want` T's (the float halves, and the packed ones through growPackedHalves)
template <class T> int Engine::growHalves(T* (&h)[2], T* (&d)[2], size_t& have, size_t want) {
    if (want <= have) return kOk;
    HIP_OK(hipStreamSynchronize(stream));
    if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
    // the new buffers first: a failed allocation leaves the old pair (and `have`) as they were
    T* nh[2] = {nullptr, nullptr}; T* nd[2] = {nullptr, nullptr};
    bool ok = true;
    for (int k = 0; k < 2 && ok; ++k)
        ok = hipHostMalloc((void**)&nh[k], want * sizeof(T), hipHostMallocDefault) == hipSuccess && hipMalloc((void**)&nd[k], want * sizeof(T)) == hipSuccess;
    if (!ok) {
        for (int k = 0; k < 2; ++k) { if (nh[k]) (void)hipHostFree(nh[k]); if (nd[k]) (void)hipFree(nd[k]); }
        (void)hipGetLastError();
        return kHipError;
    }
    for (int k = 0; k < 2; ++k) {
        if (h[k]) (void)hipHostFree(h[k]);
        if (d[k]) (void)hipFree(d[k]);
        h[k] = nh[k]; d[k] = nd[k];
    }
    have = want;
    return kOk;
}
template int Engine::growHalves(float* (&)[2], float* (&)[2], size_t&, size_t);
template int Engine::growHalves(unsigned char* (&)[2], unsigned char* (&)[2], size_t&, size_t);

int Engine::ensurePcmStaging(size_t bytes, uint32_t group) {
    const int rc = ensureRowTable(dPcmRowBase, pcmTableGroup, pcmRowDwords, group);
    return rc != kOk ? rc : growPackedHalves(hPcm, dPcm, pcmBytes, bytes);
}

int Engine::ensurePcmInStaging(size_t bytes, uint32_t group) {
    const int rc = ensureRowTable(dPcmInRowBase, pcmInTableGroup, pcmInRowDwords, group);
    return rc != kOk ? rc : growPackedHalves(hPcmIn, dPcmIn, pcmInBytes, bytes);
}

// Runtime::process for a whole offline render (offline-renderer/index.ts:87-133): planar host arrays of `numFrames` frames.
// Set k (up to `batch_blocks` blocks) is gathered into pinned half k % 2, copied in on the copy stream, rendered on the
// engine's stream into device half k % 2, copied out on the copy stream and scattered to the caller's arrays while set
// k + 1 renders. The render lock is taken per set: a commit on another thread lands between two sets (block boundary).
int Engine::processBlocksHost(const float* const* in, size_t nIn, float* const* out, size_t nOut, size_t numFrames, int64_t sampleTime) {
    if (dry) return kNoDevice;
    if (nIn > kMaxHostIn || nOut > kMaxOutBus) return kTooManyChannels;
    if ((nIn && !in) || (nOut && !out)) return kInvalidInstructionFormat;
    return renderHostSets(in, nIn, out, nOut, numFrames, sampleTime, nullptr);
}

int Engine::processBlocksPcm(const float* const* in, size_t nIn, void* const* streams, size_t nStreams, float* const* planar,
                             size_t numFrames, int64_t sampleTime, const PcmSpec& spec, PcmChannelStats* stats) {
    if (!pcm_pack::format_ok(spec.format) || spec.channelsPerStream == 0u || (nStreams && !streams) || (nIn && !in)) return kInvalidInstructionFormat;
    if (nIn > kMaxHostIn || nStreams > kMaxOutBus || nStreams * (size_t)spec.channelsPerStream > kMaxOutBus) return kTooManyChannels;
    if (dry) return kNoDevice;
    const size_t nOut = nStreams * spec.channelsPerStream;
    PcmJob job;
    job.spec = spec; job.streams = streams; job.nStreams = nStreams;
    job.tally.init(nOut);
    const int rc = nOut ? renderHostSets(in, nIn, planar, nOut, numFrames, sampleTime, &job) : kOk;
    job.tally.writeTo(stats);
    return rc;
}

int Engine::processBlocksPcmIo(const PcmSource& src, void* const* outStreams, size_t nOutStreams, const PcmSpec* outSpec, float* const* planar,
                               size_t nPlanar, size_t numFrames, int64_t sampleTime, PcmChannelStats* stats) {
    const bool flacSrc = src.nStreams && src.format == flac_decode::kFormat;
    if (src.nStreams && ((!flacSrc && !pcm_pack::format_ok(src.format)) || src.channelsPerStream == 0u || !src.streams)) return kInvalidInstructionFormat;
    if (flacSrc) { const int rc = flacInCheck(src); if (rc != kOk) return rc; }
    if (outSpec ? (!pcm_pack::format_ok(outSpec->format) || outSpec->channelsPerStream == 0u || (nOutStreams && !outStreams)) : (nPlanar && !planar))
        return kInvalidInstructionFormat;
    for (size_t s = 0; s < src.nStreams; ++s) if (!src.streams[s] && numFrames) return kInvalidInstructionFormat;
    if (src.nStreams > kMaxHostIn || src.nStreams * (size_t)src.channelsPerStream > kMaxHostIn) return kTooManyChannels;
    if (outSpec ? (nOutStreams > kMaxOutBus || nOutStreams * (size_t)outSpec->channelsPerStream > kMaxOutBus) : nPlanar > kMaxOutBus) return kTooManyChannels;
    if (dry) return kNoDevice;
    const size_t nIn = src.nStreams * src.channelsPerStream;
    const PcmSource* from = src.nStreams ? &src : nullptr;
    if (!outSpec) return renderHostSets(nullptr, nIn, planar, nPlanar, numFrames, sampleTime, nullptr, from);
    const size_t nOut = nOutStreams * outSpec->channelsPerStream;
    PcmJob job;
    job.spec = *outSpec; job.streams = outStreams; job.nStreams = nOutStreams;
    job.tally.init(nOut);
    const int rc = nOut ? renderHostSets(nullptr, nIn, planar, nOut, numFrames, sampleTime, &job, from) : kOk;
    job.tally.writeTo(stats);
    return rc;
}

// what both renderers of a host-buffer call read: the arguments and everything derived from them and from the options, computed once
Engine::HostCall Engine::hostCall(const float* const* in, size_t nIn, float* const* out, size_t nOut, size_t numFrames, int64_t sampleTime, PcmJob* pcm,
                                  const PcmSource* src, FlacJob* flac) const {
    HostCall c{};
    c.in = in; c.nIn = nIn; c.out = out; c.nOut = nOut; c.numFrames = numFrames; c.sampleTime = sampleTime; c.pcm = pcm; c.src = src; c.flac = flac;
    c.bs = (size_t)blockSize;
    c.hb = (size_t)hostBlockSize;       // whole HOST blocks, like the reference's block loop (a host block = hostBlockSize / blockSize engine blocks)
    // a FLAC source (engine_flac_in.cpp) is decoded into the packed input half as the s16 / s24 stream of the same samples: from there
    // on it IS that PCM source
    c.flacSrc = src && src->format == flac_decode::kFormat;
    c.flacInB = c.flacSrc ? flacInBits(*src) : 0u;
    c.inMd5 = c.flacSrc && flacInMd5Opt != 0u;      // option "flac_in_md5": what the decoder restores enters the input slots' digests
    c.srcG = src ? src->channelsPerStream : 1u; c.srcFmt = c.flacSrc ? flac_decode::image_format(c.flacInB) : src ? src->format : 0u;
    c.srcB = src ? pcm_pack::sample_bytes(c.srcFmt) : 0;
    c.wantFloat = nOut > 0 && out != nullptr;
    c.pcmG = pcm ? pcm->spec.channelsPerStream : 1u; c.pcmFmt = pcm ? pcm->spec.format : 0u;
    c.pcmB = pcm ? pcm_pack::sample_bytes(c.pcmFmt) : 0;
    c.packed = pcm || flac;                 // (FLAC delivery stands where PCM delivery stands: nobody asked for the floats)
    c.meter = loudnessOn && nOut > 0;       // option "loudness_meter": the delivered frames of every set go through the meter
    // option "resample_rate": what is delivered — floats, packed streams, the meter's frames — is the render converted to the delivery
    // rate; the pack kernel's time (the dither's key) is then the programme's OUTPUT frame index
    c.resamp = resampleOn && nOut > 0;
    c.rp = resPlan;
    // option "limiter": the delivered frames — converted or not — go through the gain and the limiter before they are packed, metered
    // and copied; frames in = frames out, so neither the dither's key nor any count changes
    c.limit = limiterOn && nOut > 0;
    c.lmp = limPlan;
    // noiseShapeSet: the s16 / s24 codes of a PCM or FLAC delivery come from the error-feedback quantiser, behind the limiter; float
    // delivery and calls that deliver planar floats only are not quantised at all
    c.shape = nsTaps > 0u && nOut > 0 && (flac || (pcm && c.pcmFmt != pcm_pack::F32));
    c.shapeBits = flac ? flac->spec.bits : c.pcmFmt == pcm_pack::S16 ? 16u : 24u;
    c.shapeDither = flac ? (flac->spec.dither ? 1u : 0u) : pcm ? (pcm->spec.dither ? 1u : 0u) : 0u;
    c.shapeSeed = flac ? flac->spec.seed : pcm ? pcm->spec.seed : 0u;
    c.spectrum = spcOn && nOut > 0;         // spectrumSet: the delivered frames of every set go through the analyser, next to the meter
    c.qc = qcOn && nOut > 0;                // qcSet: and through the inspector
    // option "input_rate": the inputs — planar floats or streams — arrive at another rate and are converted to the engine's in front of
    // the render; a call of numFrames ENGINE frames pulls the input frames [inputs_before(n0), inputs_before(n0 + numFrames)) of the
    // programme. Planar floats count as nIn one-channel float streams: one path for both.
    c.inres = inResOn && nIn > 0;
    c.inp = inPlan;
    c.inG = src ? c.srcG : 1u; c.inFmt = src ? c.srcFmt : pcm_pack::F32;
    c.inStreams = src ? src->nStreams : nIn; c.inB = pcm_pack::sample_bytes(c.inFmt);
    // automationSet: the lanes as this call found them; their channels are the engine's inputs behind the supplied ones
    c.lanes = std::atomic_load(&autoLanes);
    c.nEng = c.lanes ? std::max<size_t>(nIn, c.lanes->inputs) : nIn;
    return c;
}

int Engine::renderHostSets(const float* const* in, size_t nIn, float* const* out, size_t nOut, size_t numFrames, int64_t sampleTime, PcmJob* pcm,
                           const PcmSource* src, FlacJob* flac) {
    const HostCall call = hostCall(in, nIn, out, nOut, numFrames, sampleTime, pcm, src, flac);
    const size_t bs = call.bs, hb = call.hb;
    if (call.lanes && nIn > call.lanes->lowest) return kInvalidPropertyValue;      // a supplied channel is bound to a lane: nothing is rendered
    bool tapSlices = hb % bs != 0;          // ragged slices (a host block that no k divides evenly): launch sets hold whole engine blocks
    if (hb != bs && !tapSlices) { std::lock_guard<std::mutex> lock(mu); tapSlices = !tapNodeIds.empty(); }
    if (tapSlices) return renderHostBlocks(call);     // (taps under a host block longer than the engine's: engine_host_blocks.cpp)
    // the launch-set loop, under the names it has always read the call by
    const bool flacSrc = call.flacSrc, wantFloat = call.wantFloat, packed = call.packed, meter = call.meter, resamp = call.resamp, limit = call.limit, inres = call.inres, shape = call.shape;
    const bool spectrum = call.spectrum, inspect = call.qc;
    const uint32_t flacInB = call.flacInB, srcG = call.srcG, srcFmt = call.srcFmt, pcmG = call.pcmG, pcmFmt = call.pcmFmt, inG = call.inG, inFmt = call.inFmt;
    const size_t srcB = call.srcB, pcmB = call.pcmB, inStreams = call.inStreams, inB = call.inB;
    const resample::Plan rp = call.rp, inp = call.inp;
    const limiter::Plan lmp = call.lmp;
    const AutoLanes* lanes = call.lanes.get();
    const size_t nEng = call.nEng;          // the rows of a block of the set's input: the supplied channels, then the lanes' (nIn without lanes)
    auto inStream = [&](size_t s) { return call.inStream(s); };
    const size_t numBlocks = ((numFrames + hb - 1) / hb) * (hb / bs);
    if (numBlocks == 0) return kOk;
    size_t setBlocks, outCapFrames = 0, outCapBlocks = 0;     // what a set delivers at most: frames, and whole blocks of the converted half
    uint64_t inN = 0;                                         // option "input_rate": the programme's engine frame at the next set's start
    size_t inOff = 0;                                         // ... and the input frames of this call consumed so far
    {
        RenderGuard lock(*this);
        if (hipSetDevice(device) != hipSuccess) return kHipError;
        setBlocks = (size_t)std::max(1, batchBlocks);
        if (setBlocks < 8) setBlocks = std::min<size_t>(64, numBlocks);     // per-block launch path: still stage whole chunks
        setBlocks = std::min(setBlocks, numBlocks);
        // launch sets hold whole HOST blocks: a newer render sequence is adopted at a set boundary (enqueueBlocks), and the reference
        // swaps sequences at host-block boundaries only (Runtime.h:277-285)
        if (hb > bs) setBlocks = std::min(numBlocks, std::max(hb / bs, setBlocks / (hb / bs) * (hb / bs)));
        auto deliveredBy = [&](size_t blocks) { return resamp ? (size_t)resample::ceil_div((uint64_t)(blocks * bs) * rp.L, rp.M) + 1 : blocks * bs; };
        if (spectrum) {
            // the frames one set completes must fit a pinned half: the largest whole number of host blocks whose frames do
            const size_t per = std::max<size_t>(hb / bs, 1), frameBytes = nOut * spcPlan.cols * sizeof(float);
            auto fits = [&](size_t blocks) { return spectrumSetFrames(deliveredBy(blocks)) <= kSpcHalfBytes / frameBytes; };
            while (setBlocks > per && !fits(setBlocks)) setBlocks = std::max(per, (setBlocks - 1) / per * per);
            if (!fits(setBlocks)) return kInvalidPropertyValue;
        }
        outCapFrames = deliveredBy(setBlocks);
        outCapBlocks = (outCapFrames + bs - 1) / bs;
        int rc = ensureHostStaging(std::max(setBlocks, outCapBlocks) * std::max<size_t>(nOut, 1) * bs, setBlocks * std::max<size_t>(nEng, 1) * bs);
        if (rc != kOk) return rc;
        if (resamp) {
            rc = ensureResample(nOut, outCapBlocks);
            if (rc != kOk) return rc;
        }
        if (limit) {
            rc = ensureLimiter(nOut, outCapBlocks, outCapFrames);
            if (rc != kOk) return rc;
        }
        if (inres) {
            // the packed halves hold the largest stretch a set can pull: ceil(frames M / L) + 1 input frames of every stream
            const uint64_t maxIn = resample::ceil_div((uint64_t)(setBlocks * bs) * inp.M, inp.L) + 1u;
            if (maxIn > 0xFFFFFFFFull) return kInvalidPropertyValue;      // (the kernels count a set's frames in 32 bits)
            rc = ensureInputResample(nIn);
            if (rc != kOk) return rc;
            rc = growPackedHalves(hPcmIn, dPcmIn, pcmInBytes, inStreams * (size_t)pcm_pack::stream_stride(maxIn, inG, inFmt));
            if (rc != kOk) return rc;
            inN = inFramesOut;
        } else if (src) {
            rc = ensurePcmInStaging(src->nStreams * (size_t)pcm_pack::stream_stride(setBlocks * bs, srcG, srcFmt), srcG);
            if (rc != kOk) return rc;
        }
        if (flacSrc) {
            // the FLAC halves, the descriptors and the scratch hold the largest covering range of any set of this call: sized from the table
            size_t staged = 0, frames = 0, scratch = 0;
            FlacInSet probe;
            const size_t sets = (numBlocks + setBlocks - 1) / setBlocks;
            for (size_t k = 0; k < sets; ++k) {
                const uint64_t e0 = std::min<uint64_t>(k * setBlocks * bs, numFrames), e1 = std::min<uint64_t>((k + 1) * setBlocks * bs, numFrames);
                const uint64_t base = inres ? resample::inputs_before(inp, inN) : 0;
                const uint64_t i0 = inres ? resample::inputs_before(inp, inN + e0) - base : e0, i1 = inres ? resample::inputs_before(inp, inN + e1) - base : e1;
                flacInPlan(*src, i0, (size_t)(i1 - i0), probe, call.inMd5);
                staged = std::max(staged, probe.stagedBytes); frames = std::max(frames, probe.frames.size()); scratch = std::max(scratch, probe.scratchInts);
            }
            rc = ensureFlacIn(staged, std::max<size_t>(frames, 1), std::max<size_t>(scratch, 1), srcG);
            if (rc != kOk) return rc;
            if (flacInMd5Slots.size() < src->nStreams) flacInMd5Slots.resize(src->nStreams, flac_in_md5::Slot{});      // (slot s is input stream s, hashed or not)
            if (call.inMd5) { rc = ensureFlacInMd5(); if (rc != kOk) return rc; }
        }
        if (pcm) {
            rc = ensurePcmStaging(pcm->nStreams * (size_t)pcm_pack::stream_stride(outCapFrames, pcmG, pcmFmt) + nOut * sizeof(pcm_pack::ChannelStats), pcmG);
            if (rc != kOk) return rc;
        }
        if (meter) {
            rc = ensureLoudness(nOut, outCapFrames);
            if (rc != kOk) return rc;
        }
        if (spectrum) {
            rc = ensureSpectrum(nOut, spectrumSetFrames(outCapFrames));
            if (rc != kOk) return rc;
        }
        if (inspect) {
            rc = ensureQc(nOut, outCapFrames);
            if (rc != kOk) return rc;
        }
        if (flac) {
            rc = ensureFlac(*flac, outCapFrames);
            if (rc != kOk) return rc;
        }
        if (shape) {
            rc = ensureNoiseShape(nOut, std::max(setBlocks, outCapBlocks) * nOut * bs);
            if (rc != kOk) return rc;
        }
    }
    int flacRc = kOk;
    const size_t numSets = (numBlocks + setBlocks - 1) / setBlocks;
    // One thread copies ~10 GB/s; a set of many channels (C4: 128 outputs x 1024 blocks = 268 MB per 12.6 ms of rendering)
    // needs more than that to stay hidden behind the next set, so big sets are cut over a few threads.
    auto spread = [&](size_t bytes, size_t maxParts, const std::function<void(size_t, size_t)>& part) {      // part(t, threads)
        size_t threads = bytes >= (16u << 20) ? std::min<size_t>(8, std::max<size_t>(1, std::thread::hardware_concurrency() / 4)) : 1;
        threads = std::min(threads, maxParts);
        if (threads <= 1) return part(0, 1);
        std::vector<std::thread> pool;
        for (size_t t = 1; t < threads; ++t) pool.emplace_back(part, t, threads);
        part(0, threads);
        for (auto& th : pool) th.join();
    };
    auto scatter = [&](size_t k) {     // pinned half -> the caller's planar arrays (by block range)
        const size_t b0 = k * setBlocks, nb = std::min(setBlocks, numBlocks - b0);
        const float* src = hStageOut[k & 1];
        spread(nb * nOut * bs * sizeof(float), nb, [&](size_t t, size_t threads) {
            for (size_t b = nb * t / threads; b < nb * (t + 1) / threads; ++b) {
                const size_t f0 = (b0 + b) * bs;
                if (f0 >= numFrames) break;                     // (the engine blocks that only fill up the last host block)
                const size_t n = std::min(bs, numFrames - f0);
                for (size_t c = 0; c < nOut; ++c) std::memcpy(out[c] + f0, src + (b * nOut + c) * bs, n * sizeof(float));
            }
        });
    };
    auto scatterConverted = [&](size_t k) {     // the same for a converted set: its frames go where the call's earlier sets ended
        const size_t valid = resValidOf[k & 1], at = (size_t)resOffsetOf[k & 1], nb = (valid + bs - 1) / bs;
        const float* src = hStageOut[k & 1];
        spread(nb * nOut * bs * sizeof(float), nb, [&](size_t t, size_t threads) {
            for (size_t b = nb * t / threads; b < nb * (t + 1) / threads; ++b) {
                const size_t n = std::min(bs, valid - b * bs);
                for (size_t c = 0; c < nOut; ++c) std::memcpy(out[c] + at + b * bs, src + (b * nOut + c) * bs, n * sizeof(float));
            }
        });
    };
    auto deliverPcm = [&](size_t k) {  // pinned packed half -> the caller's streams (one contiguous stretch per stream), statistics summed
        const size_t valid = pcm->validOf[k & 1], f0 = resamp ? (size_t)resOffsetOf[k & 1] : k * setBlocks * bs;
        const size_t stride = (size_t)pcm_pack::stream_stride(valid, pcmG, pcmFmt), len = valid * pcmG * pcmB;
        const unsigned char* src = hPcm[k & 1];
        spread(pcm->nStreams * len, len / 4096 + 1, [&](size_t t, size_t threads) {
            const size_t lo = len * t / threads, hi = len * (t + 1) / threads;
            for (size_t s = 0; s < pcm->nStreams; ++s)
                std::memcpy(static_cast<unsigned char*>(pcm->streams[s]) + f0 * pcmG * pcmB + lo, src + s * stride + lo, hi - lo);
        });
        const pcm_pack::ChannelStats* st = reinterpret_cast<const pcm_pack::ChannelStats*>(src + pcm->nStreams * stride);
        for (size_t c = 0; c < nOut; ++c) {
            pcm->tally.peakBits[c] = std::max(pcm->tally.peakBits[c], st[c].peakBits);
            pcm->tally.over[c] += st[c].over; pcm->tally.nonfinite[c] += st[c].nonfinite;
        }
    };
    auto deliverLoudness = [&](size_t k) {   // the sums of the sub-blocks set k completed -> the programme's series
        const double* sums = hLoudOut[k & 1];
        std::lock_guard<std::mutex> lock(mu);
        for (size_t c = 0; c < nOut; ++c)
            for (uint32_t j = 0; j < loudCountOf[k & 1]; ++j) loudSeries[c].push_back(sums[c * loudOutStride + j] / (double)loudPlan.hop);
    };
    auto deliverSpectrum = [&](size_t k) {   // the frames set k completed -> the queue spectrumRead drains
        const size_t count = spcCountOf[k & 1], cols = spcPlan.cols;
        const float* frames = hSpcOut[k & 1];
        std::lock_guard<std::mutex> lock(mu);
        for (size_t c = 0; c < nOut && count; ++c) spcQueue[c].insert(spcQueue[c].end(), frames + c * count * cols, frames + (c + 1) * count * cols);
    };
    auto deliverQc = [&](size_t k) {         // the buckets set k completed -> the queue qcOverview drains
        const size_t count = qcCountOf[k & 1];
        const float* buckets = hQcOut[k & 1];
        std::lock_guard<std::mutex> lock(mu);
        for (size_t c = 0; c < nOut && count; ++c) qcQueue[c].insert(qcQueue[c].end(), buckets + c * count * 2u, buckets + (c + 1) * count * 2u);
    };
    auto deliver = [&](size_t k) { if (wantFloat) { if (resamp) scatterConverted(k); else scatter(k); } if (pcm) deliverPcm(k); if (meter) deliverLoudness(k);
                                  if (spectrum) deliverSpectrum(k);
                                  if (inspect) deliverQc(k);
                                  if (flac && flacRc == kOk) flacRc = flacDeliver(*flac, (int)(k & 1)); };
    int result = kOk;
    size_t issued = 0, scattered = 0, outOff = 0;
    // a failing HIP call ends the loop; the tail below drains both streams, releases what was deferred and reports the code —
    // `out` then holds the sets scattered so far (whole launch sets, in order), nothing is left in flight
#define HOST_TRY(call) { if ((call) != hipSuccess) { std::fprintf(stderr, "[elemhip] %s failed: %s\n", #call, hipGetErrorString(hipGetLastError())); result = kHipError; break; } }
    for (size_t k = 0; k < numSets; ++k) {
        const size_t b0 = k * setBlocks, nb = std::min(setBlocks, numBlocks - b0);
        const int half = (int)(k & 1);
        // (sets hold whole host blocks, so a set starts in front of numFrames)
        const size_t srcValid = src ? std::min(nb * bs, numFrames - b0 * bs) : 0, srcStride = src ? (size_t)pcm_pack::stream_stride(srcValid, srcG, srcFmt) : 0;
        // option "input_rate": the set's engine frames [inN, inN + inOut) pull the input frames [inT0, inT0 + inValid), which start at the
        // call's input cursor
        const size_t inOut = inres ? std::min(nb * bs, numFrames - b0 * bs) : 0;
        const uint64_t inT0 = inres ? resample::inputs_before(inp, inN) : 0;
        const size_t inValid = inres ? (size_t)(resample::inputs_before(inp, inN + inOut) - inT0) : 0;
        const size_t inStride = inres ? (size_t)pcm_pack::stream_stride(inValid, inG, inFmt) : 0;
        if (nIn) {
            if (k >= 2) HOST_TRY(hipEventSynchronize(evIn[half]));     // the H2D of set k - 2 has left this pinned half
            if (flacSrc) {
                // the FLAC frames that cover the set's input frames, found by binary search in the streams' tables, as they lie in the
                // caller's buffers: the compressed bytes and nothing more
                flacInPlan(*src, inres ? inOff : b0 * bs, inres ? inValid : srcValid, flacInSets[half], call.inMd5);
                if (flacInSets[half].stagedBytes > flacInBytes) { result = kInvariantViolation; break; }      // (sized above from the same table)
                flacInStage(*src, flacInSets[half], half);
            } else if (inres) {
                // one contiguous stretch per stream (per planar array): the input-rate bytes and nothing more
                const size_t len = inValid * inG * inB;
                unsigned char* dst = hPcmIn[half];
                spread(inStreams * len, len / 4096 + 1, [&](size_t t, size_t threads) {
                    const size_t lo = len * t / threads, hi = len * (t + 1) / threads;
                    for (size_t s = 0; s < inStreams; ++s) std::memcpy(dst + s * inStride + lo, inStream(s) + inOff * inG * inB + lo, hi - lo);
                });
            } else if (src) {
                // one contiguous stretch per stream: the set's valid frames, as they lie in the caller's streams
                const size_t len = srcValid * srcG * srcB;
                unsigned char* dst = hPcmIn[half];
                spread(src->nStreams * len, len / 4096 + 1, [&](size_t t, size_t threads) {
                    const size_t lo = len * t / threads, hi = len * (t + 1) / threads;
                    for (size_t s = 0; s < src->nStreams; ++s)
                        std::memcpy(dst + s * srcStride + lo, static_cast<const unsigned char*>(src->streams[s]) + b0 * bs * srcG * srcB + lo, hi - lo);
                });
            }
            float* dst = hStageIn[half];
            for (size_t b = 0; b < nb && !src && !inres; ++b) {
                const size_t f0 = (b0 + b) * bs;
                const size_t n = f0 < numFrames ? std::min(bs, numFrames - f0) : 0;
                for (size_t c = 0; c < nIn; ++c) {
                    float* d = dst + (b * nIn + c) * bs;
                    if (n) std::memcpy(d, in[c] + f0, n * sizeof(float));
                    if (n < bs) std::memset(d + n, 0, (bs - n) * sizeof(float));
                }
            }
        }
        {
            RenderGuard lock(*this);
            if (hipSetDevice(device) != hipSuccess) { result = kHipError; break; }
            if (nIn) {
                // (the copy stream is in order: this H2D runs behind the D2H of set k - 2, which waited for that set's render,
                //  the last reader of this device half)
                if (call.inMd5) flacInMd5Jobs(*src, flacInSets[half], half);      // (the jobs ride in the staged half, behind the bytes)
                if (flacSrc) { if (flacInSets[half].stagedBytes) HOST_TRY(hipMemcpyAsync(dFlacIn[half], hFlacIn[half], flacInSets[half].stagedBytes, hipMemcpyHostToDevice, ioStream)); }
                else if (inres) { if (inStreams * inStride) HOST_TRY(hipMemcpyAsync(dPcmIn[half], hPcmIn[half], inStreams * inStride, hipMemcpyHostToDevice, ioStream)); }
                else if (src) HOST_TRY(hipMemcpyAsync(dPcmIn[half], hPcmIn[half], src->nStreams * srcStride, hipMemcpyHostToDevice, ioStream))
                else if (lanes)      // (the supplied rows of every block: the lanes' rows behind them are the kernel's, below)
                    HOST_TRY(hipMemcpy2DAsync(dStageIn[half], nEng * bs * sizeof(float), hStageIn[half], nIn * bs * sizeof(float), nIn * bs * sizeof(float), nb,
                                              hipMemcpyHostToDevice, ioStream))
                else HOST_TRY(hipMemcpyAsync(dStageIn[half], hStageIn[half], nb * nIn * bs * sizeof(float), hipMemcpyHostToDevice, ioStream));
                HOST_TRY(hipEventRecord(evIn[half], ioStream));
                HOST_TRY(hipStreamWaitEvent(stream, evIn[half], 0));
                if (flacSrc) {
                    // the decode kernels write the packed input half the H2D of a PCM stream would have filled. The half was last read by
                    // the unpack (or the converter) of set k - 2, earlier on this stream; the FLAC half by that set's decode, and its H2D
                    // ran behind the D2H of set k - 2 like every other; the scratch is touched by this stream's kernels only.
                    const int rf = flacInLaunch(flacInSets[half], half, srcG, flacInB, inres ? inValid : srcValid, inres ? inStride : srcStride);
                    if (rf != kOk) { result = rf; break; }
                    // option "flac_in_md5": directly behind the decode kernels, which left the samples in the scratch; the next set's
                    // parse, the scratch's next writer, runs behind it on this stream. Nothing waits for it.
                    if (call.inMd5) { const int rm = flacInMd5Launch(flacInSets[half], half, srcG, flacInB); if (rm != kOk) { result = rm; break; } }
                }
                if (inres) {
                    // the input converter in the unpack kernel's place, and the argument below holds for it word for word: dStageIn[half]
                    // and dPcmIn[half] are free for the same reasons, and it too writes every row of all nb blocks, zeros behind inOut.
                    // It reads one copy of the carried frames and its history step writes the other; the kernels of set k - 1 that read
                    // the copy now written ran earlier on this stream.
                    ResampleInArgs a{};
                    a.src = dPcmIn[half]; a.dst = dStageIn[half]; a.histIn = dInHist[inHistCur]; a.histOut = dInHist[inHistCur ^ 1];
                    a.table = dInTable; a.rowBase = dInRowBase; a.t0 = inT0; a.n0 = inN; a.streamStride = inStride;
                    a.blockSize = (uint32_t)bs; a.numChannels = (uint32_t)nEng; a.G = inG; a.numStreams = (uint32_t)inStreams;
                    a.validIn = (uint32_t)inValid; a.validOut = (uint32_t)inOut; a.numBlocks = (uint32_t)nb; a.plan = inp;
                    HOST_TRY(launch_resample_in(stream, a, inFmt));
                    inHistCur ^= 1;
                    inN += inOut; inOff += inValid;
                    inFramesOut = inN; inFramesIn = inT0 + inValid;
                } else if (src) {
                    // the unpack kernel in front of the set's first level, on the render's stream. Both halves it touches are free:
                    // dStageIn[half] was last read by the render of set k - 2, earlier on this stream; dPcmIn[half] was last read by
                    // the unpack of set k - 2, earlier on this stream too, and the H2D that refilled it ran behind the D2H of set
                    // k - 1 on the copy stream, which waited for evRendered of that set — recorded behind both. The kernel writes every
                    // row of all nb blocks, zeros behind srcValid: nothing of set k - 2 is left in the half.
                    PcmUnpackArgs a{};
                    a.src = dPcmIn[half]; a.dst = dStageIn[half]; a.rowBase = dPcmInRowBase; a.streamStride = srcStride;
                    a.blockSize = (uint32_t)bs; a.numChannels = (uint32_t)nEng; a.G = srcG; a.numStreams = (uint32_t)src->nStreams;
                    a.validFrames = (uint32_t)srcValid; a.numBlocks = (uint32_t)nb; a.tilesPerBlock = pcm_pack::tiles_per_block((uint32_t)bs, srcG);
                    a.rowDwords = pcmInRowDwords;
                    HOST_TRY(launch_pcm_unpack(stream, a, srcFmt));
                }
            }
            if (lanes) {
                // the lanes' kernel in front of the set's first level, on the render's stream, next to the unpack kernel: it writes the
                // rows of channels [nIn, nEng) of all nb blocks — the lanes' values, zeros for a channel without a lane and behind the
                // call's last frame — and nothing else, the H2D and the kernels above write the rows in front of them and nothing else.
                // dStageIn[half] was last read by the render of set k - 2, earlier on this stream. It reads the tables only, which the
                // call holds.
                AutomationArgs a{};
                a.dst = dStageIn[half]; a.points = lanes->dev; a.numPoints = lanes->points.size(); a.time0 = sampleTime + (int64_t)(b0 * bs);
                a.validFrames = std::min(nb * bs, numFrames - b0 * bs);
                a.blockSize = (uint32_t)bs; a.numChannels = (uint32_t)nEng; a.firstChannel = (uint32_t)nIn; a.numBlocks = (uint32_t)nb;
                std::memcpy(a.offset, lanes->offset, sizeof a.offset); std::memcpy(a.count, lanes->count, sizeof a.count);
                HOST_TRY(launch_automation(stream, a));
            }
            if (k >= 2) HOST_TRY(hipStreamWaitEvent(stream, evOut[half], 0));   // the D2H of set k - 2 has drained this device half
            int rc = enqueueBlocks(nEng ? dStageIn[half] : nullptr, nEng, nOut ? dStageOut[half] : nullptr, nOut, nb,
                                   sampleTime + (int64_t)(b0 * bs));
            if (rc != kOk) { result = rc; break; }
            if (hb > bs) {                                      // (whole host blocks of hb / bs slices each: where each one ended, for the event relay)
                const uint64_t per = hb / bs, base = st.blocksRendered - nb;
                for (uint64_t e = per; e <= nb; e += per) { if (hostBlockEnds.size() >= 65536) hostBlockEnds.pop_front(); hostBlockEnds.push_back(base + e); }
            }
            // what the set delivers: its valid frames where the levels left them, or their conversion
            const float* got = dStageOut[half];
            size_t valid = std::min(nb * bs, numFrames - b0 * bs), gotBlocks = nb;
            int64_t gotTime = sampleTime + (int64_t)(b0 * bs);
            if (resamp) {
                // the converter behind the set's last level, in front of the pack kernel and the meter, on the same stream: it reads the
                // block that is still warm in L2 and one copy of the carried frames, its history step writes the other copy. The converted
                // half was drained by the D2H of set k - 2 (evOut above).
                ResampleArgs a{};
                a.src = dStageOut[half]; a.dst = dRes[half]; a.histIn = dResHist[resHistCur]; a.histOut = dResHist[resHistCur ^ 1];
                a.table = dResTable; a.rowBase = dResRowBase; a.t0 = resFramesIn; a.n0 = resFramesOut;
                a.blockSize = (uint32_t)bs; a.numChannels = (uint32_t)nOut; a.validIn = (uint32_t)valid;
                a.validOut = (uint32_t)(resample::outputs_before(rp, resFramesIn + valid) - resFramesOut);
                a.outBlocks = (uint32_t)((a.validOut + bs - 1) / bs); a.outBlocksCap = (uint32_t)outCapBlocks; a.plan = rp;
                HOST_TRY(launch_resample(stream, a));
                resHistCur ^= 1;
                resValidOf[half] = a.validOut; resOffsetOf[half] = outOff;
                got = dRes[half]; gotBlocks = a.outBlocks; gotTime = (int64_t)resFramesOut;
                resFramesIn += valid; resFramesOut += a.validOut;
                valid = a.validOut; outOff += valid;
            }
            if (limit && valid) {
                // the limiter behind the converter, in front of the pack kernel and the meter, on the same stream: it reads one copy of
                // its carried state, its history step writes the other. The limited half was drained by the D2H of set k - 2 (evOut above).
                LimiterArgs a{};
                a.src = got; a.dst = dLim[half]; a.stateIn = dLimState[limCur]; a.stateOut = dLimState[limCur ^ 1]; a.stats = dLimStats;
                a.frames = dLimFrames; a.tiles = dLimTiles; a.n0 = limFrames;
                a.blockSize = (uint32_t)bs; a.numChannels = (uint32_t)nOut; a.validFrames = (uint32_t)valid;
                a.outBlocks = (uint32_t)gotBlocks; a.outBlocksCap = (uint32_t)outCapBlocks; a.frameCap = (uint32_t)limFrameCap; a.tileCap = (uint32_t)limTileCap;
                a.plan = lmp; a.meter = limMeter;
                HOST_TRY(launch_limiter(stream, a));
                limCur ^= 1;
                got = dLim[half];
                limFrames += valid;
            }
            const int32_t* shaped = nullptr;
            if (shape && valid) {
                // the error-feedback quantiser behind the limiter, in front of the pack kernel or the FLAC stage kernel, on the same
                // stream: all of the set's delivered frames (a FLAC call's `drop` discards codes, not state) at the dither's time. The
                // states are updated in place and the codes lie in one buffer: this stream's kernels touch them, in order, nobody else.
                NoiseShapeArgs a{};
                a.src = got; a.dst = dNsCodes; a.state = dNsState; a.time0 = gotTime;
                a.blockSize = (uint32_t)bs; a.numChannels = (uint32_t)nOut; a.validFrames = (uint32_t)valid;
                a.bits = call.shapeBits; a.dither = call.shapeDither; a.seed = call.shapeSeed; a.taps = nsTaps;
                std::memcpy(a.cq, nsCq, sizeof a.cq);
                HOST_TRY(launch_noise_shape(stream, a));
                shaped = dNsCodes;
                nsFrames += valid;
            }
            size_t pcmCopy = 0;
            if (pcm) {
                // the pack kernel behind the set's last level, on the same stream: the output block is still warm in L2. Its packed
                // half was drained by the D2H of set k - 2 (evOut above).
                const size_t stride = (size_t)pcm_pack::stream_stride(valid, pcmG, pcmFmt), statsOff = pcm->nStreams * stride;
                pcm->validOf[half] = (uint32_t)valid;
                HOST_TRY(hipMemsetAsync(dPcm[half] + statsOff, 0, nOut * sizeof(pcm_pack::ChannelStats), stream));
                PcmPackArgs a{};
                a.src = got; a.dst = dPcm[half]; a.stats = reinterpret_cast<pcm_pack::ChannelStats*>(dPcm[half] + statsOff);
                a.rowBase = dPcmRowBase; a.time0 = gotTime; a.streamStride = stride;
                a.blockSize = (uint32_t)bs; a.numChannels = (uint32_t)nOut; a.G = pcmG; a.numStreams = (uint32_t)pcm->nStreams;
                a.validFrames = (uint32_t)valid; a.tilesPerBlock = pcm_pack::tiles_per_block((uint32_t)bs, pcmG); a.rowDwords = pcmRowDwords;
                a.dither = pcm->spec.dither ? 1u : 0u; a.seed = pcm->spec.seed; a.shaped = shaped;
                HOST_TRY(launch_pcm_pack(stream, a, pcmFmt));
                pcmCopy = statsOff + nOut * sizeof(pcm_pack::ChannelStats);
            }
            if (flac) {
                // the FLAC kernels in the pack kernel's place, on the same stream: the carried codes and the set's, quantised, behind one
                // another per channel; every whole frame among them encoded and assembled; what is left over is the next set's carry.
                // The codes, the slots and the carry are touched by this stream's kernels only, in order; the packed half was drained by
                // the D2H of set k - 2 (evOut above) and its payload copy, which the host waited for before it delivered that set.
                const uint64_t lead = std::min<uint64_t>(flac->dropLeft, valid), enter = std::min<uint64_t>(flac->takeLeft, valid - lead);
                flac->dropLeft -= lead; flac->takeLeft -= enter;
                const uint32_t ff = flacFF, total = flacOpen + (uint32_t)enter, nF = total / ff, rem = total % ff;
                if (flacEmitted + nF > 0x7FFFFFFFull) { result = kInvariantViolation; break; }
                flac->framesOf[half] = nF;
                pcm_pack::ChannelStats* fst = reinterpret_cast<pcm_pack::ChannelStats*>(dPcm[half] + flac->statsOff);
                HOST_TRY(hipMemsetAsync(fst, 0, nOut * sizeof(pcm_pack::ChannelStats), stream));
                FlacStageArgs sa{};
                sa.src = got; sa.carry = dFlacCarry; sa.codes = dFlacCodes; sa.stats = fst; sa.time0 = gotTime;
                sa.blockSize = (uint32_t)bs; sa.numChannels = (uint32_t)nOut; sa.validFrames = (uint32_t)enter; sa.srcOffset = (uint32_t)lead; sa.open = flacOpen;
                sa.cap = (uint32_t)flacCodesCap; sa.bits = flac->spec.bits; sa.dither = flac->spec.dither ? 1u : 0u; sa.seed = flac->spec.seed; sa.shaped = shaped;
                HOST_TRY(launch_flac_stage(stream, sa));
                // the codes that entered with this set go into their streams' MD5 where they lie (the carried ones did when they were staged)
                if (flacMd5 && enter > 0u) { const int rm = flacMd5Launch(flacOpen, (uint32_t)enter, false); if (rm != kOk) { result = rm; break; } }
                FlacEncodeArgs ea{};
                ea.codes = dFlacCodes; ea.slots = dFlacSlots; ea.subBits = dFlacSubBits; ea.dst = dPcm[half] + flac->payloadOff;
                ea.frameBytes = reinterpret_cast<uint32_t*>(dPcm[half]); ea.streamStride = flac->stride; ea.cap = (uint32_t)flacCodesCap;
                ea.G = flac->spec.channelsPerStream; ea.numStreams = (uint32_t)flac->nStreams; ea.bits = flac->spec.bits; ea.flacFrame = ff; ea.n = ff;
                ea.numFrames = nF; ea.slotWords = flac_encode::slot_words(ff, flac->spec.bits); ea.rate = flacRate; ea.firstNumber = (uint32_t)flacEmitted;
                ea.lpcOrder = flacLpc;
                HOST_TRY(launch_flac_encode(stream, ea));
                HOST_TRY(launch_flac_carry(stream, dFlacCodes, dFlacCarry, (uint32_t)nOut, (uint32_t)flacCodesCap, ff, nF * ff, rem));
                flacOpen = rem; flacEmitted += nF; flacFrames += enter;
            }
            if (meter) {
                // the meter's kernels behind the set's last level too, next to the pack kernel: they read the same block. The state they
                // carry lives on the device; the sums of the sub-blocks this set completes go to this half's small region, drained like
                // the packed half by the D2H of set k - 2.
                LoudnessArgs a{};
                a.src = got; a.state = dLoudState; a.segState = dLoudSeg; a.segEnergy = dLoudEnergy; a.out = dLoudOut[half];
                a.blockSize = (uint32_t)bs; a.numChannels = (uint32_t)nOut; a.validFrames = (uint32_t)valid;
                a.numSegs = loudness::segment_count((uint32_t)valid, loudPlan.L); a.segCap = (uint32_t)loudSegCap; a.outStride = (uint32_t)loudOutStride;
                a.q0 = (uint32_t)(loudFrames % loudPlan.hop); a.plan = loudPlan;
                loudCountOf[half] = loudness::subblocks_complete(a.q0, a.validFrames, loudPlan.hop);
                HOST_TRY(launch_loudness(stream, a));
                loudFrames += valid;
            }
            if (spectrum) {
                // the analyser's kernels behind the set's last level too, next to the meter: they read the same block. One copy of the
                // carried frames is read, the carry step writes the other; the sums are added to in place by this stream's kernels
                // only; the frames this set completes go to this half's region, drained by the D2H of set k - 2 (evOut above).
                SpectrumArgs a{};
                a.src = got; a.tailIn = dSpcTail[spcTailCur]; a.tailOut = dSpcTail[spcTailCur ^ 1]; a.out = dSpcOut[half]; a.sums = dSpcSums;
                a.n0 = spcFrames; a.j0 = spcEmitted;
                a.numFrames = (uint32_t)(spectrum::frames_complete(spcFrames + valid, spcPlan.size, spcPlan.hop, spcPlan.pad) - spcEmitted);
                a.validFrames = (uint32_t)valid; a.blockSize = (uint32_t)bs; a.numChannels = (uint32_t)nOut; a.updateTail = valid ? 1u : 0u;
                a.plan = spcPlanDev;
                if (a.numFrames > spcOutCap) { result = kInvariantViolation; break; }       // (sized above for the largest set)
                spcCountOf[half] = a.numFrames;
                if (valid) {
                    HOST_TRY(launch_spectrum(stream, a));
                    spcTailCur ^= 1;
                    spcFrames += valid; spcEmitted += a.numFrames;
                }
            }
            if (inspect) {
                // the inspector's kernels behind the set's last level too: they read the same block. The programme's summaries live on
                // the device and are folded in place by this stream's kernels only; the overview buckets this set completes go to this
                // half's region, drained by the D2H of set k - 2 (evOut above).
                const qc::Window w = qc::window(qcDelivered, qcFrames, qcSkip, qcLimit, valid);
                QcArgs a{};
                a.src = got; a.state = dQcState; a.pairState = dQcPairState; a.pairs = dQcPairs; a.tileStretch = dQcTiles; a.leafSums = dQcLeaves;
                a.tileEdge = dQcEdges; a.out = dQcOut[half]; a.p0 = qcFrames; a.q0 = w.q0; a.count = w.count; a.blockSize = (uint32_t)bs;
                a.numChannels = (uint32_t)nOut; a.numPairs = (uint32_t)(qcPairs.size() / 2u); a.numTiles = qc::tile_count(a.p0, a.count);
                a.tileCap = (uint32_t)(qcSetCap / qc::kTileFrames + 2u); a.leafCap = (uint32_t)(qcSetCap / qc::kLeaf + 2u);
                a.outCount = qc::buckets_complete(a.p0, a.count, qcSpec.bucket); a.spec = qcSpec;
                if (a.outCount > qcOutCap || valid > qcSetCap) { result = kInvariantViolation; break; }       // (sized above for the largest set)
                qcCountOf[half] = a.outCount;
                HOST_TRY(launch_qc(stream, a));
                qcDelivered += valid; qcFrames += w.count;
            }
            HOST_TRY(hipEventRecord(evRendered[half], stream));
            HOST_TRY(hipStreamWaitEvent(ioStream, evRendered[half], 0));
            if (flacSrc) HOST_TRY(hipMemcpyAsync(hFlacInErr + half, dFlacInErr + half, sizeof(FlacInError), hipMemcpyDeviceToHost, ioStream));   // the decode's error record
            if (call.inMd5 && flacInSets[half].md5Finish) {     // the digests this set finished come back with it
                bool ok = true;
                for (size_t s = 0; s < flacInSets[half].jobs.size() && ok; ++s)
                    if (flacInSets[half].jobs[s].finish) ok = hipMemcpyAsync(hFlacInMd5 + 16u * s, flacInMd5Digests() + 16u * s, 16u, hipMemcpyDeviceToHost, ioStream) == hipSuccess;
                if (!ok) { result = kHipError; break; }
            }
            if (wantFloat || !packed) { if (nOut && gotBlocks) HOST_TRY(hipMemcpyAsync(hStageOut[half], got, gotBlocks * nOut * bs * sizeof(float), hipMemcpyDeviceToHost, ioStream)); }
            if (pcm) HOST_TRY(hipMemcpyAsync(hPcm[half], dPcm[half], pcmCopy, hipMemcpyDeviceToHost, ioStream));
            if (flac) {     // the length table and the statistics; the frames follow once the table says how many bytes they are (flacDeliver)
                const size_t tab = flac->nStreams * (size_t)flac->framesOf[half] * sizeof(uint32_t);
                if (tab) HOST_TRY(hipMemcpyAsync(hPcm[half], dPcm[half], tab, hipMemcpyDeviceToHost, ioStream));
                HOST_TRY(hipMemcpyAsync(hPcm[half] + flac->statsOff, dPcm[half] + flac->statsOff, nOut * sizeof(pcm_pack::ChannelStats), hipMemcpyDeviceToHost, ioStream));
            }
            if (meter && loudCountOf[half]) HOST_TRY(hipMemcpyAsync(hLoudOut[half], dLoudOut[half], nOut * loudOutStride * sizeof(double), hipMemcpyDeviceToHost, ioStream));
            if (spectrum && spcCountOf[half])
                HOST_TRY(hipMemcpyAsync(hSpcOut[half], dSpcOut[half], nOut * spcCountOf[half] * spcPlan.cols * sizeof(float), hipMemcpyDeviceToHost, ioStream));
            if (inspect && qcCountOf[half]) HOST_TRY(hipMemcpyAsync(hQcOut[half], dQcOut[half], nOut * qcCountOf[half] * 2u * sizeof(float), hipMemcpyDeviceToHost, ioStream));
            HOST_TRY(hipEventRecord(evOut[half], ioStream));
            issued = k + 1;
        }
        if (k >= 1) {   // set k - 1 arrives while set k renders
            HOST_TRY(hipEventSynchronize(evOut[(k - 1) & 1]));
            if (flacSrc && flacInFailed((int)((k - 1) & 1))) { result = kFlacInput; break; }      // a frame of set k - 1 did not decode: nothing further
            if (nOut) deliver(k - 1);
            scattered = k;
            if (flacRc != kOk) { result = flacRc; break; }
        }
    }
#undef HOST_TRY
    if (issued > scattered && result == kOk) {       // the last set (every earlier one was scattered while its successor rendered)
        const size_t last = issued - 1;
        if (hipEventSynchronize(evOut[last & 1]) != hipSuccess) result = kHipError;
        else if (flacSrc && flacInFailed((int)(last & 1))) result = kFlacInput;
        else if (nOut) deliver(last);
        if (flacRc != kOk) result = flacRc;
    }
    {
        RenderGuard lock(*this);
        if (hipStreamSynchronize(stream) != hipSuccess) result = result == kOk ? kHipError : result;
        if (hipStreamSynchronize(ioStream) != hipSuccess) result = result == kOk ? kHipError : result;
        if (hipGetLastError() != hipSuccess && result == kOk) result = kHipError;
        if (profUsed) profCollect();
        freeDeferred();
        // a metered call that failed may have advanced the carried state past sets whose sums never arrived: the programme starts anew
        if (meter && result != kOk) (void)loudnessResetLocked(loudChannels);
        if (spectrum && result != kOk) (void)spectrumResetLocked(spcChannels);      // the same for the analyser's
        if (inspect && result != kOk) (void)qcResetLocked(qcChannels);             // and the inspector's
        if (resamp && result != kOk) (void)resampleResetLocked(0);      // likewise: the clock may be ahead of what was delivered
        if (limit && result != kOk) (void)limiterResetLocked(0);
        if (shape && result != kOk) (void)noiseShapeResetLocked();
        if (inres && result != kOk) (void)inputResampleResetLocked(0);   // and the input programme: its clock may be ahead of what was rendered
        // a call that failed for another reason than a frame that did not decode may have left records and slots apart: the slots break
        if (call.inMd5 && result != kOk && result != kFlacInput) for (flac_in_md5::Slot& sl : flacInMd5Slots) if (sl.state != flac_in_md5::kOff) sl.state = flac_in_md5::kBroken;
    }
    return result;
}

} // namespace elemhip
