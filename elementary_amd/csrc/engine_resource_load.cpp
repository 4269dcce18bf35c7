// engine_resource_load.cpp — the host side of the resource loader (resource_load.h, resource_load.hip): the checks of a source, the
// pieces' way through two pinned staging halves on a stream of the loader's own, the FLAC decode in front of the load kernels, the
// scalar path of a handle without a device, and what a resource made on the device needs besides: its lazy host mirror and the two
// calls that tell what a resource holds.
#include "engine_impl.h"

namespace elemhip {

namespace rl = resource_load;
namespace fd = flac_decode;
namespace pp = pcm_pack;
namespace fi = flac_in_md5;

void Engine::resourceLoadFree() {
    if (loadStream) (void)hipStreamSynchronize(loadStream);
    for (int k = 0; k < 2; ++k) {
        if (hLoad[k]) (void)hipHostFree(hLoad[k]);
        if (dLoadFlac[k]) (void)hipFree(dLoadFlac[k]);
        if (dLoadImage[k]) (void)hipFree(dLoadImage[k]);
        if (loadDone[k]) (void)hipEventDestroy(loadDone[k]);
        hLoad[k] = dLoadFlac[k] = dLoadImage[k] = nullptr; loadDone[k] = nullptr;
    }
    if (hLoadErr) (void)hipHostFree(hLoadErr);
    if (dLoadErr) (void)hipFree(dLoadErr);
    if (dLoadSubs) (void)hipFree(dLoadSubs);
    if (dLoadState) (void)hipFree(dLoadState);
    if (dLoadScratch) (void)hipFree(dLoadScratch);
    if (dLoadTable) (void)hipFree(dLoadTable);
    if (dLoadRowBase) (void)hipFree(dLoadRowBase);
    if (dLoadRowTable) (void)hipFree(dLoadRowTable);
    if (dLoadMd5) (void)hipFree(dLoadMd5);
    dLoadMd5 = nullptr;
    if (loadStream) (void)hipStreamDestroy(loadStream);
    hLoadErr = dLoadErr = nullptr; dLoadSubs = nullptr; dLoadState = nullptr; dLoadScratch = nullptr;
    dLoadTable = nullptr; dLoadRowBase = nullptr; dLoadRowTable = nullptr; loadStream = nullptr;
    hLoadBytes = dLoadFlacBytes = dLoadImageBytes = loadFrameCap = loadScratchCap = 0; loadRowGroup = 0; loadPlan = resample::Plan{};
}

// the tables of a rate pair, kept for the next file of the same pair (a folder of samples is one pair as a rule)
int Engine::resourceLoadTables(const resample::Plan& p) {
    if (loadPlan.L != p.L || loadPlan.M != p.M || loadTable.empty()) {
        loadTable.assign((size_t)p.T * p.L, 0.0f); loadRowBase.assign(p.L, 0);
        resample::make_tables(p, loadTable.data(), loadRowBase.data());
        loadPlan = p;
        if (dLoadTable) { (void)hipStreamSynchronize(loadStream); (void)hipFree(dLoadTable); (void)hipFree(dLoadRowBase); dLoadTable = nullptr; dLoadRowBase = nullptr; }
    }
    if (dry || dLoadTable) return kOk;
    HIP_OK(hipMalloc((void**)&dLoadTable, loadTable.size() * sizeof(float)));
    HIP_OK(hipMalloc((void**)&dLoadRowBase, loadRowBase.size() * sizeof(int32_t)));
    HIP_OK(hipMemcpy(dLoadTable, loadTable.data(), loadTable.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dLoadRowBase, loadRowBase.data(), loadRowBase.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return kOk;
}

// the loader's stream, events and staging, grown to what the largest piece of this load needs (the loader's stream is idle)
int Engine::resourceLoadGrow(size_t pinned, size_t flacBytes, size_t imageBytes, size_t frames, size_t scratchInts, uint32_t G) {
    if (!loadStream) {
        HIP_OK(hipStreamCreateWithFlags(&loadStream, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) HIP_OK(hipEventCreateWithFlags(&loadDone[k], hipEventDisableTiming));
    }
    auto grow = [&](unsigned char* (&buf)[2], size_t& have, size_t want, bool host) -> int {
        if (want <= have) return kOk;
        for (int k = 0; k < 2; ++k) {
            if (buf[k]) { if (host) (void)hipHostFree(buf[k]); else (void)hipFree(buf[k]); buf[k] = nullptr; }
            have = 0;
            if (host) HIP_OK(hipHostMalloc((void**)&buf[k], want, hipHostMallocDefault)); else HIP_OK(hipMalloc((void**)&buf[k], want));
        }
        have = want;
        return kOk;
    };
    int rc = grow(hLoad, hLoadBytes, pinned, true);
    if (rc == kOk) rc = grow(dLoadImage, dLoadImageBytes, imageBytes, false);
    if (rc == kOk && flacBytes) rc = grow(dLoadFlac, dLoadFlacBytes, flacBytes, false);
    if (rc != kOk || !flacBytes) return rc;
    if (!hLoadErr) {
        HIP_OK(hipHostMalloc((void**)&hLoadErr, 2 * sizeof(FlacInError), hipHostMallocDefault));
        HIP_OK(hipMalloc((void**)&dLoadErr, 2 * sizeof(FlacInError)));
    }
    if (frames * G > loadFrameCap) {
        if (dLoadSubs) (void)hipFree(dLoadSubs);
        if (dLoadState) (void)hipFree(dLoadState);
        dLoadSubs = nullptr; dLoadState = nullptr; loadFrameCap = 0;
        HIP_OK(hipMalloc(&dLoadSubs, frames * G * sizeof(fd::Sub)));
        HIP_OK(hipMalloc((void**)&dLoadState, frames * G * sizeof(uint32_t)));
        loadFrameCap = frames * G;
    }
    if (scratchInts > loadScratchCap) {
        if (dLoadScratch) (void)hipFree(dLoadScratch);
        dLoadScratch = nullptr; loadScratchCap = 0;
        HIP_OK(hipMalloc((void**)&dLoadScratch, scratchInts * sizeof(int32_t)));
        loadScratchCap = scratchInts;
    }
    return kOk;
}

// The scalar path: the whole source through load_host() into the host vectors (a FLAC source through decode_host and image_host
// first, the kernels' functions).
int Engine::resourceLoadHost(const ResourceSrc& src, uint32_t fmt, uint64_t N, const resample::Plan* plan, Resource& r) {
    const uint32_t G = src.channels;
    std::vector<unsigned char> image;
    const unsigned char* data = static_cast<const unsigned char*>(src.data);
    if (src.format == fd::kFormat) {
        const FlacIn& f = *src.flac;
        std::vector<int32_t> codes((size_t)G * std::max<uint64_t>(N, 1));
        int32_t* planar[fd::kMaxChannels];
        for (uint32_t g = 0; g < G; ++g) planar[g] = codes.data() + (size_t)g * std::max<uint64_t>(N, 1);
        size_t bad = 0;
        const uint32_t why = fd::decode_host(f.data, f.frameOffsets, f.frameFirstSamples, (size_t)f.frames, G, f.bits, f.position, (size_t)N, planar, &bad);
        if (why != fd::OK) {
            std::lock_guard<std::mutex> lock(mu);
            flacInErrSet = true; flacInErrStream = 0u; flacInErrFrame = bad; flacInErrReason = why;
            return kFlacInput;
        }
        if (flacInMd5Opt) {         // option "flac_in_md5": the scalar twin over what was decoded, under the device path's rule
            const uint64_t total = fi::total_of(f.totalSamples, f.frames ? f.frameFirstSamples[f.frames] : 0u);
            fi::Slot slot{}; flac_md5::Record rec; flac_md5::init(rec);
            uint64_t lo = 0; bool finish = false;
            if (fi::advance(slot, f.bits, G, total, f.position, f.position + N, lo, finish)) fi::update_codes(rec, planar, G, 0u, N, f.bits, finish ? r.md5 : nullptr);
            r.md5State = slot.state == fi::kComplete ? 2u : 1u;
        }
        image.assign(std::max<size_t>((size_t)N * G * pp::sample_bytes(fmt), 1), 0);
        fd::image_host(f.bits, G, planar, (size_t)N, image.data());
        data = image.data();
    }
    const uint64_t outN = rl::out_frames(plan, N);
    r.channels.assign(G, std::vector<float>((size_t)outN, 0.0f));
    float* rows[rl::kMaxChannels];
    for (uint32_t g = 0; g < G; ++g) rows[g] = r.channels[g].data();
    rl::load_host(fmt, G, N, data, plan, loadTable.data(), loadRowBase.data(), rows);
    return kOk;
}

// The device path. Piece j goes through half j % 2: the host copies the piece as it lies in the file into the pinned half while the
// other half's H2D and kernels run; an event per half says when it may be written again.
int Engine::resourceLoadDevice(const ResourceSrc& src, uint32_t fmt, uint64_t N, const resample::Plan* plan, Resource& r) {
    const uint32_t G = src.channels, P = resourceLoadFramesOpt, B = pp::sample_bytes(fmt);
    const bool flac = src.format == fd::kFormat, md5 = flac && flacInMd5Opt != 0u;
    const uint64_t outN = rl::out_frames(plan, N), pieces = rl::piece_count(N, P);
    const size_t rowFloats = std::max<size_t>((size_t)outN, (size_t)blockSize);      // (ensureResourceOnDevice's rule: a block at least, zero behind the frames)

    // what the largest piece stages
    const PcmSource one{fd::kFormat, G, reinterpret_cast<const void* const*>(&src.flac), 1};
    FlacInSet sets[2];
    size_t pinned = 16, flacBytes = 0, maxFrames = 0, maxScratch = 0;
    const size_t imageBytes = (size_t)rl::staging_bytes(plan, P, G, fmt);
    for (uint64_t j = 0; j < pieces; ++j) {
        const rl::Piece pc = rl::piece_of(plan, N, P, j);
        if (!flac) { pinned = std::max<size_t>(pinned, (size_t)rl::piece_bytes(rl::piece_head(pc.in0, G, fmt), pc.in1 - pc.in0, G, fmt)); continue; }
        flacInPlan(one, pc.in0, (size_t)(pc.in1 - pc.in0), sets[0], md5);
        if (sets[0].stagedBytes > 0xFFFFFFFFull || sets[0].scratchInts > 0xFFFFFFFFull) return kInvalidPropertyValue;      // (the records count in 32 bits)
        pinned = std::max(pinned, sets[0].stagedBytes); maxFrames = std::max(maxFrames, sets[0].frames.size()); maxScratch = std::max(maxScratch, sets[0].scratchInts);
    }
    if (flac) flacBytes = pinned;
    int rc = resourceLoadGrow(pinned, flacBytes, imageBytes, std::max<size_t>(maxFrames, 1), std::max<size_t>(maxScratch, 1), G);
    if (rc != kOk) return rc;
    if (!plan && loadRowGroup != G) {
        std::vector<uint16_t> table(G);
        loadRowDwords = pcm_pack_row_table(G, table.data());
        HIP_OK(hipStreamSynchronize(loadStream));
        if (!dLoadRowTable) HIP_OK(hipMalloc((void**)&dLoadRowTable, rl::kMaxChannels * sizeof(uint16_t)));
        HIP_OK(hipMemcpy(dLoadRowTable, table.data(), G * sizeof(uint16_t), hipMemcpyHostToDevice));
        loadRowGroup = G;
    }

    // option "flac_in_md5": a record of this load's own at its initial value; the slot is the load's too
    fi::Slot md5Slot{};
    if (md5) {
        if (!dLoadMd5) HIP_OK(hipMalloc((void**)&dLoadMd5, sizeof(flac_md5::Record) + 16u));
        flac_md5::Record fresh; flac_md5::init(fresh);
        HIP_OK(hipStreamSynchronize(loadStream));
        HIP_OK(hipMemcpy(dLoadMd5, &fresh, sizeof fresh, hipMemcpyHostToDevice));
    }

    // the rows: the resource's own device buffers, zeroed on the loader's stream in front of the first piece
    r.devCh.assign(G, DevBuf{});
    auto drop = [&](int code) {
        (void)hipStreamSynchronize(loadStream);
        if (r.dev.ptr) (void)hipFree(r.dev.ptr);
        for (DevBuf& d : r.devCh) if (d.ptr) (void)hipFree(d.ptr);
        r.dev = DevBuf{}; r.devCh.clear();
        return code;
    };
    ResourceLoadArgs a{};
    for (uint32_t g = 0; g < G; ++g) {
        DevBuf& d = g == 0 ? r.dev : r.devCh[g];
        if (hipMalloc(&d.ptr, rowFloats * sizeof(float)) != hipSuccess) { d.ptr = nullptr; return drop(kHipError); }
        d.bytes = rowFloats * sizeof(float);
        if (hipMemsetAsync(d.ptr, 0, d.bytes, loadStream) != hipSuccess) return drop(kHipError);
        a.rows[g] = static_cast<float*>(d.ptr);
    }
    a.rowTable = dLoadRowTable; a.rowDwords = loadRowDwords; a.table = dLoadTable; a.rowBase = dLoadRowBase;
    a.totalIn = N; a.rowFloats = rowFloats; a.G = G;
    if (plan) a.plan = *plan;

    // a half's error record, once its event has passed: anything in it ends the load
    bool used[2] = {false, false};
    auto failed = [&](int half) {
        if (!flac || !used[half]) return false;
        const FlacInError e = hLoadErr[half];
        if (e.count == 0u) return false;
        const unsigned long long key = ~e.first;
        const size_t rec = (size_t)(key >> 8);
        std::lock_guard<std::mutex> lock(mu);
        flacInErrSet = true; flacInErrReason = (uint32_t)(key & 0xFFu); flacInErrStream = 0u;
        flacInErrFrame = rec < sets[half].frames.size() ? sets[half].frames[rec].index : 0u;
        return true;
    };
#define LOAD_OK(expr) do { if ((expr) != hipSuccess) { std::fprintf(stderr, "[elemhip] %s failed (%s:%d)\n", #expr, __FILE__, __LINE__); return drop(kHipError); } } while (0)
    for (uint64_t j = 0; j < pieces; ++j) {
        const int half = (int)(j & 1u);
        const rl::Piece pc = rl::piece_of(plan, N, P, j);
        const uint64_t validIn = pc.in1 - pc.in0;
        if (used[half]) {
            LOAD_OK(hipEventSynchronize(loadDone[half]));
            if (failed(half)) return drop(kFlacInput);
        }
        used[half] = true;
        a.in0 = pc.in0; a.out0 = pc.out0; a.validIn = (uint32_t)validIn; a.validOut = (uint32_t)(pc.out1 - pc.out0);
        a.src = dLoadImage[half];
        if (!flac) {
            a.head = rl::piece_head(pc.in0, G, fmt);
            a.srcBytes = rl::piece_bytes(a.head, validIn, G, fmt);
            // (the lines' first and last bytes beside the stretch: the file's where it has them, else whatever the half held — loaded, never decoded)
            const uint64_t from = rl::piece_begin(pc.in0, G, fmt) - a.head, have = std::min<uint64_t>(a.srcBytes, N * G * B - from);
            std::memcpy(hLoad[half], static_cast<const unsigned char*>(src.data) + from, (size_t)have);
            LOAD_OK(hipMemcpyAsync(dLoadImage[half], hLoad[half], (size_t)a.srcBytes, hipMemcpyHostToDevice, loadStream));
        } else {
            FlacInSet& set = sets[half];
            flacInPlan(one, pc.in0, (size_t)validIn, set, md5);
            const size_t nF = set.frames.size(), tables = nF * sizeof(FlacInFrame) + sizeof(FlacInStream);
            unsigned char* dst = hLoad[half];
            if (nF) std::memcpy(dst, set.frames.data(), nF * sizeof(FlacInFrame));
            std::memcpy(dst + nF * sizeof(FlacInFrame), set.streams.data(), sizeof(FlacInStream));
            if (set.len[0]) std::memcpy(dst + tables, src.flac->data + set.from[0], (size_t)set.len[0]);
            if (md5) { set.jobs[0] = flacInMd5Job(*src.flac, set, 0, md5Slot); std::memcpy(dst + set.jobsOff, set.jobs.data(), sizeof(fi::Job)); }
            LOAD_OK(hipMemcpyAsync(dLoadFlac[half], dst, set.stagedBytes, hipMemcpyHostToDevice, loadStream));
            LOAD_OK(hipMemsetAsync(dLoadErr + half, 0, sizeof(FlacInError), loadStream));
            a.head = 0u; a.srcBytes = pp::stream_stride(validIn, G, fmt);
            FlacDecodeArgs d{};
            d.frames = reinterpret_cast<const FlacInFrame*>(dLoadFlac[half]);
            d.streams = reinterpret_cast<const FlacInStream*>(dLoadFlac[half] + nF * sizeof(FlacInFrame));
            d.staged = dLoadFlac[half] + tables;
            d.subs = dLoadSubs; d.state = dLoadState; d.scratch = dLoadScratch; d.error = dLoadErr + half;
            d.dst = dLoadImage[half]; d.streamStride = a.srcBytes;
            d.numFrames = (uint32_t)nF; d.numStreams = 1u; d.G = G; d.bits = src.flac->bits; d.valid = (uint32_t)validIn;
            if (nF * G > loadFrameCap || set.scratchInts > loadScratchCap || set.stagedBytes > dLoadFlacBytes || a.srcBytes > dLoadImageBytes) return drop(kInvariantViolation);
            LOAD_OK(launch_flac_decode(loadStream, d, set.frames.data(), set.streams.data(), set.stagedBytes - tables, set.scratchInts));
            LOAD_OK(hipMemcpyAsync(hLoadErr + half, dLoadErr + half, sizeof(FlacInError), hipMemcpyDeviceToHost, loadStream));
            if (md5) {      // the piece's new samples enter the load's digest behind its decode, in front of the next piece's, which reuses the scratch
                FlacInMd5Args m{};
                m.scratch = dLoadScratch; m.records = reinterpret_cast<flac_md5::Record*>(dLoadMd5); m.digests = dLoadMd5 + sizeof(flac_md5::Record);
                m.jobs = reinterpret_cast<const fi::Job*>(dLoadFlac[half] + set.jobsOff); m.numStreams = 1u; m.G = G; m.bits = src.flac->bits;
                LOAD_OK(launch_flac_in_md5(loadStream, m, set.jobs.data(), set.scratchInts));
            }
        }
        if (a.srcBytes > dLoadImageBytes) return drop(kInvariantViolation);
        LOAD_OK(plan ? launch_resource_convert(loadStream, a, fmt) : launch_resource_copy(loadStream, a, fmt));
        LOAD_OK(hipEventRecord(loadDone[half], loadStream));
    }
    LOAD_OK(hipStreamSynchronize(loadStream));
#undef LOAD_OK
    if (failed(0) || failed(1)) return drop(kFlacInput);
    if (md5) {      // a load that covered the stream from sample 0 to its end leaves its digest with the resource
        r.md5State = md5Slot.state == fi::kComplete ? 2u : 1u;
        if (r.md5State == 2u && hipMemcpy(r.md5, dLoadMd5 + sizeof(flac_md5::Record), 16u, hipMemcpyDeviceToHost) != hipSuccess) return drop(kHipError);
    }
    r.devCh[0] = DevBuf{};                          // (channel 0 is `dev`)
    r.onDevice = true; r.deviceChannels = G; r.deviceFrames = outN;
    return kOk;
}

int Engine::addSharedResourcePcm(const std::string& name, const ResourceSrc& src, bool* inserted) {
    std::lock_guard<std::mutex> control(ctl);
    if (inserted) *inserted = false;
    // ---- the source ----
    const bool flac = src.format == fd::kFormat;
    if (!flac && !pp::format_ok(src.format)) return kInvalidInstructionFormat;
    if (src.channels == 0u || src.channels > rl::kMaxChannels) return kInvalidInstructionFormat;
    uint32_t fmt = src.format;
    uint64_t N = src.frames;
    if (flac) {
        if (!src.flac) return kInvalidInstructionFormat;
        const PcmSource one{fd::kFormat, src.channels, reinterpret_cast<const void* const*>(&src.flac), 1};
        const int rc = flacInCheck(one);
        if (rc != kOk) return rc;
        fmt = fd::image_format(src.flac->bits);
        const uint64_t end = src.flac->frames ? src.flac->frameFirstSamples[src.flac->frames] : 0u;
        N = std::min<uint64_t>(N, end > src.flac->position ? end - src.flac->position : 0u);
    } else {
        if (N > rl::kMaxFrames) return kInvalidPropertyValue;
        if ((N && !src.data) || src.bytes < N * src.channels * pp::sample_bytes(fmt)) return kInvalidInstructionFormat;
    }
    // ---- the rate ----
    resample::Plan plan{};
    const bool convert = src.sampleRate != 0.0 && src.sampleRate != sampleRate;
    if (convert && !resample::make_plan(src.sampleRate, sampleRate, plan)) return kInvalidPropertyValue;
    if (N > rl::kMaxFrames || (convert && (N > rl::kMaxFrames / plan.L * plan.M + plan.M || resample::outputs_before(plan, N) > rl::kMaxFrames))) return kInvalidPropertyValue;
    {
        RenderGuard lock(*this);
        if (resources.count(name)) return kOk;                // insert-only (SharedResource.h:61-63): the bytes are not even read
    }
    if (!dry && hipSetDevice(device) != hipSuccess) return kHipError;
    if (convert) { const int rc = resourceLoadTables(plan); if (rc != kOk) return rc; }
    auto r = std::make_shared<Resource>();
    const int rc = dry ? resourceLoadHost(src, fmt, N, convert ? &plan : nullptr, *r) : resourceLoadDevice(src, fmt, N, convert ? &plan : nullptr, *r);
    if (rc != kOk) return rc;
    // ---- the finished resource: the render lock for the insertion and no longer (`ctl` kept every other writer of the map out) ----
    RenderGuard lock(*this);
    resources.emplace(name, r);
    if (inserted) *inserted = true;
    return kOk;
}

const std::vector<std::vector<float>>& Engine::resourceHost(const ResourcePtr& r) {
    if (r->onDevice && r->channels.empty() && !dry) {
        std::vector<std::vector<float>> host(r->deviceChannels, std::vector<float>((size_t)r->deviceFrames));
        bool ok = true;
        for (uint32_t c = 0; c < r->deviceChannels && r->deviceFrames; ++c) {
            const void* p = c == 0 ? r->dev.ptr : r->devCh[c].ptr;
            ok = hipMemcpy(host[c].data(), p, (size_t)r->deviceFrames * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess && ok;
        }
        if (!ok) std::fprintf(stderr, "[elemhip] the host mirror of a device resource could not be fetched\n");
        r->channels.swap(host);
    }
    return r->channels;
}

int Engine::sharedResourceInfo(const std::string& name, uint32_t* channels, uint64_t* frames) {
    std::lock_guard<std::mutex> control(ctl);
    RenderGuard lock(*this);
    auto it = resources.find(name);
    if (it == resources.end()) return kInvalidPropertyValue;
    if (channels) *channels = (uint32_t)it->second->numChannels();
    if (frames) *frames = it->second->frames(0);
    return kOk;
}

int Engine::sharedResourceMd5(const std::string& name, uint8_t digest[16], uint32_t* state) {
    std::lock_guard<std::mutex> control(ctl);
    RenderGuard lock(*this);
    auto it = resources.find(name);
    if (it == resources.end()) return kInvalidPropertyValue;
    if (state) *state = it->second->md5State;
    if (digest) std::memcpy(digest, it->second->md5, 16u);
    return kOk;
}

int Engine::sharedResourceRead(const std::string& name, uint32_t channel, uint64_t first, uint64_t count, float* out) {
    std::lock_guard<std::mutex> control(ctl);
    RenderGuard lock(*this);
    auto it = resources.find(name);
    if (it == resources.end()) return kInvalidPropertyValue;
    const Resource& r = *it->second;
    // a device row is a block long at least, zero behind the resource's frames (ensureResourceOnDevice): that padding can be read too
    if (channel >= r.numChannels()) return kInvalidPropertyValue;
    const uint64_t have = r.frames(channel), padded = std::max<uint64_t>(have, (uint64_t)blockSize);
    if (first > padded || count > padded - first) return kInvalidPropertyValue;
    if (count == 0) return kOk;
    if (!out) return kInvalidInstructionFormat;
    if (r.onDevice) {
        if (hipSetDevice(device) != hipSuccess) return kHipError;
        const float* p = static_cast<const float*>(channel == 0 ? r.dev.ptr : r.devCh[channel].ptr);
        HIP_OK(hipMemcpy(out, p + first, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
        return kOk;
    }
    for (uint64_t i = 0; i < count; ++i) out[i] = first + i < have ? r.channels[channel][(size_t)(first + i)] : 0.0f;
    return kOk;
}

} // namespace elemhip
