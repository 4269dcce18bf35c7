// engine_flac.cpp — the host side of FLAC delivery (options "flac_frame", "flac_bits", "flac_lpc_order", "flac_md5"; flac_encode.h, flac_encode.hip, flac_md5.hip): the programme's
// state, the device buffers' life, the hand-over of a set's frames to the caller's buffers, the flush, the read-out and the reset. The
// set loop that launches the kernels is renderHostSets (engine_render.cpp).
#include "engine_impl.h"
#include "flac_encode.h"

namespace elemhip {

namespace fe = flac_encode;

void Engine::flacFree() {
    if (dFlacCarry) (void)hipFree(dFlacCarry);
    if (dFlacCodes) (void)hipFree(dFlacCodes);
    if (dFlacSlots) (void)hipFree(dFlacSlots);
    if (dFlacSubBits) (void)hipFree(dFlacSubBits);
    if (flacStream) (void)hipStreamDestroy(flacStream);
    if (dFlacMd5) (void)hipFree(dFlacMd5);
    dFlacMd5 = nullptr; flacMd5Cap = 0;
    dFlacCarry = dFlacCodes = nullptr; dFlacSlots = dFlacSubBits = nullptr; flacStream = nullptr;
    flacCarryCh = flacCodesCh = flacCodesCap = flacSlotCount = flacSlotWords = 0;
}

// a new programme: nothing open, frame number 0; its shape is set by the first call (`mu` held), which also starts the streams'
// MD5 records anew (ensureFlac: the device is current there, and nothing of the old programme is in flight)
int Engine::flacResetLocked() {
    flacFF = flacBits = flacG = flacStreams = flacRate = flacOpen = flacLpc = flacMd5 = 0;
    flacMd5Final = false; flacDigests.clear();
    flacFlushed = false; flacFrames = flacEmitted = 0;
    flacFrameBytes.clear();
    return kOk;
}

// The programme takes its shape from its first call. The codes hold the open frame and `setFrames` frames of every channel, the slots
// one subframe per candidate of every whole FLAC frame in them; the packed halves the length table, the statistics and the frames.
int Engine::ensureFlac(FlacJob& job, size_t setFrames) {
    const uint32_t G = job.spec.channelsPerStream, bits = job.spec.bits, S = (uint32_t)job.nStreams;
    const size_t nOut = (size_t)S * G;
    if (flacStreams == 0) {
        const double rate = deliveryRate();
        if (!(rate >= 1.0) || rate > 1048575.0 || rate != std::floor(rate)) return kInvalidPropertyValue;       // (STREAMINFO holds 20 bits of Hz)
        flacFF = flacFrameOpt; flacLpc = flacLpcOpt; flacBits = bits; flacG = G; flacStreams = S; flacRate = (uint32_t)rate; flacOpen = 0;
        flacFrameBytes.assign(S, std::vector<uint32_t>());
        flacMd5 = flacMd5Opt;
        if (flacMd5) {          // S records at their initial value, the digests behind them
            HIP_OK(hipStreamSynchronize(stream));
            if (S > flacMd5Cap) {
                if (dFlacMd5) (void)hipFree(dFlacMd5);
                dFlacMd5 = nullptr; flacMd5Cap = 0;
                HIP_OK(hipMalloc((void**)&dFlacMd5, (size_t)S * (sizeof(flac_md5::Record) + 16u)));
                flacMd5Cap = S;
            }
            std::vector<flac_md5::Record> fresh(S);
            for (flac_md5::Record& r : fresh) flac_md5::init(r);
            HIP_OK(hipMemcpy(dFlacMd5, fresh.data(), (size_t)S * sizeof(flac_md5::Record), hipMemcpyHostToDevice));
        }
    } else if (flacBits != bits || flacG != G || flacStreams != S || flacRate != (uint32_t)deliveryRate()) return kInvalidPropertyValue;
    const uint32_t ff = flacFF;
    const size_t cap = (size_t)ff - 1u + setFrames, maxF = cap / ff, slotCount = (size_t)S * maxF * fe::candidates(G), words = fe::slot_words(ff, bits);
    if (cap > 0x7FFFFFFFull) return kInvalidPropertyValue;              // (the kernels count a set's frames in 32 bits)
    if (nOut > flacCarryCh || nOut > flacCodesCh || cap > flacCodesCap || slotCount > flacSlotCount || slotCount * words > flacSlotWords) {
        HIP_OK(hipStreamSynchronize(stream));
        if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
    }
    if (nOut > flacCarryCh) {           // (only a programme's first call gets here: nothing is open)
        if (dFlacCarry) (void)hipFree(dFlacCarry);
        dFlacCarry = nullptr; flacCarryCh = 0;
        HIP_OK(hipMalloc((void**)&dFlacCarry, nOut * fe::kMaxFrame * sizeof(int32_t)));
        flacCarryCh = nOut;
    }
    if (nOut > flacCodesCh || cap > flacCodesCap) {
        const size_t ch = std::max(nOut, flacCodesCh), cp = std::max(cap, flacCodesCap);
        if (dFlacCodes) (void)hipFree(dFlacCodes);
        dFlacCodes = nullptr; flacCodesCh = flacCodesCap = 0;
        HIP_OK(hipMalloc((void**)&dFlacCodes, ch * cp * sizeof(int32_t)));
        flacCodesCh = ch; flacCodesCap = cp;
    }
    if (slotCount > flacSlotCount) {
        if (dFlacSubBits) (void)hipFree(dFlacSubBits);
        dFlacSubBits = nullptr; flacSlotCount = 0;
        HIP_OK(hipMalloc((void**)&dFlacSubBits, std::max<size_t>(slotCount, 1) * sizeof(uint32_t)));
        flacSlotCount = slotCount;
    }
    if (slotCount * words > flacSlotWords) {
        if (dFlacSlots) (void)hipFree(dFlacSlots);
        dFlacSlots = nullptr; flacSlotWords = 0;
        HIP_OK(hipMalloc((void**)&dFlacSlots, slotCount * words * sizeof(uint32_t)));
        flacSlotWords = slotCount * words;
    }
    if (!flacStream) HIP_OK(hipStreamCreateWithFlags(&flacStream, hipStreamNonBlocking));
    auto up16 = [](size_t v) { return (v + 15u) & ~(size_t)15u; };
    job.statsOff = up16((size_t)S * maxF * sizeof(uint32_t));
    job.payloadOff = job.statsOff + up16(nOut * sizeof(pcm_pack::ChannelStats));
    job.stride = up16(std::max<size_t>(maxF, 1) * fe::frame_bound(ff, G, bits));
    return growPackedHalves(hPcm, dPcm, pcmBytes, job.payloadOff + (size_t)S * job.stride);
}

// The table and the statistics of the set in `half` have arrived: the frames' bytes, known only now, follow on a stream of their own
// (the copy stream already waits for the next set's render) and go to the caller's buffers behind what earlier sets left there.
int Engine::flacDeliver(FlacJob& job, int half) {
    const size_t S = job.nStreams, nOut = S * job.spec.channelsPerStream;
    const unsigned char* h = hPcm[half];
    const pcm_pack::ChannelStats* st = reinterpret_cast<const pcm_pack::ChannelStats*>(h + job.statsOff);
    for (size_t c = 0; c < nOut; ++c) {
        job.tally.peakBits[c] = std::max(job.tally.peakBits[c], st[c].peakBits);
        job.tally.over[c] += st[c].over; job.tally.nonfinite[c] += st[c].nonfinite;
    }
    const uint32_t nF = job.framesOf[half];
    if (nF == 0) return kOk;
    const uint32_t* table = reinterpret_cast<const uint32_t*>(h);
    std::vector<size_t> len(S, 0);
    for (size_t s = 0; s < S; ++s) {
        for (uint32_t j = 0; j < nF; ++j) len[s] += table[s * nF + j];
        if (len[s] > job.stride || job.bytes[s] + len[s] > job.caps[s]) return kInvariantViolation;      // (the bounds were checked up front)
    }
    {
        RenderGuard lock(*this);
        if (hipSetDevice(device) != hipSuccess) return kHipError;
        for (size_t s = 0; s < S; ++s)
            HIP_OK(hipMemcpyAsync(hPcm[half] + job.payloadOff + s * job.stride, dPcm[half] + job.payloadOff + s * job.stride, len[s], hipMemcpyDeviceToHost, flacStream));
        HIP_OK(hipStreamSynchronize(flacStream));
        for (size_t s = 0; s < S; ++s) flacFrameBytes[s].insert(flacFrameBytes[s].end(), table + s * nF, table + (s + 1) * nF);
    }
    for (size_t s = 0; s < S; ++s) {
        std::memcpy(static_cast<unsigned char*>(job.streams[s]) + job.bytes[s], h + job.payloadOff + s * job.stride, len[s]);
        job.bytes[s] += len[s];
    }
    return kOk;
}

int Engine::processBlocksFlac(const PcmSource& src, void* const* outStreams, const size_t* capacities, size_t* bytesOut, size_t nOutStreams,
                              const FlacSpec& specIn, size_t numFrames, int64_t sampleTime, PcmChannelStats* stats) {
    const bool flacSrc = src.nStreams && src.format == flac_decode::kFormat;
    if (src.nStreams && ((!flacSrc && !pcm_pack::format_ok(src.format)) || src.channelsPerStream == 0u || !src.streams)) return kInvalidInstructionFormat;
    if (flacSrc) { const int rc = flacInCheck(src); if (rc != kOk) return rc; }
    for (size_t s = 0; s < src.nStreams; ++s) if (!src.streams[s] && numFrames) return kInvalidInstructionFormat;
    FlacSpec spec = specIn;
    if (spec.bits == 0u) { std::lock_guard<std::mutex> lock(mu); spec.bits = flacBitsOpt; }
    if (!fe::bits_ok(spec.bits) || spec.channelsPerStream == 0u || spec.channelsPerStream > fe::kMaxChannels) return kInvalidInstructionFormat;
    if (nOutStreams == 0 || !outStreams || !capacities || !bytesOut) return kInvalidInstructionFormat;
    for (size_t s = 0; s < nOutStreams; ++s) if (!outStreams[s]) return kInvalidInstructionFormat;
    if (src.nStreams > kMaxHostIn || src.nStreams * (size_t)src.channelsPerStream > kMaxHostIn) return kTooManyChannels;
    if (nOutStreams > kMaxOutBus || nOutStreams * (size_t)spec.channelsPerStream > kMaxOutBus) return kTooManyChannels;
    if (dry) return kNoDevice;
    {   // a closed programme, or one of another shape: refused before anything is rendered, and the programme stays as it is
        std::lock_guard<std::mutex> lock(mu);
        if (flacFlushed) return kInvalidPropertyValue;
        if (flacStreams != 0u && (flacBits != spec.bits || flacG != spec.channelsPerStream || flacStreams != nOutStreams || flacRate != (uint32_t)deliveryRate()))
            return kInvalidPropertyValue;
    }
    size_t delivered = numFrames;
    (void)resampleFrames(numFrames, &delivered);
    const size_t entering = (size_t)std::min<uint64_t>(spec.take, delivered - std::min<uint64_t>(spec.drop, delivered));
    for (size_t s = 0; s < nOutStreams; ++s) {
        bytesOut[s] = 0;
        if (capacities[s] < fe::stream_bound(entering, spec.channelsPerStream, spec.bits)) return kTooManyChannels;
    }
    const size_t nIn = src.nStreams * src.channelsPerStream, nOut = nOutStreams * spec.channelsPerStream;
    FlacJob job;
    job.spec = spec; job.streams = outStreams; job.caps = capacities; job.bytes = bytesOut; job.nStreams = nOutStreams;
    job.tally.init(nOut);
    job.dropLeft = spec.drop; job.takeLeft = spec.take;
    const int rc = renderHostSets(nullptr, nIn, nullptr, nOut, numFrames, sampleTime, nullptr, src.nStreams ? &src : nullptr, &job);
    if (rc != kOk) { RenderGuard lock(*this); (void)flacResetLocked(); }       // (the carried codes may be ahead of what was delivered)
    job.tally.writeTo(stats);
    return rc;
}

// the open remainder as one short final frame per stream, through the same kernels; the programme is closed
int Engine::flacFlush(void* const* outStreams, const size_t* capacities, size_t* bytesOut, size_t nOutStreams) {
    if (dry) return kNoDevice;
    RenderGuard lock(*this);
    if (flacFlushed) return kInvalidPropertyValue;
    for (size_t s = 0; s < nOutStreams; ++s) if (bytesOut) bytesOut[s] = 0;
    if (flacStreams == 0 || flacOpen == 0) {          // (a programme whose frames were all dropped still has a digest: the empty message's)
        if (flacStreams != 0u && flacMd5) { const int rc = flacMd5Finish(); if (rc != kOk) return rc; }
        flacFlushed = true;
        return kOk;
    }
    if (nOutStreams != flacStreams || !outStreams || !capacities || !bytesOut) return kInvalidInstructionFormat;
    const uint32_t fb = fe::frame_bound(flacOpen, flacG, flacBits);
    for (size_t s = 0; s < nOutStreams; ++s) { if (!outStreams[s]) return kInvalidInstructionFormat; if (capacities[s] < fb) return kTooManyChannels; }
    if (flacEmitted >= 0x7FFFFFFFull) return kInvariantViolation;
    if (hipSetDevice(device) != hipSuccess) return kHipError;
    FlacJob job;
    job.spec = FlacSpec{flacBits, flacG, 0u, 0u, 0u, 0u}; job.nStreams = flacStreams;
    int rc = ensureFlac(job, 1);
    if (rc != kOk) return rc;
    const size_t nOut = (size_t)flacStreams * flacG;
    HIP_OK(hipStreamSynchronize(stream));
    if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
    HIP_OK(hipMemsetAsync(dPcm[0] + job.statsOff, 0, nOut * sizeof(pcm_pack::ChannelStats), stream));
    FlacStageArgs sa{};
    sa.src = nullptr; sa.carry = dFlacCarry; sa.codes = dFlacCodes; sa.stats = reinterpret_cast<pcm_pack::ChannelStats*>(dPcm[0] + job.statsOff);
    sa.blockSize = (uint32_t)blockSize; sa.numChannels = (uint32_t)nOut; sa.validFrames = 0u; sa.open = flacOpen; sa.cap = (uint32_t)flacCodesCap; sa.bits = flacBits;
    HIP_OK(launch_flac_stage(stream, sa));
    FlacEncodeArgs ea{};
    ea.codes = dFlacCodes; ea.slots = dFlacSlots; ea.subBits = dFlacSubBits; ea.dst = dPcm[0] + job.payloadOff; ea.frameBytes = reinterpret_cast<uint32_t*>(dPcm[0]);
    ea.streamStride = job.stride; ea.cap = (uint32_t)flacCodesCap; ea.G = flacG; ea.numStreams = flacStreams; ea.bits = flacBits; ea.flacFrame = flacFF;
    ea.n = flacOpen; ea.numFrames = 1u; ea.slotWords = fe::slot_words(flacFF, flacBits); ea.rate = flacRate; ea.firstNumber = (uint32_t)flacEmitted;
    ea.lpcOrder = flacLpc;
    HIP_OK(launch_flac_encode(stream, ea));
    HIP_OK(hipMemcpyAsync(hPcm[0], dPcm[0], job.payloadOff + (size_t)flacStreams * job.stride, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    const uint32_t* table = reinterpret_cast<const uint32_t*>(hPcm[0]);
    for (size_t s = 0; s < nOutStreams; ++s) {
        const uint32_t len = table[s];
        if (len > capacities[s] || len > job.stride) return kInvariantViolation;
        std::memcpy(outStreams[s], hPcm[0] + job.payloadOff + s * job.stride, len);
        bytesOut[s] = len;
        flacFrameBytes[s].push_back(len);
    }
    if (flacMd5) { rc = flacMd5Finish(); if (rc != kOk) return rc; }       // (the open frame's codes were hashed when they were staged)
    flacEmitted += 1; flacOpen = 0; flacFlushed = true;
    return kOk;
}

// the set's new codes [first, first + count) of every channel enter their stream's digest, on `stream` behind the stage kernel
int Engine::flacMd5Launch(uint32_t first, uint32_t count, bool finish) {
    FlacMd5Args a{};
    a.codes = dFlacCodes; a.records = flacMd5Records(); a.digests = flacMd5Digests();
    a.cap = (uint32_t)flacCodesCap; a.G = flacG; a.numStreams = flacStreams; a.bits = flacBits; a.first = first; a.count = count; a.finish = finish ? 1u : 0u;
    if (flacStreams > flacMd5Cap) return kInvariantViolation;
    HIP_OK(launch_flac_md5(stream, a));
    return kOk;
}

int Engine::flacMd5Finish() {
    if (hipSetDevice(device) != hipSuccess) return kHipError;
    const int rc = flacMd5Launch(0u, 0u, true);
    if (rc != kOk) return rc;
    flacDigests.assign((size_t)flacStreams * 16u, 0u);
    HIP_OK(hipMemcpyAsync(flacDigests.data(), flacMd5Digests(), flacDigests.size(), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    flacMd5Final = true;
    return kOk;
}

int Engine::flacMd5Read(uint8_t* digests, size_t capacity, uint32_t* state) {
    RenderGuard lock(*this);
    const uint32_t st = flacStreams == 0u || !flacMd5 ? 0u : flacMd5Final ? 2u : 1u;
    if (state) *state = st;
    if (!digests || st == 0u) return kOk;
    if (capacity < flacStreams) return kInvalidPropertyValue;
    if (st == 2u) std::memcpy(digests, flacDigests.data(), (size_t)flacStreams * 16u);
    else std::memset(digests, 0, (size_t)flacStreams * 16u);
    return kOk;
}

int Engine::flacRead(FlacInfo* info, FlacStreamInfo* perStream, size_t capacity, uint32_t* frameBytes, size_t frameCap) {
    RenderGuard lock(*this);
    const uint32_t ff = flacStreams ? flacFF : flacFrameOpt;
    if (info) *info = FlacInfo{ff, flacStreams ? flacBits : flacBitsOpt, flacG, flacStreams, flacRate, flacFlushed ? 1u : 0u, flacFrames};
    if (!flacStreams || (!perStream && !frameBytes)) return kOk;
    if (perStream && capacity < flacStreams) return kInvalidPropertyValue;
    for (uint32_t s = 0; s < flacStreams; ++s) {
        const std::vector<uint32_t>& fb = flacFrameBytes[s];
        if (perStream) {
            FlacStreamInfo si{fb.size(), flacFrames - flacOpen, 0u, 0u};
            for (uint32_t b : fb) { si.minFrameBytes = si.minFrameBytes && si.minFrameBytes < b ? si.minFrameBytes : b; si.maxFrameBytes = std::max(si.maxFrameBytes, b); }
            perStream[s] = si;
        }
        if (frameBytes) {
            if (frameCap < fb.size()) return kInvalidPropertyValue;
            if (!fb.empty()) std::memcpy(frameBytes + (size_t)s * frameCap, fb.data(), fb.size() * sizeof(uint32_t));
        }
    }
    return kOk;
}

uint32_t Engine::flacLpcOrder() {
    RenderGuard lock(*this);
    return flacStreams ? flacLpc : flacLpcOpt;
}

int Engine::flacReset() {
    RenderGuard lock(*this);
    if (!dry) {
        if (hipSetDevice(device) != hipSuccess) return kHipError;
        HIP_OK(hipStreamSynchronize(stream));
        if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
    }
    return flacResetLocked();
}

} // namespace elemhip
