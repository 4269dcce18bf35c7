// engine_flac_in.cpp — the host side of FLAC input (input format 4; flac_decode.h, flac_decode.hip): the checks of a FLAC source, the
// per-set lookup of the covering frames by binary search, the staging halves, the launch, the error record's way back and the host
// decode of the block-by-block path (engine_host_blocks.cpp). The set loop that stages, copies and launches is renderHostSets (engine_render.cpp).
#include "engine_impl.h"

namespace elemhip {

namespace fd = flac_decode;
namespace fi = flac_in_md5;

void Engine::flacInFree() {
    for (int k = 0; k < 2; ++k) { if (hFlacIn[k]) (void)hipHostFree(hFlacIn[k]); if (dFlacIn[k]) (void)hipFree(dFlacIn[k]); hFlacIn[k] = dFlacIn[k] = nullptr; }
    if (hFlacInErr) (void)hipHostFree(hFlacInErr);
    if (dFlacInErr) (void)hipFree(dFlacInErr);
    if (dFlacInSubs) (void)hipFree(dFlacInSubs);
    if (dFlacInState) (void)hipFree(dFlacInState);
    if (dFlacInScratch) (void)hipFree(dFlacInScratch);
    hFlacInErr = dFlacInErr = nullptr; dFlacInSubs = nullptr; dFlacInState = nullptr; dFlacInScratch = nullptr;
    flacInBytes = flacInFrameCap = flacInScratchCap = 0;
    if (dFlacInMd5) (void)hipFree(dFlacInMd5);
    if (hFlacInMd5) (void)hipHostFree(hFlacInMd5);
    dFlacInMd5 = nullptr; hFlacInMd5 = nullptr;
}

uint32_t Engine::flacInBits(const PcmSource& src) const { return src.nStreams ? static_cast<const FlacIn*>(src.streams[0])->bits : 16u; }

// what a FLAC source has to be before anything is rendered
int Engine::flacInCheck(const PcmSource& src) const {
    static_assert(sizeof(FlacInFrame) == 32 && sizeof(FlacInStream) == 32 && sizeof(FlacInError) == 16, "the records' layout");
    if (!src.streams) return kInvalidInstructionFormat;
    for (size_t s = 0; s < src.nStreams; ++s) {
        const FlacIn* f = static_cast<const FlacIn*>(src.streams[s]);
        if (!f || !f->frameOffsets || !f->frameFirstSamples || (f->bytes && !f->data)) return kInvalidInstructionFormat;
        if (!fd::bits_ok(f->bits) || f->bits != flacInBits(src) || f->channels == 0u || f->channels > fd::kMaxChannels) return kInvalidInstructionFormat;
        if (f->channels != src.channelsPerStream) return kInvalidInstructionFormat;
        // the table: offsets inside the bytes and rising, first samples rising by a block at most, the closing entry the stream's total
        for (uint64_t j = 0; j < f->frames; ++j) {
            const uint64_t o0 = f->frameOffsets[j], o1 = f->frameOffsets[j + 1], t0 = f->frameFirstSamples[j], t1 = f->frameFirstSamples[j + 1];
            if (o1 < o0 || o1 > f->bytes || o1 - o0 > 0x7FFFFFFFull || t1 <= t0 || t1 - t0 > fd::kMaxBlock) return kInvalidInstructionFormat;
            if (j + 1 < f->frames && t1 - t0 != f->frameFirstSamples[1] - f->frameFirstSamples[0]) return kInvalidInstructionFormat;      // fixed block size
            if (t1 - t0 > f->frameFirstSamples[1] - f->frameFirstSamples[0]) return kInvalidInstructionFormat;
        }
        if (f->frames && f->position < f->frameFirstSamples[0]) return kInvalidInstructionFormat;      // (the table has to reach back to the position)
    }
    return kOk;
}

// The records of the set that reads input frames [from, from + valid) of the call: per stream the frames that cover stream samples
// [position + from, position + from + valid), cut at the stream's end.
void Engine::flacInPlan(const PcmSource& src, uint64_t from, size_t valid, FlacInSet& set, bool md5) const {
    const size_t S = src.nStreams;
    const uint32_t G = src.channelsPerStream;
    set.frames.clear(); set.streams.assign(S, FlacInStream{}); set.from.assign(S, 0); set.len.assign(S, 0);
    uint64_t scratch = 0, bytes = 0;
    for (size_t s = 0; s < S; ++s) {
        const FlacIn& f = *static_cast<const FlacIn*>(src.streams[s]);
        FlacInStream& st = set.streams[s];
        st.firstFrame = (uint32_t)set.frames.size(); st.scratchBase = (uint32_t)scratch;
        const uint64_t end = f.frames ? f.frameFirstSamples[f.frames] : 0u, p0 = f.position + from;
        if (valid == 0 || f.frames == 0 || p0 >= end || p0 < f.frameFirstSamples[0]) continue;
        const uint64_t p1 = std::min<uint64_t>(p0 + valid, end);
        const size_t j0 = fd::frame_of(f.frameFirstSamples, (size_t)f.frames, p0), j1 = fd::frame_of(f.frameFirstSamples, (size_t)f.frames, p1 - 1u);
        st.frames = (uint32_t)(j1 - j0 + 1u);
        st.blockSize = (uint32_t)(f.frameFirstSamples[j0 + 1u] - f.frameFirstSamples[j0]);
        st.skip = (uint32_t)(p0 - f.frameFirstSamples[j0]);
        st.have = (uint32_t)(p1 - p0);
        st.covered = (uint32_t)(f.frameFirstSamples[j1 + 1u] - f.frameFirstSamples[j0]);
        set.from[s] = f.frameOffsets[j0]; set.len[s] = f.frameOffsets[j1 + 1u] - f.frameOffsets[j0];
        for (size_t j = j0; j <= j1; ++j) {
            FlacInFrame r{};
            r.byteOff = (uint32_t)(bytes + (f.frameOffsets[j] - f.frameOffsets[j0])); r.len = (uint32_t)(f.frameOffsets[j + 1u] - f.frameOffsets[j]);
            r.stream = (uint32_t)s; r.index = (uint32_t)j; r.n = (uint32_t)(f.frameFirstSamples[j + 1u] - f.frameFirstSamples[j]);
            r.scratchOff = (uint32_t)(scratch + (f.frameFirstSamples[j] - f.frameFirstSamples[j0])); r.chStride = st.covered;
            set.frames.push_back(r);
        }
        scratch += (uint64_t)G * st.covered;
        bytes += (set.len[s] + 15u) & ~(uint64_t)15u;
    }
    // the staged half: the two tables, 16-byte aligned, in front of the bytes (byteOff counts from the bytes' start)
    const size_t tables = set.frames.size() * sizeof(FlacInFrame) + S * sizeof(FlacInStream);
    set.stagedBytes = tables + (size_t)bytes; set.scratchInts = (size_t)scratch;
    // option "flac_in_md5": the streams' jobs behind the bytes (flacInMd5Jobs fills them in)
    set.jobs.clear(); set.md5Work = set.md5Finish = false; set.jobsOff = 0;
    if (md5) {
        set.jobs.assign(S, fi::Job{});
        set.jobsOff = (set.stagedBytes + 15u) & ~(size_t)15u;
        set.stagedBytes = set.jobsOff + S * sizeof(fi::Job);
    }
}

int Engine::ensureFlacIn(size_t stagedBytes, size_t frames, size_t scratchInts, uint32_t G) {
    if (stagedBytes > 0xFFFFFFFFull || scratchInts > 0xFFFFFFFFull) return kInvalidPropertyValue;      // (the records count in 32 bits)
    int rc = growPackedHalves(hFlacIn, dFlacIn, flacInBytes, std::max<size_t>(stagedBytes, 16));
    if (rc != kOk) return rc;
    if (!hFlacInErr) {
        HIP_OK(hipHostMalloc((void**)&hFlacInErr, 2 * sizeof(FlacInError), hipHostMallocDefault));
        HIP_OK(hipMalloc((void**)&dFlacInErr, 2 * sizeof(FlacInError)));
    }
    if (frames * G > flacInFrameCap || scratchInts > flacInScratchCap) {
        HIP_OK(hipStreamSynchronize(stream));
        if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
    }
    if (frames * G > flacInFrameCap) {
        if (dFlacInSubs) (void)hipFree(dFlacInSubs);
        if (dFlacInState) (void)hipFree(dFlacInState);
        dFlacInSubs = nullptr; dFlacInState = nullptr; flacInFrameCap = 0;
        HIP_OK(hipMalloc(&dFlacInSubs, frames * G * sizeof(fd::Sub)));
        HIP_OK(hipMalloc((void**)&dFlacInState, frames * G * sizeof(uint32_t)));
        flacInFrameCap = frames * G;
    }
    if (scratchInts > flacInScratchCap) {
        if (dFlacInScratch) (void)hipFree(dFlacInScratch);
        dFlacInScratch = nullptr; flacInScratchCap = 0;
        HIP_OK(hipMalloc((void**)&dFlacInScratch, scratchInts * sizeof(int32_t)));
        flacInScratchCap = scratchInts;
    }
    return kOk;
}

// the set's tables and covering bytes into the pinned half, as they lie in the caller's buffers
void Engine::flacInStage(const PcmSource& src, const FlacInSet& set, int half) {
    unsigned char* dst = hFlacIn[half];
    const size_t nF = set.frames.size(), S = set.streams.size();
    if (nF) std::memcpy(dst, set.frames.data(), nF * sizeof(FlacInFrame));
    if (S) std::memcpy(dst + nF * sizeof(FlacInFrame), set.streams.data(), S * sizeof(FlacInStream));
    size_t at = nF * sizeof(FlacInFrame) + S * sizeof(FlacInStream);
    for (size_t s = 0; s < S; ++s) {
        if (set.len[s]) std::memcpy(dst + at, static_cast<const FlacIn*>(src.streams[s])->data + set.from[s], (size_t)set.len[s]);
        at += (size_t)((set.len[s] + 15u) & ~(uint64_t)15u);
    }
}

// the decode kernels behind the staged half's H2D, on the render's stream, into the packed input half
int Engine::flacInLaunch(const FlacInSet& set, int half, uint32_t G, uint32_t bits, size_t valid, size_t streamStride) {
    const size_t nF = set.frames.size(), S = set.streams.size(), tables = nF * sizeof(FlacInFrame) + S * sizeof(FlacInStream);
    if (set.stagedBytes > flacInBytes || nF * G > flacInFrameCap || set.scratchInts > flacInScratchCap || S * streamStride > pcmInBytes) return kInvariantViolation;
    HIP_OK(hipMemsetAsync(dFlacInErr + half, 0, sizeof(FlacInError), stream));
    FlacDecodeArgs a{};
    a.frames = reinterpret_cast<const FlacInFrame*>(dFlacIn[half]);
    a.streams = reinterpret_cast<const FlacInStream*>(dFlacIn[half] + nF * sizeof(FlacInFrame));
    a.staged = dFlacIn[half] + tables;
    a.subs = dFlacInSubs; a.state = dFlacInState; a.scratch = dFlacInScratch; a.error = dFlacInErr + half;
    a.dst = dPcmIn[half]; a.streamStride = streamStride;
    a.numFrames = (uint32_t)nF; a.numStreams = (uint32_t)S; a.G = G; a.bits = bits; a.valid = (uint32_t)valid;
    HIP_OK(launch_flac_decode(stream, a, set.frames.data(), set.streams.data(), set.stagedBytes - tables, set.scratchInts));
    return kOk;
}

bool Engine::flacInFailed(int half) {
    const FlacInError e = hFlacInErr[half];
    if (e.count == 0u) return false;
    const unsigned long long key = ~e.first;
    const size_t rec = (size_t)(key >> 8);
    std::lock_guard<std::mutex> lock(mu);
    flacInErrSet = true; flacInErrReason = (uint32_t)(key & 0xFFu);
    const FlacInSet& set = flacInSets[half];
    flacInErrStream = rec < set.frames.size() ? set.frames[rec].stream : 0u;
    flacInErrFrame = rec < set.frames.size() ? set.frames[rec].index : 0u;
    // (what the failed frame left in the scratch went into the digest: the slot is broken; so is every slot another failed frame of the
    //  set may belong to — the record names the first one only)
    if (!set.jobs.empty()) for (size_t s = 0; s < set.jobs.size() && s < flacInMd5Slots.size(); ++s)
        if (s == flacInErrStream || e.count > 1u) flacInMd5Slots[s].state = fi::kBroken;
    return true;
}

// ---- option "flac_in_md5" ---------------------------------------------------------------------------------------------------------------------
int Engine::ensureFlacInMd5() {
    if (dFlacInMd5) return kOk;
    const size_t S = kMaxHostIn;
    HIP_OK(hipMalloc((void**)&dFlacInMd5, S * (sizeof(flac_md5::Record) + 16u)));
    HIP_OK(hipHostMalloc((void**)&hFlacInMd5, S * 16u, hipHostMallocDefault));
    std::memset(hFlacInMd5, 0, S * 16u);
    return flacInMd5ResetLocked();
}

// every slot off, every record at its initial value (a slot that is fed for the first time finds it so)
int Engine::flacInMd5ResetLocked() {
    flacInMd5Slots.clear();
    if (!dFlacInMd5) return kOk;
    if (hipSetDevice(device) != hipSuccess) return kHipError;
    HIP_OK(hipStreamSynchronize(stream));
    if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
    std::vector<flac_md5::Record> fresh(kMaxHostIn);
    for (flac_md5::Record& r : fresh) flac_md5::init(r);
    HIP_OK(hipMemcpy(dFlacInMd5, fresh.data(), fresh.size() * sizeof(flac_md5::Record), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(flacInMd5Digests(), 0, (size_t)kMaxHostIn * 16u));
    std::memset(hFlacInMd5, 0, (size_t)kMaxHostIn * 16u);
    return kOk;
}

int Engine::flacInMd5Reset() {
    RenderGuard lock(*this);
    return flacInMd5ResetLocked();
}

int Engine::flacInMd5Read(uint8_t* digests, uint32_t* states, uint64_t* hashed, size_t capacity, size_t* slots) {
    RenderGuard lock(*this);
    const size_t S = flacInMd5Slots.size();
    if (slots) *slots = S;
    if (!digests && !states && !hashed) return kOk;
    if (capacity < S) return kInvalidPropertyValue;
    if (dFlacInMd5) {       // what is in flight: the digests come back on the copy stream behind the set that finished them
        if (hipSetDevice(device) != hipSuccess) return kHipError;
        HIP_OK(hipStreamSynchronize(stream));
        if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
    }
    for (size_t s = 0; s < S; ++s) {
        const fi::Slot& sl = flacInMd5Slots[s];
        if (states) states[s] = sl.state;
        if (hashed) hashed[s] = sl.state == fi::kOff ? 0u : sl.hashedTo;
        if (digests) { if (sl.state == fi::kComplete && hFlacInMd5) std::memcpy(digests + 16u * s, hFlacInMd5 + 16u * s, 16u); else std::memset(digests + 16u * s, 0, 16u); }
    }
    return kOk;
}

// The rule per stream of a planned set (flac_in_md5::advance): the set decodes its covered frames whole, stream samples [c0, c1); what
// of them is new enters the digest, and the launch that takes a stream's last sample finishes it. The jobs go into the pinned half.
fi::Job Engine::flacInMd5Job(const FlacIn& f, const FlacInSet& set, size_t s, fi::Slot& slot) {
    const FlacInStream& st = set.streams[s];
    fi::Job j{};
    if (st.frames == 0u) return j;
    const uint64_t total = fi::total_of(f.totalSamples, f.frames ? f.frameFirstSamples[f.frames] : 0u);
    const uint64_t c0 = f.frameFirstSamples[set.frames[st.firstFrame].index], c1 = c0 + st.covered;
    uint64_t lo = 0; bool finish = false;
    if (!fi::advance(slot, f.bits, f.channels, total, c0, c1, lo, finish)) return j;
    j.base = st.scratchBase; j.stride = st.covered; j.first = (uint32_t)(lo - c0); j.count = (uint32_t)(c1 - lo); j.finish = finish ? 1u : 0u;
    return j;
}

void Engine::flacInMd5Jobs(const PcmSource& src, FlacInSet& set, int half) {
    const size_t S = set.streams.size();
    if (flacInMd5Slots.size() < S) flacInMd5Slots.resize(S, fi::Slot{});
    set.md5Work = set.md5Finish = false;
    for (size_t s = 0; s < S && s < set.jobs.size(); ++s) {
        const fi::Job j = set.jobs[s] = flacInMd5Job(*static_cast<const FlacIn*>(src.streams[s]), set, s, flacInMd5Slots[s]);
        set.md5Work = set.md5Work || j.count || j.finish; set.md5Finish = set.md5Finish || j.finish;
    }
    if (!set.jobs.empty()) std::memcpy(hFlacIn[half] + set.jobsOff, set.jobs.data(), set.jobs.size() * sizeof(fi::Job));
}

int Engine::flacInMd5Launch(const FlacInSet& set, int half, uint32_t G, uint32_t bits) {
    if (!set.md5Work) return kOk;
    if (!dFlacInMd5 || set.jobs.size() > kMaxHostIn || set.jobsOff + set.jobs.size() * sizeof(fi::Job) > flacInBytes) return kInvariantViolation;
    FlacInMd5Args a{};
    a.scratch = dFlacInScratch; a.records = flacInMd5Records(); a.digests = flacInMd5Digests();
    a.jobs = reinterpret_cast<const fi::Job*>(dFlacIn[half] + set.jobsOff);
    a.numStreams = (uint32_t)set.jobs.size(); a.G = G; a.bits = bits;
    HIP_OK(launch_flac_in_md5(stream, a, set.jobs.data(), set.scratchInts));
    return kOk;
}

int Engine::flacInError(uint32_t* stream, uint64_t* frame, uint32_t* reason) {
    std::lock_guard<std::mutex> lock(mu);
    if (!flacInErrSet) return kInvalidPropertyValue;
    if (stream) *stream = flacInErrStream;
    if (frame) *frame = flacInErrFrame;
    if (reason) *reason = flacInErrReason;
    return kOk;
}

// the block-by-block path: input frames [from, from + n) of the call decoded on the host (decode_host) into the interleaved image
// unpack_host reads — the kernels' functions, the kernels' bits (`mu` held)
int Engine::flacInHostImage(const PcmSource& src, uint64_t from, size_t n, std::vector<std::vector<unsigned char>>& images, flac_md5::Record* md5) {
    const uint32_t G = src.channelsPerStream, bits = flacInBits(src), B = bits <= 16u ? 2u : 3u;
    images.resize(src.nStreams);
    std::vector<int32_t> codes((size_t)G * std::max<size_t>(n, 1));
    int32_t* planar[fd::kMaxChannels];
    for (uint32_t g = 0; g < G; ++g) planar[g] = codes.data() + (size_t)g * std::max<size_t>(n, 1);
    for (size_t s = 0; s < src.nStreams; ++s) {
        const FlacIn& f = *static_cast<const FlacIn*>(src.streams[s]);
        size_t bad = 0;
        const uint32_t r = fd::decode_host(f.data, f.frameOffsets, f.frameFirstSamples, (size_t)f.frames, G, bits, f.position + from, n, planar, &bad);
        if (flacInMd5Slots.size() < src.nStreams) flacInMd5Slots.resize(src.nStreams, fi::Slot{});
        if (r != fd::OK) {
            flacInErrSet = true; flacInErrStream = (uint32_t)s; flacInErrFrame = bad; flacInErrReason = r;
            if (md5) flacInMd5Slots[s].state = fi::kBroken;
            return kFlacInput;
        }
        if (md5) {
            // option "flac_in_md5": the range this block decoded, [c0, c1) of the stream, under the launch sets' rule, through the
            // kernel's scalar twin on the record brought over for the call
            const uint64_t closing = f.frames ? f.frameFirstSamples[f.frames] : 0u, total = fi::total_of(f.totalSamples, closing);
            const uint64_t c0 = f.position + from, c1 = std::min<uint64_t>(c0 + n, closing);
            uint64_t lo = 0; bool finish = false;
            if (c0 < closing && c0 >= f.frameFirstSamples[0] && fi::advance(flacInMd5Slots[s], f.bits, f.channels, total, c0, c1, lo, finish))
                fi::update_codes(md5[s], planar, G, (uint32_t)(lo - c0), c1 - lo, bits, finish ? hFlacInMd5 + 16u * s : nullptr);
        }
        images[s].assign(std::max<size_t>(n * G * B, 1), 0);
        fd::image_host(bits, G, planar, n, images[s].data());
    }
    return kOk;
}

} // namespace elemhip
