// engine_host_blocks.cpp — the block-by-block host render (renderHostBlocks): taps under a host block longer than the engine's, and ragged
// slices. Every slice needs its own stretch of the shared tap buffers (setTapSlice), which launch sets do not do, so every host block goes
// through process() and each delivery stage runs on the host through its header's scalar twin — the kernel's functions, the kernel's bits —
// with the stage's carried state brought over from the device for the call and taken back afterwards. No kernels of its own, no events,
// no second stream; renderHostSets (engine_render.cpp) decides between this and its launch-set loop.
#include "engine_impl.h"
#include "pcm_unpack.h"
#include "flac_encode.h"
#include "flac_md5.h"
#include <functional>

namespace elemhip {

namespace {
struct Span { void* host; void* dev; size_t bytes; };      // a piece of carried state, as it lies on either side
// One stage's carried state. Opening: `ensure`, then the spans device -> host. Closing: the same spans host -> device, then `closed`.
// Abandoning (the call failed): what `abandon` says. One driver (HostCarry::sync / open / abandon / close) does this for every stage.
struct Carried {
    bool on;
    std::function<int()> ensure;                       // (`mu` held) the device side exists, the host copy is sized
    std::function<std::vector<Span>()> spans;          // (`mu` held, the stream idle) where the state lies right now
    enum { kWriteBack, kReset, kNothing } abandon;     // the state goes back as it is / the programme starts anew / nothing
    std::function<int()> reset;                        // (`mu` held) kReset's
    std::function<void()> closed;                      // (`mu` held) what else a write-back settles
};
}

// the carried state of a call, on the host: the stages in the order they open, and the one unwind
struct Engine::HostCarry {
    Engine& e; const HostCall& c;
    std::vector<loudness::ChannelState> meterState;
    std::vector<float> resHist, inHist;
    std::vector<unsigned char> limState; std::vector<limiter::GroupStats> limStats;
    std::vector<std::vector<int32_t>> flacCodes;        // FLAC delivery: the open frame's codes per channel
    std::vector<flac_md5::Record> flacMd5;              // ... and, with option "flac_md5", the streams' running digests
    std::vector<flac_md5::Record> flacInMd5;            // option "flac_in_md5": the input slots' running digests
    std::vector<noise_shape::ChannelState> shapeState;  // noise-shaped requantisation: the channels' errors
    std::vector<float> spcTail; std::vector<double> spcSums;      // the spectrum analyser: the carried frames, the running sums
    std::vector<qc::ChannelState> qcState; std::vector<qc::PairState> qcPairState;      // the inspector: the programme's summaries
    std::vector<Carried> stages;
    size_t opened = 0;                                  // stages [0, opened) are open

    HostCarry(Engine& eng, const HostCall& call) : e(eng), c(call) {
        stages = {
            // the meter: the floats are here, the header's scalar loop meters them; a failed call's frames were not metered
            {c.meter, [this] { meterState.resize(c.nOut); return e.ensureLoudness(c.nOut, 0); },
             [this] { return std::vector<Span>{{meterState.data(), e.dLoudState, c.nOut * sizeof(loudness::ChannelState)}}; }, Carried::kWriteBack, nullptr, nullptr},
            // the delivery-rate converter's carried frames
            {c.resamp, [this] { resHist.resize(c.nOut * (size_t)c.rp.H); return e.ensureResample(c.nOut, 0); },
             [this] { return std::vector<Span>{{resHist.data(), e.dResHist[e.resHistCur], resHist.size() * sizeof(float)}}; },
             Carried::kReset, [this] { return e.resampleResetLocked(0); }, nullptr},
            // the limiter's state and statistics
            {c.limit, [this] { limState.resize(limiter::state_bytes(c.lmp, (uint32_t)c.nOut)); limStats.resize(limiter::group_count(c.lmp, (uint32_t)c.nOut)); return e.ensureLimiter(c.nOut, 0, 0); },
             [this] { return std::vector<Span>{{limState.data(), e.dLimState[e.limCur], limState.size()},
                                               {limStats.data(), e.dLimStats, limStats.size() * sizeof(limiter::GroupStats)}}; },
             Carried::kReset, [this] { return e.limiterResetLocked(0); }, nullptr},
            // the input-rate converter's carried frames
            {c.inres, [this] { inHist.resize(c.nIn * (size_t)c.inp.H); return e.ensureInputResample(c.nIn); },
             [this] { return std::vector<Span>{{inHist.data(), e.dInHist[e.inHistCur], inHist.size() * sizeof(float)}}; },
             Carried::kReset, [this] { return e.inputResampleResetLocked(0); }, nullptr},
            // the error-feedback quantiser's states
            {c.shape, [this] { shapeState.resize(c.nOut); return e.ensureNoiseShape(c.nOut, 0); },
             [this] { return std::vector<Span>{{shapeState.data(), e.dNsState, shapeState.size() * sizeof(noise_shape::ChannelState)}}; },
             Carried::kReset, [this] { return e.noiseShapeResetLocked(); }, nullptr},
            // FLAC delivery: the open frame's codes (processBlocksFlac resets the programme itself when the call fails)
            {c.flac != nullptr, [this] { const int rc = e.ensureFlac(*c.flac, 0);
                                         if (rc == kOk) { flacCodes.assign(c.nOut, std::vector<int32_t>(e.flacOpen)); flacMd5.resize(e.flacMd5 ? e.flacStreams : 0u); }
                                         return rc; },
             [this] { std::vector<Span> s;
                      for (auto& codes : flacCodes) s.push_back({codes.data(), e.dFlacCarry + s.size() * flac_encode::kMaxFrame, codes.size() * sizeof(int32_t)});
                      if (!flacMd5.empty()) s.push_back({flacMd5.data(), e.dFlacMd5, flacMd5.size() * sizeof(flac_md5::Record)});
                      return s; },
             Carried::kNothing, nullptr, [this] { e.flacOpen = (uint32_t)flacCodes[0].size(); }},
            // option "flac_in_md5": the input slots' records (the slots' states live on the host and stay with what was hashed)
            {c.inMd5, [this] { flacInMd5.resize(c.src->nStreams); return e.ensureFlacInMd5(); },
             [this] { return std::vector<Span>{{flacInMd5.data(), e.dFlacInMd5, flacInMd5.size() * sizeof(flac_md5::Record)}}; }, Carried::kWriteBack, nullptr, nullptr},
            // the spectrum analyser: the carried frames and the running sums; a failed call starts a new programme
            {c.spectrum, [this] { const int rc = e.ensureSpectrum(c.nOut, 0);
                                  if (rc == kOk) { spcTail.resize(c.nOut * (size_t)(e.spcPlan.size - 1u)); spcSums.resize(c.nOut * (size_t)e.spcPlan.cols); }
                                  return rc; },
             [this] { return std::vector<Span>{{spcTail.data(), e.dSpcTail[e.spcTailCur], spcTail.size() * sizeof(float)},
                                               {spcSums.data(), e.dSpcSums, spcSums.size() * sizeof(double)}}; },
             Carried::kReset, [this] { return e.spectrumResetLocked(e.spcChannels); }, nullptr},
            // the inspector: the channels' and the pairs' summaries; a failed call starts a new programme
            {c.qc, [this] { const int rc = e.ensureQc(c.nOut, 0);
                            if (rc == kOk) { qcState.resize(c.nOut); qcPairState.resize(e.qcPairs.size() / 2u); }
                            return rc; },
             [this] { return std::vector<Span>{{qcState.data(), e.dQcState, qcState.size() * sizeof(qc::ChannelState)},
                                               {qcPairState.data(), e.dQcPairState, qcPairState.size() * sizeof(qc::PairState)}}; },
             Carried::kReset, [this] { return e.qcResetLocked(e.qcChannels); }, nullptr},
        };
    }

    // the common body of a round trip (a guard of its own: nothing that locks is called under it)
    int sync(Carried& s, bool toHost) {
        RenderGuard lock(e);
        if (hipSetDevice(e.device) != hipSuccess) return kHipError;
        if (toHost) { const int rc = s.ensure(); if (rc != kOk) return rc; }
        HIP_OK(hipStreamSynchronize(e.stream));
        for (const Span& p : s.spans())
            if (p.bytes) HIP_OK(toHost ? hipMemcpy(p.host, p.dev, p.bytes, hipMemcpyDeviceToHost) : hipMemcpy(p.dev, p.host, p.bytes, hipMemcpyHostToDevice));
        if (!toHost && s.closed) s.closed();
        return kOk;
    }
    int open() {         // a stage that does not open abandons those in front of it
        for (; opened < stages.size(); ++opened)
            if (stages[opened].on) { const int rc = sync(stages[opened], true); if (rc != kOk) { abandon(); return rc; } }
        return kOk;
    }
    void resetProgrammes() {
        for (size_t i = 0; i < opened; ++i) if (stages[i].on && stages[i].abandon == Carried::kReset) { RenderGuard lock(e); (void)stages[i].reset(); }
    }
    void abandon() {     // (no lock held)
        for (size_t i = 0; i < opened; ++i) if (stages[i].on && stages[i].abandon == Carried::kWriteBack) (void)sync(stages[i], false);
        resetProgrammes();
    }
    int close() {        // every stage is written back; the first failure is the call's code and leaves the resettable programmes new
        int rc = kOk;
        for (size_t i = 0; i < opened; ++i) if (stages[i].on) { const int r = sync(stages[i], false); if (rc == kOk) rc = r; }
        if (rc != kOk) resetProgrammes();
        return rc;
    }

    // FLAC delivery of a host block's nd delivered frames: quantised here behind the open frame's codes, and the header's scalar twin
    // encodes every frame they complete
    // (`shaped`: null, or the codes of `got`'s frames where noise_shape::shape_host left them, rows gotStride apart)
    int encodeFlac(const float* got, size_t gotStride, size_t nd, int64_t gotTime, const int32_t* shaped) {
        std::lock_guard<std::mutex> lock(e.mu);
        FlacJob* flac = c.flac;
        const uint64_t lead = std::min<uint64_t>(flac->dropLeft, nd), enter = std::min<uint64_t>(flac->takeLeft, nd - lead);
        flac->dropLeft -= lead; flac->takeLeft -= enter;
        const uint32_t G = flac->spec.channelsPerStream, bits = flac->spec.bits, ff = e.flacFF;
        for (size_t ch = 0; ch < c.nOut; ++ch) {
            const uint32_t k0 = pcm_pack::channel_key(flac->spec.seed, (uint32_t)ch);
            pcm_pack::ChannelStats st{flac->tally.peakBits[ch], 0u, 0u};
            for (size_t f = (size_t)lead; f < (size_t)(lead + enter); ++f) {
                const float x = got[ch * gotStride + f];
                st = pcm_pack::stats_fold(x, st);
                flacCodes[ch].push_back(shaped ? shaped[ch * gotStride + f]
                                               : pcm_pack::quantise(x, bits, flac->spec.dither ? pcm_pack::dither(k0, gotTime + (int64_t)f) : 0.0f));
            }
            flac->tally.peakBits[ch] = st.peakBits; flac->tally.over[ch] += st.over; flac->tally.nonfinite[ch] += st.nonfinite;
        }
        // the codes that entered go into their streams' digests, as flac_md5.hip takes a launch set's
        for (size_t s = 0; s < flacMd5.size(); ++s) {
            const int32_t* planar[flac_encode::kMaxChannels];
            for (uint32_t g = 0; g < G; ++g) planar[g] = flacCodes[s * G + g].data();
            flac_md5::update_codes(flacMd5[s], planar, G, (uint32_t)(flacCodes[s * G].size() - (size_t)enter), enter, bits);
        }
        e.flacFrames += enter;
        const size_t nF = flacCodes[0].size() / ff;
        if (nF == 0) return kOk;
        if (e.flacEmitted + nF > 0x7FFFFFFFull) return kInvariantViolation;
        std::vector<uint32_t> lens(nF);
        for (size_t s = 0; s < flac->nStreams; ++s) {
            const int32_t* planar[flac_encode::kMaxChannels];
            for (uint32_t g = 0; g < G; ++g) planar[g] = flacCodes[s * G + g].data();
            size_t count = 0;
            const size_t n = flac_encode::encode_host(planar, G, nF * ff, ff, bits, e.flacRate, (uint32_t)e.flacEmitted, false,
                                                      static_cast<uint8_t*>(flac->streams[s]) + flac->bytes[s], flac->caps[s] - flac->bytes[s], lens.data(), &count, e.flacLpc);
            if (n == (size_t)-1 || count != nF) return kInvariantViolation;
            flac->bytes[s] += n;
            e.flacFrameBytes[s].insert(e.flacFrameBytes[s].end(), lens.begin(), lens.end());
        }
        for (size_t ch = 0; ch < c.nOut; ++ch) flacCodes[ch].erase(flacCodes[ch].begin(), flacCodes[ch].begin() + (ptrdiff_t)(nF * ff));
        e.flacEmitted += nF;
        return kOk;
    }
};

// Host block by host block through process(), which is called with no lock held; every host stage step takes `mu` for itself.
int Engine::renderHostBlocks(const HostCall& c) {
    const float* const* in = c.in; float* const* out = c.out;
    const size_t nIn = c.nIn, nOut = c.nOut, hb = c.hb, numFrames = c.numFrames;
    const PcmSource* src = c.src; PcmJob* pcm = c.pcm;
    const bool staged = c.packed || c.meter || c.resamp || c.limit || c.spectrum || c.qc;      // every host block renders into tailOut: a stage reads it there
    const AutoLanes* lanes = c.lanes.get();
    std::vector<const float*> ip(c.nEng);       // the supplied channels, then the lanes' (automationSet)
    std::vector<float*> op(nOut);
    std::vector<float> tailIn, tailOut, inX, resOut, limOut, spcOut, laneIn, qcOut;
    std::vector<int32_t> shaped;
    std::vector<uint8_t*> sp(pcm ? pcm->nStreams : 0);
    std::vector<const unsigned char*> srcAt(src ? src->nStreams : 0);
    std::vector<std::vector<unsigned char>> flacImg;
    HostCarry carry(*this, c);
    { const int rc = carry.open(); if (rc != kOk) return rc; }
    size_t inOff = 0, outOff = 0;           // input frames of this call consumed so far, and frames delivered
    for (size_t f0 = 0; f0 < numFrames; f0 += hb) {
        const size_t nf = std::min(hb, numFrames - f0);
        for (size_t ch = 0; ch < nIn; ++ch) ip[ch] = src ? nullptr : in[ch] + f0;
        for (size_t ch = 0; ch < nOut; ++ch) op[ch] = c.wantFloat ? out[ch] + f0 : nullptr;
        if (nf < hb || staged) {
            // the last, partly filled host block is still a whole block to the engine (offline-renderer/index.ts:104-131: inputs
            // padded with zeros, the frames beyond the caller's arrays dropped); a PCM call renders every host block here
            tailOut.assign(nOut * hb, 0.0f);
            for (size_t ch = 0; ch < nOut; ++ch) op[ch] = tailOut.data() + ch * hb;
        }
        int flacInRc = kOk;       // a FLAC source is decoded on the host in front of unpack_host (decode_host): the kernels' bits
        if (c.inres) {
            // the stretch this host block's nf engine frames pull, from the input cursor on: decoded where it is PCM, then converted
            // into the block's rows (zeros behind nf)
            std::lock_guard<std::mutex> lock(mu);
            const size_t ni = (size_t)(resample::inputs_before(c.inp, inFramesOut + nf) - inFramesIn), stride = std::max<size_t>(ni, 1);
            tailIn.assign(nIn * hb, 0.0f);
            if (c.flacSrc) flacInRc = flacInHostImage(*src, inOff, ni, flacImg, c.inMd5 ? carry.flacInMd5.data() : nullptr);
            if (src && flacInRc == kOk) {
                inX.resize(nIn * stride);
                for (size_t s = 0; s < src->nStreams; ++s) srcAt[s] = c.flacSrc ? flacImg[s].data() : c.inStream(s) + inOff * c.srcG * c.srcB;
                pcm_unpack::unpack_host(c.srcFmt, c.srcG, (uint32_t)src->nStreams, srcAt.data(), ni, inX.data(), stride, ni);
            }
            for (size_t ch = 0; ch < nIn && flacInRc == kOk; ++ch) {
                (void)resample::resample_in_host(c.inp, inTable.data(), inRowBase.data(), carry.inHist.data() + ch * c.inp.H, src ? inX.data() + ch * stride : in[ch] + inOff,
                                                 inFramesOut, nf, tailIn.data() + ch * hb);
                ip[ch] = tailIn.data() + ch * hb;
            }
            inOff += ni; inFramesIn += ni; inFramesOut += nf;
        } else if (src) {
            // the inputs are needed on the host: the header's scalar loop unpacks them — the kernel's functions, the kernel's floats
            tailIn.resize(nIn * hb);
            if (c.flacSrc) { std::lock_guard<std::mutex> lock(mu); flacInRc = flacInHostImage(*src, f0, nf, flacImg, c.inMd5 ? carry.flacInMd5.data() : nullptr); }
            for (size_t s = 0; s < src->nStreams && flacInRc == kOk; ++s)
                srcAt[s] = c.flacSrc ? flacImg[s].data() : static_cast<const unsigned char*>(src->streams[s]) + f0 * c.srcG * c.srcB;
            if (flacInRc == kOk) pcm_unpack::unpack_host(c.srcFmt, c.srcG, (uint32_t)src->nStreams, srcAt.data(), nf, tailIn.data(), hb, hb);
            for (size_t ch = 0; ch < nIn; ++ch) ip[ch] = tailIn.data() + ch * hb;
        } else if (nf < hb) {
            tailIn.assign(nIn * hb, 0.0f);
            for (size_t ch = 0; ch < nIn; ++ch) { std::memcpy(tailIn.data() + ch * hb, in[ch] + f0, nf * sizeof(float)); ip[ch] = tailIn.data() + ch * hb; }
        }
        if (lanes) {
            // the lane channels' rows of this host block from the header's scalar twin — the kernel's functions, the kernel's floats:
            // the lanes' values at the block's nf frames, zeros behind them and in a channel without a lane
            laneIn.assign((c.nEng - nIn) * hb, 0.0f);
            for (size_t ch = nIn; ch < c.nEng; ++ch) {
                float* row = laneIn.data() + (ch - nIn) * hb;
                if (lanes->count[ch]) automation::value_host(lanes->points.data() + lanes->offset[ch], lanes->count[ch], c.sampleTime + (int64_t)f0, nf, row);
                ip[ch] = row;
            }
        }
        const int rc = flacInRc != kOk ? flacInRc : process(ip.data(), c.nEng, op.data(), nOut, hb, c.sampleTime + (int64_t)f0);
        if (rc != kOk) { carry.abandon(); return rc; }
        // what is delivered of this host block: its nf frames, or their conversion
        const float* got = tailOut.data();
        size_t gotStride = hb, nd = nf, at = f0;
        int64_t gotTime = c.sampleTime + (int64_t)f0;
        if (c.resamp) {
            std::lock_guard<std::mutex> lock(mu);
            nd = (size_t)(resample::outputs_before(c.rp, resFramesIn + nf) - resample::outputs_before(c.rp, resFramesIn));
            gotStride = std::max<size_t>(nd, 1);
            resOut.resize(nOut * gotStride);
            for (size_t ch = 0; ch < nOut; ++ch)
                (void)resample::resample_host(c.rp, resTable.data(), resRowBase.data(), carry.resHist.data() + ch * c.rp.H, tailOut.data() + ch * hb, nf, resFramesIn,
                                              resOut.data() + ch * gotStride);
            got = resOut.data(); at = outOff; gotTime = (int64_t)resFramesOut;
            resFramesIn += nf; resFramesOut += nd;
        }
        if (c.limit && nd) {
            std::lock_guard<std::mutex> lock(mu);
            limOut.resize(nOut * gotStride);
            limiter::limiter_host(limMeter, c.lmp, (uint32_t)nOut, carry.limState.data(), carry.limStats.data(), got, gotStride, nd, limFrames, limOut.data(), gotStride);
            got = limOut.data();
            limFrames += nd;
        }
        if (c.meter) {
            std::lock_guard<std::mutex> lock(mu);
            for (size_t ch = 0; ch < nOut; ++ch)
                loudness::meter_host(loudPlan, carry.meterState[ch], got + ch * gotStride, nd, loudFrames, [&](double ms) { loudSeries[ch].push_back(ms); });
            loudFrames += nd;
        }
        if (c.spectrum && nd) {
            // the floats are on the host: the header's scalar twin frames and transforms them — the kernel's phases, thread by thread
            std::lock_guard<std::mutex> lock(mu);
            const spectrum::Plan& sp = spcPlan;
            const uint64_t j0 = spcEmitted, j1 = spectrum::frames_complete(spcFrames + nd, sp.size, sp.hop, sp.pad);
            spcOut.resize((size_t)(j1 - j0) * sp.cols);
            for (size_t ch = 0; ch < nOut; ++ch) {
                spectrum::analyse_host(sp, carry.spcTail.data() + ch * (sp.size - 1u), got + ch * gotStride, nd, spcFrames, j0, j1, spcOut.data(),
                                       carry.spcSums.data() + ch * sp.cols);
                spcQueue[ch].insert(spcQueue[ch].end(), spcOut.begin(), spcOut.end());
            }
            spcFrames += nd; spcEmitted = j1;
        }
        if (c.qc && nd) {
            // the floats are on the host: the header's scalar twin inspects the frames the window lets in — the kernel's functions
            std::lock_guard<std::mutex> lock(mu);
            const qc::Window w = qc::window(qcDelivered, qcFrames, qcSkip, qcLimit, nd);
            const uint32_t buckets = qc::buckets_complete(qcFrames, w.count, qcSpec.bucket);
            qcOut.resize((size_t)buckets * 2u);
            for (size_t ch = 0; ch < nOut; ++ch) {
                qc::channel_host(qcSpec, carry.qcState[ch], got + ch * gotStride + w.q0, w.count, qcFrames, qcOut.data());
                qcQueue[ch].insert(qcQueue[ch].end(), qcOut.begin(), qcOut.end());
            }
            for (size_t k = 0; k < carry.qcPairState.size(); ++k)
                qc::pair_host(carry.qcPairState[k], got + qcPairs[2u * k] * gotStride + w.q0, got + qcPairs[2u * k + 1u] * gotStride + w.q0, w.count, qcFrames, qcSpec);
            qcDelivered += nd; qcFrames += w.count;
        }
        if (c.shape && nd) {
            // the floats are on the host: the header's scalar loop quantises all nd of them — the kernel's functions, the kernel's bits
            std::lock_guard<std::mutex> lock(mu);
            shaped.resize(nOut * gotStride);
            noise_shape::shape_host(nsCq, nsTaps, c.shapeBits, c.shapeDither != 0u, c.shapeSeed, 0u, gotTime, got, (uint32_t)nOut, gotStride, nd,
                                    carry.shapeState.data(), shaped.data());
            nsFrames += nd;
        }
        const int32_t* codes = c.shape && nd ? shaped.data() : nullptr;
        if ((nf < hb || staged) && c.wantFloat) for (size_t ch = 0; ch < nOut; ++ch) std::memcpy(out[ch] + at, got + ch * gotStride, nd * sizeof(float));
        if (pcm) {
            // the floats are on the host: the header's scalar loop packs them — the kernel's functions, the kernel's bits
            for (size_t s = 0; s < pcm->nStreams; ++s) sp[s] = static_cast<uint8_t*>(pcm->streams[s]) + at * c.pcmG * c.pcmB;
            pcm_pack::pack_host(c.pcmFmt, c.pcmG, (uint32_t)pcm->nStreams, pcm->spec.dither != 0u, pcm->spec.seed, got, gotStride, nd,
                                gotTime, sp.data(), pcm->tally.peakBits.data(), pcm->tally.over.data(), pcm->tally.nonfinite.data(), codes);
        }
        if (c.flac) {
            const int rf = carry.encodeFlac(got, gotStride, nd, gotTime, codes);
            if (rf != kOk) { carry.abandon(); return rf; }
        }
        outOff += nd;
    }
    return carry.close();
}

} // namespace elemhip
