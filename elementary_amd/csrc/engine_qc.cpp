// engine_qc.cpp — the host side of the inspector (elemhip_qc_set; qc.h, qc.hip): the spec, the carried state's and the scratch buffers'
// life, the queue of overview buckets, the read-out and the reset. The set loop that launches the kernels is renderHostSets
// (engine_render.cpp); the host-block renderer runs the header's scalar twin on the same state.
#include "engine_impl.h"

namespace elemhip {

void Engine::qcFree() {
    for (int k = 0; k < 2; ++k) {
        if (dQcOut[k]) (void)hipFree(dQcOut[k]);
        if (hQcOut[k]) (void)hipHostFree(hQcOut[k]);
        dQcOut[k] = hQcOut[k] = nullptr;
    }
    if (dQcState) (void)hipFree(dQcState);
    if (dQcPairState) (void)hipFree(dQcPairState);
    if (dQcPairs) (void)hipFree(dQcPairs);
    if (dQcTiles) (void)hipFree(dQcTiles);
    if (dQcLeaves) (void)hipFree(dQcLeaves);
    if (dQcEdges) (void)hipFree(dQcEdges);
    dQcState = nullptr; dQcPairState = nullptr; dQcPairs = nullptr; dQcTiles = nullptr; dQcLeaves = nullptr; dQcEdges = nullptr;
    qcStateCap = qcSetCap = qcScratchChannels = qcOutCap = qcOutChannels = 0;
}

// a new programme of `channels` channels (0: the count is set by the first inspected call); buckets nobody read are dropped; `mu` held
int Engine::qcResetLocked(size_t channels) {
    qcChannels = 0; qcFrames = qcDelivered = 0; qcQueueFirst = 0;
    qcQueue.clear();
    if (dry || !qcOn) return kOk;
    if (hipSetDevice(device) != hipSuccess) return kHipError;
    HIP_OK(hipStreamSynchronize(stream));
    if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
    const size_t np = qcPairs.size() / 2u;
    if (channels > qcStateCap) {
        if (dQcState) (void)hipFree(dQcState);
        dQcState = nullptr; qcStateCap = 0;
        HIP_OK(hipMalloc((void**)&dQcState, channels * sizeof(qc::ChannelState)));
        qcStateCap = channels;
    }
    if (np && !dQcPairState) {
        HIP_OK(hipMalloc((void**)&dQcPairState, np * sizeof(qc::PairState)));
        HIP_OK(hipMalloc((void**)&dQcPairs, 2u * np * sizeof(uint32_t)));
        HIP_OK(hipMemcpy(dQcPairs, qcPairs.data(), 2u * np * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (channels) {
        const std::vector<qc::ChannelState> fresh(channels, qc::state_empty());
        HIP_OK(hipMemcpy(dQcState, fresh.data(), channels * sizeof(qc::ChannelState), hipMemcpyHostToDevice));
    }
    if (np) HIP_OK(hipMemset(dQcPairState, 0, np * sizeof(qc::PairState)));
    qcChannels = (uint32_t)channels;
    qcQueue.assign(channels, std::vector<float>());
    return kOk;
}

// (`mu` held) a programme of `channels`; scratch and halves for sets of `setFrames` delivered frames (0: none — the host-block path)
int Engine::ensureQc(size_t channels, size_t setFrames) {
    for (uint32_t c : qcPairs) if (c >= channels) return kInvalidPropertyValue;       // a pair names a channel this call does not deliver
    if (channels != qcChannels) { const int rc = qcResetLocked(channels); if (rc != kOk) return rc; }
    if (setFrames == 0) return kOk;
    const size_t np = qcPairs.size() / 2u;
    if (setFrames > qcSetCap || channels > qcScratchChannels) {
        HIP_OK(hipStreamSynchronize(stream));
        if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
        const size_t ch = std::max(channels, qcScratchChannels), fr = std::max(setFrames, qcSetCap);
        const size_t tiles = fr / qc::kTileFrames + 2u, leaves = fr / qc::kLeaf + 2u;
        if (dQcTiles) (void)hipFree(dQcTiles);
        if (dQcLeaves) (void)hipFree(dQcLeaves);
        if (dQcEdges) (void)hipFree(dQcEdges);
        dQcTiles = nullptr; dQcLeaves = nullptr; dQcEdges = nullptr; qcSetCap = qcScratchChannels = 0;
        HIP_OK(hipMalloc((void**)&dQcTiles, ch * tiles * sizeof(qc::Stretch<uint32_t>)));
        HIP_OK(hipMalloc((void**)&dQcLeaves, (2u * ch + np) * leaves * sizeof(double)));
        HIP_OK(hipMalloc((void**)&dQcEdges, ch * tiles * 4u * sizeof(float)));
        qcSetCap = fr; qcScratchChannels = ch;
    }
    const size_t buckets = qcSpec.bucket ? setFrames / qcSpec.bucket + 1u : 0u;
    if (buckets > qcOutCap || (buckets && channels > qcOutChannels)) {
        HIP_OK(hipStreamSynchronize(stream));
        if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
        const size_t ch = std::max(channels, qcOutChannels), n = std::max(buckets, qcOutCap), bytes = ch * n * 2u * sizeof(float);
        for (int k = 0; k < 2; ++k) {
            if (dQcOut[k]) (void)hipFree(dQcOut[k]);
            if (hQcOut[k]) (void)hipHostFree(hQcOut[k]);
            dQcOut[k] = hQcOut[k] = nullptr;
        }
        qcOutCap = qcOutChannels = 0;
        for (int k = 0; k < 2; ++k) {
            HIP_OK(hipMalloc((void**)&dQcOut[k], bytes));
            HIP_OK(hipHostMalloc((void**)&hQcOut[k], bytes, hipHostMallocDefault));
        }
        qcOutCap = n; qcOutChannels = ch;
    }
    return kOk;
}

int Engine::qcSet(const QcSpec* spec) {
    RenderGuard lock(*this);
    if (spec) {
        if (!qc::spec_ok(spec->silenceLevel, spec->clipLevel, spec->clipRun, spec->dropoutFrames, spec->bucket, spec->numPairs) || (spec->numPairs && !spec->pairs))
            return kInvalidPropertyValue;
        for (uint32_t k = 0; k < spec->numPairs; ++k) if (spec->pairs[2u * k] == spec->pairs[2u * k + 1u]) return kInvalidPropertyValue;
    }
    if (!dry && (qcOn || spec)) {
        if (hipSetDevice(device) != hipSuccess) return kHipError;
        HIP_OK(hipStreamSynchronize(stream));
        if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
        qcFree();
    }
    qcOn = false;
    (void)qcResetLocked(0);
    qcSpec = qc::Spec{}; qcPairs.clear(); qcSkip = qcLimit = 0;
    if (!spec) return kOk;
    qcSpec = qc::Spec{spec->silenceLevel, spec->clipLevel, spec->clipRun, spec->dropoutFrames, spec->bucket, spec->numPairs};
    qcPairs.assign(spec->pairs, spec->pairs + 2u * (size_t)spec->numPairs);
    qcSkip = spec->skip; qcLimit = spec->limit;
    qcOn = true;
    return kOk;
}

int Engine::qcReset() {
    if (dry) return kNoDevice;
    RenderGuard lock(*this);
    if (!qcOn) return kInvalidPropertyValue;
    return qcResetLocked(0);
}

int Engine::qcRead(QcInfo* info, qc::ChannelReport* channels, size_t channelCap, double* pairSums, size_t pairCap) {
    if (dry) return kNoDevice;
    RenderGuard lock(*this);
    if (!qcOn) return kInvalidPropertyValue;
    const size_t ch = qcChannels, np = qcPairs.size() / 2u, queued = ch ? qcQueue[0].size() / 2u : 0;
    if (info) *info = QcInfo{(uint32_t)ch, (uint32_t)np, qcSpec.bucket, 0u, qcFrames, qcDelivered, qcQueueFirst, queued};
    if ((channels && channelCap < ch) || (pairSums && pairCap < np)) return kInvalidPropertyValue;
    if ((channels && ch) || (pairSums && np)) {
        // (every inspected call ends with both streams synchronised; copies: the programme may go on)
        if (hipSetDevice(device) != hipSuccess) return kHipError;
        HIP_OK(hipStreamSynchronize(stream));
    }
    if (channels && ch) {
        std::vector<qc::ChannelState> st(ch);
        HIP_OK(hipMemcpy(st.data(), dQcState, ch * sizeof(qc::ChannelState), hipMemcpyDeviceToHost));
        for (size_t c = 0; c < ch; ++c) channels[c] = qc::report(qcSpec, st[c]);
    }
    if (pairSums && np) {
        std::vector<qc::PairState> ps(np);
        if (ch) HIP_OK(hipMemcpy(ps.data(), dQcPairState, np * sizeof(qc::PairState), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < np; ++k) pairSums[k] = ch ? qc::sums_value(ps[k]) : 0.0;
    }
    return kOk;
}

int Engine::qcOverview(float* out, size_t capacity) {
    if (dry) return kNoDevice;
    RenderGuard lock(*this);
    if (!qcOn) return kInvalidPropertyValue;
    const size_t ch = qcChannels, n = ch ? qcQueue[0].size() / 2u : 0;
    if (!out || capacity < ch * n * 2u) return kInvalidPropertyValue;
    for (size_t c = 0; c < ch; ++c) {
        if (n) std::memcpy(out + c * n * 2u, qcQueue[c].data(), n * 2u * sizeof(float));
        qcQueue[c].clear();
    }
    qcQueueFirst += n;
    return kOk;
}

} // namespace elemhip
