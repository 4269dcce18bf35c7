// engine_loudness.cpp — the host side of the loudness meter (option "loudness_meter"; loudness.h, loudness.hip): the carried state's
// and the scratch buffers' life, the read-out and the reset. The set loop that launches the kernels is renderHostSets (engine_render.cpp).
#include "engine_impl.h"

namespace elemhip {

void Engine::loudnessFree() {
    if (dLoudState) (void)hipFree(dLoudState);
    if (dLoudSeg) (void)hipFree(dLoudSeg);
    if (dLoudEnergy) (void)hipFree(dLoudEnergy);
    for (int k = 0; k < 2; ++k) { if (dLoudOut[k]) (void)hipFree(dLoudOut[k]); if (hLoudOut[k]) (void)hipHostFree(hLoudOut[k]); }
    dLoudState = nullptr; dLoudSeg = dLoudEnergy = nullptr; dLoudOut[0] = dLoudOut[1] = hLoudOut[0] = hLoudOut[1] = nullptr;
    loudStateCap = loudSegCap = loudSegChannels = loudOutStride = loudOutChannels = 0;
}

// a new programme of `channels` channels (0: the count is set by the first metered call); `mu` held
int Engine::loudnessResetLocked(size_t channels) {
    if (hipSetDevice(device) != hipSuccess) return kHipError;
    HIP_OK(hipStreamSynchronize(stream));
    if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
    if (channels > loudStateCap) {
        if (dLoudState) (void)hipFree(dLoudState);
        dLoudState = nullptr; loudStateCap = 0;
        HIP_OK(hipMalloc((void**)&dLoudState, channels * sizeof(loudness::ChannelState)));
        loudStateCap = channels;
    }
    if (channels) HIP_OK(hipMemset(dLoudState, 0, channels * sizeof(loudness::ChannelState)));
    loudChannels = (uint32_t)channels; loudFrames = 0;
    loudSeries.assign(channels, std::vector<double>());
    return kOk;
}

int Engine::ensureLoudness(size_t channels, size_t setFrames) {
    if (channels != loudChannels) { const int rc = loudnessResetLocked(channels); if (rc != kOk) return rc; }
    const size_t segs = loudness::segment_count((uint32_t)setFrames, loudPlan.L) + 1, subs = setFrames / loudPlan.hop + 2;
    if (segs > loudSegCap || channels > loudSegChannels || subs > loudOutStride || channels > loudOutChannels) {
        HIP_OK(hipStreamSynchronize(stream));
        if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
        const size_t ch = std::max(channels, loudSegChannels), sg = std::max(segs, loudSegCap), sb = std::max(subs, loudOutStride);
        loudness::ChannelState* keep = dLoudState; const size_t keepCap = loudStateCap;
        dLoudState = nullptr;                               // (the programme's state outlives the scratch)
        loudnessFree();
        dLoudState = keep; loudStateCap = keepCap;
        HIP_OK(hipMalloc((void**)&dLoudSeg, ch * sg * 4 * sizeof(double)));
        HIP_OK(hipMalloc((void**)&dLoudEnergy, ch * sg * 2 * sizeof(double)));
        for (int k = 0; k < 2; ++k) {
            HIP_OK(hipMalloc((void**)&dLoudOut[k], ch * sb * sizeof(double)));
            HIP_OK(hipHostMalloc((void**)&hLoudOut[k], ch * sb * sizeof(double), hipHostMallocDefault));
        }
        loudSegCap = sg; loudSegChannels = loudOutChannels = ch; loudOutStride = sb;
    }
    return kOk;
}

int Engine::loudnessReset() {
    if (dry) return kNoDevice;
    RenderGuard lock(*this);
    if (!loudnessOn) return kInvalidPropertyValue;
    return loudnessResetLocked(0);
}

int Engine::loudnessRead(LoudnessInfo* info, double* meanSquares, size_t capacity, double* truePeak, float* samplePeak) {
    if (dry) return kNoDevice;
    RenderGuard lock(*this);
    if (!loudnessOn) return kInvalidPropertyValue;
    const size_t ch = loudChannels, n = ch ? loudSeries[0].size() : 0;
    if (info) { info->channels = (uint32_t)ch; info->hop = loudPlan.hop; info->subBlocks = n; info->frames = loudFrames; }
    if (meanSquares && capacity < ch * n) return kInvalidPropertyValue;
    if (meanSquares && n) for (size_t c = 0; c < ch; ++c) std::memcpy(meanSquares + c * n, loudSeries[c].data(), n * sizeof(double));
    if (ch && (truePeak || samplePeak)) {
        // (every metered call ends with both streams synchronised; a copy of the state: the programme may go on)
        if (hipSetDevice(device) != hipSuccess) return kHipError;
        std::vector<loudness::ChannelState> st(ch);
        HIP_OK(hipStreamSynchronize(stream));
        HIP_OK(hipMemcpy(st.data(), dLoudState, ch * sizeof(loudness::ChannelState), hipMemcpyDeviceToHost));
        for (size_t c = 0; c < ch; ++c) {
            if (truePeak) truePeak[c] = loudness::peak_with_tail(loudPlan, st[c]);
            if (samplePeak) std::memcpy(&samplePeak[c], &st[c].samplePeakBits, 4);
        }
    }
    return kOk;
}

} // namespace elemhip
