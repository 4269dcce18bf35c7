// engine_resample.cpp — the host side of the delivery-rate converter (option "resample_rate"; resample.h, resample.hip): the plan and
// the tables, the carried frames' and the converted halves' life, the programme's clock, the read-out and the reset. The set loop that
// launches the kernels is renderHostSets (engine_render.cpp).
#include "engine_impl.h"

namespace elemhip {

void Engine::resampleFree() {
    if (dResTable) (void)hipFree(dResTable);
    if (dResRowBase) (void)hipFree(dResRowBase);
    for (int k = 0; k < 2; ++k) { if (dResHist[k]) (void)hipFree(dResHist[k]); if (dRes[k]) (void)hipFree(dRes[k]); }
    dResTable = nullptr; dResRowBase = nullptr; dResHist[0] = dResHist[1] = dRes[0] = dRes[1] = nullptr;
    resHistChannels = 0; resFloats = 0; resHistCur = 0;
}

// (`mu` held.) 0 or the engine's own rate: off. A rate resample.h has no plan for is refused and changes nothing.
int Engine::setResampleRate(double hz) {
    const bool on = hz != 0.0 && hz != sampleRate, was = resampleOn;
    resample::Plan plan{};
    if (on && !resample::make_plan(sampleRate, hz, plan)) return kInvalidPropertyValue;
    if (limiterOn && limiterReplan(on ? hz : sampleRate, false) != kOk) return kInvalidPropertyValue;      // (no limiter plan at that rate: nothing changes)
    if (!dry) {
        if (hipSetDevice(device) != hipSuccess) return kHipError;
        HIP_OK(hipStreamSynchronize(stream));
        if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
        resampleFree();
    }
    resampleOn = on; resampleRate = on ? hz : 0.0; resPlan = plan;
    resChannels = 0; resFramesIn = resFramesOut = 0;
    resTable.clear(); resRowBase.clear();
    if (on) {
        resTable.resize((size_t)plan.T * plan.L); resRowBase.resize(plan.L);
        resample::make_tables(plan, resTable.data(), resRowBase.data());
        if (!dry) {
            HIP_OK(hipMalloc((void**)&dResTable, resTable.size() * sizeof(float)));
            HIP_OK(hipMalloc((void**)&dResRowBase, resRowBase.size() * sizeof(int32_t)));
            HIP_OK(hipMemcpy(dResTable, resTable.data(), resTable.size() * sizeof(float), hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(dResRowBase, resRowBase.data(), resRowBase.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        }
    }
    // the meter meters what is delivered: its plan follows the delivery rate, whichever option was set first
    if (loudnessOn && !dry && (on || was)) { loudness::make_plan(deliveryRate(), loudPlan); const int rc = loudnessResetLocked(0); if (rc != kOk) return rc; }
    // so does the limiter's: it limits what is delivered
    if (limiterOn && (on || was)) { const int rc = limiterReplan(deliveryRate(), true); if (rc != kOk) return rc; }
    return kOk;
}

// a new programme of `channels` channels (0: the count is set by the first call); `mu` held
int Engine::resampleResetLocked(size_t channels) {
    if (hipSetDevice(device) != hipSuccess) return kHipError;
    HIP_OK(hipStreamSynchronize(stream));
    if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
    if (channels > resHistChannels) {
        for (int k = 0; k < 2; ++k) { if (dResHist[k]) (void)hipFree(dResHist[k]); dResHist[k] = nullptr; }
        resHistChannels = 0;
        for (int k = 0; k < 2; ++k) HIP_OK(hipMalloc((void**)&dResHist[k], channels * resPlan.H * sizeof(float)));
        resHistChannels = channels;
    }
    for (int k = 0; k < 2 && channels; ++k) HIP_OK(hipMemset(dResHist[k], 0, channels * resPlan.H * sizeof(float)));
    resHistCur = 0;
    resChannels = (uint32_t)channels; resFramesIn = resFramesOut = 0;
    return kOk;
}

// the programme takes the channel count of its first call; the converted halves hold outBlocksCap blocks of every channel
int Engine::ensureResample(size_t channels, size_t outBlocksCap) {
    if (resChannels == 0) { const int rc = resampleResetLocked(channels); if (rc != kOk) return rc; }
    else if (channels != resChannels) return kInvalidPropertyValue;
    const size_t want = outBlocksCap * channels * (size_t)blockSize;
    if (want > resFloats) {
        HIP_OK(hipStreamSynchronize(stream));
        if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
        for (int k = 0; k < 2; ++k) { if (dRes[k]) (void)hipFree(dRes[k]); dRes[k] = nullptr; }
        resFloats = 0;
        for (int k = 0; k < 2; ++k) HIP_OK(hipMalloc((void**)&dRes[k], want * sizeof(float)));
        resFloats = want;
    }
    return kOk;
}

int Engine::resampleFrames(size_t numFrames, size_t* out) {
    if (!out) return kInvalidInstructionFormat;
    RenderGuard lock(*this);
    *out = resampleOn ? (size_t)(resample::outputs_before(resPlan, resFramesIn + numFrames) - resample::outputs_before(resPlan, resFramesIn)) : numFrames;
    return kOk;
}

int Engine::resampleRead(ResampleInfo* info) {
    RenderGuard lock(*this);
    if (!resampleOn) return kInvalidPropertyValue;
    if (info) *info = ResampleInfo{resPlan.L, resPlan.M, resPlan.T, resPlan.Do, resFramesIn, resFramesOut};
    return kOk;
}

int Engine::resampleReset() {
    RenderGuard lock(*this);
    if (!resampleOn) return kInvalidPropertyValue;
    if (dry) { resChannels = 0; resFramesIn = resFramesOut = 0; return kOk; }
    return resampleResetLocked(0);
}

} // namespace elemhip
