// engine_resample_in.cpp — the host side of the input-rate converter (option "input_rate"; resample.h, resample_in.hip): the plan and
// the tables, the carried frames' life, the input programme's clock, the read-out and the reset. The set loop that launches the
// kernels is renderHostSets (engine_render.cpp).
#include "engine_impl.h"

namespace elemhip {

void Engine::inputResampleFree() {
    if (dInTable) (void)hipFree(dInTable);
    if (dInRowBase) (void)hipFree(dInRowBase);
    for (int k = 0; k < 2; ++k) if (dInHist[k]) (void)hipFree(dInHist[k]);
    dInTable = nullptr; dInRowBase = nullptr; dInHist[0] = dInHist[1] = nullptr;
    inHistChannels = 0; inHistCur = 0;
}

// (`mu` held.) 0 or the engine's own rate: off. A rate resample.h has no input-side plan for is refused and changes nothing.
int Engine::setInputRate(double hz) {
    const bool on = hz != 0.0 && hz != sampleRate;
    resample::Plan plan{};
    if (on && !resample::make_plan_in(hz, sampleRate, plan)) return kInvalidPropertyValue;
    if (!dry) {
        if (hipSetDevice(device) != hipSuccess) return kHipError;
        HIP_OK(hipStreamSynchronize(stream));
        if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
        inputResampleFree();
    }
    inResOn = on; inResRate = on ? hz : 0.0; inPlan = plan;
    inChannels = 0; inFramesIn = inFramesOut = 0;
    inTable.clear(); inRowBase.clear();
    if (on) {
        inTable.resize((size_t)plan.T * plan.L); inRowBase.resize(plan.L);
        resample::make_tables(plan, inTable.data(), inRowBase.data());
        if (!dry) {
            HIP_OK(hipMalloc((void**)&dInTable, inTable.size() * sizeof(float)));
            HIP_OK(hipMalloc((void**)&dInRowBase, inRowBase.size() * sizeof(int32_t)));
            HIP_OK(hipMemcpy(dInTable, inTable.data(), inTable.size() * sizeof(float), hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(dInRowBase, inRowBase.data(), inRowBase.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        }
    }
    return kOk;
}

// a new programme of `channels` channels (0: the count is set by the first call); `mu` held
int Engine::inputResampleResetLocked(size_t channels) {
    if (hipSetDevice(device) != hipSuccess) return kHipError;
    HIP_OK(hipStreamSynchronize(stream));
    if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
    if (channels > inHistChannels) {
        for (int k = 0; k < 2; ++k) { if (dInHist[k]) (void)hipFree(dInHist[k]); dInHist[k] = nullptr; }
        inHistChannels = 0;
        for (int k = 0; k < 2; ++k) HIP_OK(hipMalloc((void**)&dInHist[k], channels * inPlan.H * sizeof(float)));
        inHistChannels = channels;
    }
    for (int k = 0; k < 2 && channels; ++k) HIP_OK(hipMemset(dInHist[k], 0, channels * inPlan.H * sizeof(float)));
    inHistCur = 0;
    inChannels = (uint32_t)channels; inFramesIn = inFramesOut = 0;
    return kOk;
}

// the programme takes the channel count of its first call
int Engine::ensureInputResample(size_t channels) {
    if (inChannels == 0) return inputResampleResetLocked(channels);
    return channels == inChannels ? kOk : kInvalidPropertyValue;
}

int Engine::inputResampleFrames(size_t numFrames, size_t* out) {
    if (!out) return kInvalidInstructionFormat;
    RenderGuard lock(*this);
    *out = inResOn ? (size_t)(resample::inputs_before(inPlan, inFramesOut + numFrames) - inFramesIn) : numFrames;
    return kOk;
}

int Engine::inputResampleRead(ResampleInfo* info) {
    RenderGuard lock(*this);
    if (!inResOn) return kInvalidPropertyValue;
    if (info) *info = ResampleInfo{inPlan.L, inPlan.M, inPlan.T, inPlan.Do, inFramesIn, inFramesOut};
    return kOk;
}

int Engine::inputResampleReset() {
    RenderGuard lock(*this);
    if (!inResOn) return kInvalidPropertyValue;
    if (dry) { inChannels = 0; inFramesIn = inFramesOut = 0; return kOk; }
    return inputResampleResetLocked(0);
}

} // namespace elemhip
