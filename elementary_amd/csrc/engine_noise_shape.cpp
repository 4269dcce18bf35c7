// engine_noise_shape.cpp — the host side of noise-shaped requantisation (elemhip_noise_shape_set; noise_shape.h, noise_shape.hip): the
// coefficients, the carried states' and the code buffer's life, the programme's clock, the read-out and the reset. The set loop that
// launches the kernel is renderHostSets (engine_render.cpp); the host-block renderer runs the header's scalar loop on the same states.
#include "engine_impl.h"

namespace elemhip {

void Engine::noiseShapeFree() {
    if (dNsState) (void)hipFree(dNsState);
    if (dNsCodes) (void)hipFree(dNsCodes);
    dNsState = nullptr; dNsCodes = nullptr; nsStateCap = nsCodesCap = 0;
    nsChannels = 0; nsFrames = 0;
}

// a new programme: its channel count is set by the next call; `mu` held
int Engine::noiseShapeResetLocked() {
    nsChannels = 0; nsFrames = 0;
    if (dry || !dNsState) return kOk;
    if (hipSetDevice(device) != hipSuccess) return kHipError;
    HIP_OK(hipStreamSynchronize(stream));
    if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
    return kOk;
}

int Engine::noiseShapeSet(const float* coeffs, uint32_t count) {
    RenderGuard lock(*this);
    int32_t cq[noise_shape::kMaxTaps] = {};
    if (count && !noise_shape::quantise_coeffs(coeffs, count, cq)) return kInvalidPropertyValue;
    if (count == 0u) {
        if (nsTaps && !dry) {
            if (hipSetDevice(device) != hipSuccess) return kHipError;
            HIP_OK(hipStreamSynchronize(stream));
            if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
            noiseShapeFree();
        }
        nsTaps = 0; nsChannels = 0; nsFrames = 0;
        std::memset(nsCq, 0, sizeof nsCq);
        return kOk;
    }
    const int rc = noiseShapeResetLocked();
    if (rc != kOk) return rc;
    nsTaps = count;
    std::memcpy(nsCq, cq, sizeof nsCq);
    return kOk;
}

// the programme takes the channel count of the call: another count than the open programme's starts a new one (states zero)
int Engine::ensureNoiseShape(size_t channels, size_t codes) {
    if (channels > nsStateCap || codes > nsCodesCap) {
        HIP_OK(hipStreamSynchronize(stream));
        if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
    }
    if (channels > nsStateCap) {
        if (dNsState) (void)hipFree(dNsState);
        dNsState = nullptr; nsStateCap = 0; nsChannels = 0; nsFrames = 0;
        HIP_OK(hipMalloc((void**)&dNsState, channels * sizeof(noise_shape::ChannelState)));
        nsStateCap = channels;
    }
    if (codes > nsCodesCap) {
        if (dNsCodes) (void)hipFree(dNsCodes);
        dNsCodes = nullptr; nsCodesCap = 0;
        HIP_OK(hipMalloc((void**)&dNsCodes, codes * sizeof(int32_t)));
        nsCodesCap = codes;
    }
    if (channels != nsChannels) {
        HIP_OK(hipStreamSynchronize(stream));
        HIP_OK(hipMemset(dNsState, 0, channels * sizeof(noise_shape::ChannelState)));
        nsChannels = (uint32_t)channels; nsFrames = 0;
    }
    return kOk;
}

int Engine::noiseShapeRead(NoiseShapeInfo* info, int32_t* cq, uint64_t* saturated, size_t capacity) {
    RenderGuard lock(*this);
    if (info) *info = NoiseShapeInfo{nsTaps, nsTaps ? nsChannels : 0u, nsTaps ? nsFrames : 0u};
    if (!nsTaps) return kOk;
    if (cq) { if (capacity < nsTaps) return kInvalidPropertyValue; std::memcpy(cq, nsCq, nsTaps * sizeof(int32_t)); }
    if (!saturated || !nsChannels) return kOk;
    if (capacity < nsChannels) return kInvalidPropertyValue;
    if (dry) return kNoDevice;
    // (every shaped call ends with both streams synchronised)
    if (hipSetDevice(device) != hipSuccess) return kHipError;
    std::vector<noise_shape::ChannelState> st(nsChannels);
    HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(hipMemcpy(st.data(), dNsState, nsChannels * sizeof(noise_shape::ChannelState), hipMemcpyDeviceToHost));
    for (uint32_t c = 0; c < nsChannels; ++c) saturated[c] = st[c].saturated;
    return kOk;
}

int Engine::noiseShapeAfter(int rc) {
    if (rc == kOk) return rc;
    RenderGuard lock(*this);
    if (nsTaps) (void)noiseShapeResetLocked();
    return rc;
}

int Engine::noiseShapeReset() {
    RenderGuard lock(*this);
    return noiseShapeResetLocked();
}

} // namespace elemhip
