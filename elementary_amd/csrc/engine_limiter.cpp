// engine_limiter.cpp — the host side of the true-peak limiter (options "limiter", "limiter_*"; limiter.h, limiter.hip): the plan, the
// carried state's, the scratch's and the limited halves' life, the programme's clock, the read-out and the reset. The set loop that
// launches the kernels is renderHostSets (engine_render.cpp).
#include "engine_impl.h"

namespace elemhip {

void Engine::limiterFree() {
    for (int k = 0; k < 2; ++k) { if (dLimState[k]) (void)hipFree(dLimState[k]); if (dLim[k]) (void)hipFree(dLim[k]); }
    if (dLimStats) (void)hipFree(dLimStats);
    if (dLimFrames) (void)hipFree(dLimFrames);
    if (dLimTiles) (void)hipFree(dLimTiles);
    dLimState[0] = dLimState[1] = nullptr; dLim[0] = dLim[1] = nullptr; dLimStats = nullptr; dLimFrames = dLimTiles = nullptr;
    limStateCap = limStatsCap = limFrameCap = limTileCap = limScratchGroups = limFloats = 0; limCur = 0;
}

// the plan at `rate` from the current parameters; `apply`: adopt it and start a new programme, else only say whether there is one
int Engine::limiterReplan(double rate, bool apply) {
    limiter::Plan plan{};
    if (!limiter::make_plan(rate, limCeilingDb, limGainDb, limLookaheadMs, limReleaseMs, limLink, plan)) return kInvalidPropertyValue;
    if (!apply) return kOk;
    limPlan = plan;
    loudness::make_plan(rate, limMeter);
    if (dry) { limChannels = 0; limFrames = 0; return kOk; }
    return limiterResetLocked(0);
}

// (`mu` held.) A value outside its range, or one that leaves no plan at the delivery rate (1 <= D <= 1024, R >= 1), is refused and
// changes nothing — while the limiter is off as well, so that turning it on cannot fail on a parameter.
int Engine::setLimiterOption(const std::string& key, double value) {
    double* slot = key == "limiter_ceiling_dbtp" ? &limCeilingDb : key == "limiter_gain_db" ? &limGainDb : key == "limiter_lookahead_ms" ? &limLookaheadMs
                 : key == "limiter_release_ms" ? &limReleaseMs : key == "limiter_link" ? &limLink : nullptr;
    if (slot) {
        const double old = *slot;
        *slot = value;
        const int rc = limiterReplan(deliveryRate(), limiterOn);
        if (rc == kInvalidPropertyValue) *slot = old;
        return rc;
    }
    if (key != "limiter") return kInvalidPropertyValue;
    if (value != 0.0 && value != 1.0) return kInvalidPropertyValue;
    if (value != 0.0) {
        const int rc = limiterReplan(deliveryRate(), true);
        if (rc != kOk) return rc;
        limiterOn = true;
        return kOk;
    }
    if (limiterOn && !dry) {
        if (hipSetDevice(device) != hipSuccess) return kHipError;
        HIP_OK(hipStreamSynchronize(stream));
        if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
        limiterFree();
    }
    limiterOn = false; limChannels = 0; limFrames = 0;
    return kOk;
}

// a new programme of `channels` channels (0: the count is set by the first call); `mu` held
int Engine::limiterResetLocked(size_t channels) {
    if (hipSetDevice(device) != hipSuccess) return kHipError;
    HIP_OK(hipStreamSynchronize(stream));
    if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
    if (channels) {
        const size_t bytes = limiter::state_bytes(limPlan, (uint32_t)channels), groups = limiter::group_count(limPlan, (uint32_t)channels);
        if (bytes > limStateCap) {
            for (int k = 0; k < 2; ++k) { if (dLimState[k]) (void)hipFree(dLimState[k]); dLimState[k] = nullptr; }
            limStateCap = 0;
            for (int k = 0; k < 2; ++k) HIP_OK(hipMalloc((void**)&dLimState[k], bytes));
            limStateCap = bytes;
        }
        if (groups > limStatsCap) {
            if (dLimStats) (void)hipFree(dLimStats);
            dLimStats = nullptr; limStatsCap = 0;
            HIP_OK(hipMalloc((void**)&dLimStats, groups * sizeof(limiter::GroupStats)));
            limStatsCap = groups;
        }
        std::vector<unsigned char> fresh(bytes);
        limiter::state_reset(limPlan, (uint32_t)channels, fresh.data());
        for (int k = 0; k < 2; ++k) HIP_OK(hipMemcpy(dLimState[k], fresh.data(), bytes, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(dLimStats, 0, groups * sizeof(limiter::GroupStats)));
    }
    limCur = 0;
    limChannels = (uint32_t)channels; limFrames = 0;
    return kOk;
}

// the programme takes the channel count of its first call; the limited halves hold outBlocksCap blocks of every channel, the scratch
// setFrames frames of every group
int Engine::ensureLimiter(size_t channels, size_t outBlocksCap, size_t setFrames) {
    if (limChannels == 0) {
        if (!limiter::channels_ok(limPlan, (uint32_t)channels)) return kInvalidPropertyValue;
        const int rc = limiterResetLocked(channels);
        if (rc != kOk) return rc;
    } else if (channels != limChannels) return kInvalidPropertyValue;
    const size_t want = outBlocksCap * channels * (size_t)blockSize, groups = limiter::group_count(limPlan, (uint32_t)channels);
    const size_t tiles = limiter::tile_count((uint32_t)setFrames);
    if (want > limFloats || setFrames > limFrameCap || tiles > limTileCap || groups > limScratchGroups) {
        HIP_OK(hipStreamSynchronize(stream));
        if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
    }
    if (want > limFloats) {
        for (int k = 0; k < 2; ++k) { if (dLim[k]) (void)hipFree(dLim[k]); dLim[k] = nullptr; }
        limFloats = 0;
        for (int k = 0; k < 2; ++k) HIP_OK(hipMalloc((void**)&dLim[k], want * sizeof(float)));
        limFloats = want;
    }
    if (setFrames > limFrameCap || tiles > limTileCap || groups > limScratchGroups) {
        const size_t fc = std::max(setFrames, limFrameCap), tc = std::max(tiles, limTileCap), gc = std::max(groups, limScratchGroups);
        if (dLimFrames) (void)hipFree(dLimFrames);
        if (dLimTiles) (void)hipFree(dLimTiles);
        dLimFrames = dLimTiles = nullptr; limFrameCap = limTileCap = limScratchGroups = 0;
        HIP_OK(hipMalloc((void**)&dLimFrames, gc * fc * sizeof(double)));
        HIP_OK(hipMalloc((void**)&dLimTiles, gc * tc * sizeof(double)));
        limFrameCap = fc; limTileCap = tc; limScratchGroups = gc;
    }
    return kOk;
}

int Engine::limiterRead(LimiterInfo* info, double* maxReduction, uint64_t* limitedFrames, size_t capacity) {
    RenderGuard lock(*this);
    if (!limiterOn) return kInvalidPropertyValue;
    const uint32_t groups = limChannels ? limiter::group_count(limPlan, limChannels) : 0u;
    if (info) *info = LimiterInfo{limPlan.D, limiter::latency(limPlan), limPlan.R, limPlan.link, groups, limFrames};
    if (!groups || (!maxReduction && !limitedFrames)) return kOk;
    if (capacity < groups) return kInvalidPropertyValue;
    if (dry) return kNoDevice;
    // (every limited call ends with both streams synchronised)
    if (hipSetDevice(device) != hipSuccess) return kHipError;
    std::vector<limiter::GroupStats> st(groups);
    HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(hipMemcpy(st.data(), dLimStats, groups * sizeof(limiter::GroupStats), hipMemcpyDeviceToHost));
    for (uint32_t g = 0; g < groups; ++g) {
        if (maxReduction) maxReduction[g] = loudness::bits_double(st[g].maxBits);
        if (limitedFrames) limitedFrames[g] = st[g].limited;
    }
    return kOk;
}

int Engine::limiterReset() {
    RenderGuard lock(*this);
    if (!limiterOn) return kInvalidPropertyValue;
    if (dry) { limChannels = 0; limFrames = 0; return kOk; }
    return limiterResetLocked(0);
}

} // namespace elemhip
