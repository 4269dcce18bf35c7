// engine_automation.cpp — the host side of breakpoint automation (elemhip_automation_set; automation.h, automation.hip): the lanes'
// tables on both sides, the read-out and the reset. The set loop that launches the kernel is renderHostSets (engine_render.cpp); the
// host-block renderer fills the lane channels with the header's scalar twin.
#include "engine_impl.h"

namespace elemhip {

Engine::AutoLanes::~AutoLanes() {
    if (dev) (void)hipFree(dev);       // (every call that read the table held this set and has returned: hipFree waits for the device besides)
}

// the set with lane `channel` replaced by `count` points (0: removed), uploaded; null where no lane is left
int Engine::automationSet(uint32_t channel, const automation::Point* points, size_t count) {
    namespace au = automation;
    if (channel >= au::kMaxChannels) return kInvalidPropertyValue;
    if (count != 0 && !au::lane_ok(points, count)) return kInvalidPropertyValue;
    RenderGuard lock(*this);
    const std::shared_ptr<const AutoLanes> old = std::atomic_load(&autoLanes);
    if (count == 0 && (!old || old->count[channel] == 0u)) return kOk;
    auto next = std::make_shared<AutoLanes>();
    for (uint32_t c = 0; c < au::kMaxChannels; ++c) {
        const au::Point* from = c == channel ? points : old ? old->points.data() + old->offset[c] : nullptr;
        const size_t n = c == channel ? count : old ? old->count[c] : 0;
        next->offset[c] = (uint32_t)next->points.size(); next->count[c] = (uint32_t)n;
        if (n == 0) continue;
        if (next->points.size() + n > 0xFFFFFFFFull) return kInvalidPropertyValue;
        next->points.insert(next->points.end(), from, from + n);
        if (next->inputs == 0u) next->lowest = c;
        next->inputs = c + 1u;
    }
    if (next->inputs == 0u) { std::atomic_store(&autoLanes, std::shared_ptr<const AutoLanes>()); return kOk; }
    if (!dry) {
        if (hipSetDevice(device) != hipSuccess) return kHipError;
        HIP_OK(hipMalloc((void**)&next->dev, next->points.size() * sizeof(au::Point)));
        HIP_OK(hipMemcpy(next->dev, next->points.data(), next->points.size() * sizeof(au::Point), hipMemcpyHostToDevice));
    }
    std::atomic_store(&autoLanes, std::shared_ptr<const AutoLanes>(std::move(next)));
    return kOk;
}

int Engine::automationRead(uint32_t channel, AutomationInfo* info, automation::Point* points, size_t capacity) {
    if (channel >= automation::kMaxChannels) return kInvalidPropertyValue;
    const std::shared_ptr<const AutoLanes> lanes = std::atomic_load(&autoLanes);
    AutomationInfo ai{0u, 0u, 0u};
    if (lanes) {
        for (uint32_t c = 0; c < automation::kMaxChannels; ++c) if (lanes->count[c]) ai.lanes |= 1u << c;
        ai.inputs = lanes->inputs; ai.count = lanes->count[channel];
    }
    if (info) *info = ai;
    if (points && capacity < ai.count) return kInvalidPropertyValue;
    if (points && ai.count) std::memcpy(points, lanes->points.data() + lanes->offset[channel], ai.count * sizeof(automation::Point));
    return kOk;
}

int Engine::automationReset() {
    RenderGuard lock(*this);
    std::atomic_store(&autoLanes, std::shared_ptr<const AutoLanes>());
    return kOk;
}

} // namespace elemhip
