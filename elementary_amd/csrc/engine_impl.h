// engine_impl.h — what more than one of the engine's translation units needs (engine.cpp, engine_nodes.cpp, engine_relay.cpp,
// engine_render.cpp, engine_host_blocks.cpp) and no one else does: included by those files only.
#pragma once
#include "engine.h"

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "launch.h"
#include "resource_load.h"

namespace elemhip {

// ELEMHIP_DEBUG_SYNC=1 (fault hunting on the GPU box): every launch is followed by a device synchronise and a line on stderr, so
// the last line printed before a "Memory access fault" abort names the kernel that faulted.
static bool debugSyncOn() { static const bool on = std::getenv("ELEMHIP_DEBUG_SYNC") != nullptr; return on; }
static void debugSync(const char* what, unsigned a = 0, unsigned b = 0) {
    if (!debugSyncOn()) return;
    std::fprintf(stderr, "[elemhip sync] %s %u %u ...", what, a, b); std::fflush(stderr);
    const hipError_t e = hipDeviceSynchronize();
    std::fprintf(stderr, " %s\n", e == hipSuccess ? "ok" : hipGetErrorString(e)); std::fflush(stderr);
}

#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    std::fprintf(stderr, "[elemhip] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); return kHipError; } } while (0)
#define HIP_WARN(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    std::fprintf(stderr, "[elemhip] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } } while (0)

// Every entry point that takes the render lock — except the per-block process() calls themselves — first asks a resident kernel
// (option "resident") to leave: it owns the engine's stream for as long as it lives.
struct RenderGuard {
    std::lock_guard<std::mutex> l;
    explicit RenderGuard(Engine& e) : l(e.mu) { e.residentStop(); }
};

static inline uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static int bitceil(int n) {   // builtins/helpers/BitUtils.h:9-20
    if ((n & (n - 1)) == 0) return n;
    int o = 1;
    while (o < n) o <<= 1;
    return o;
}

static inline float clampf(float v, float lo, float hi) { return (v < lo) ? lo : ((hi < v) ? hi : v); }

static double msToStep(double sr, double ms) {   // helpers/GainFade.h:10-12
    return ms > 1e-6 ? 1.0 / (sr * ms / 1000.0) : 1.0;
}

// `size` of a scope / fft node: the property, or the reference's default (Analyzers.h:142-149: 512; wasm/FFT.h:18-25: 1024) —
// createNode sets the same default, the relay and eventWindowBlocks read it back
inline double analyzerDefaultSize(uint16_t op) { return op == OP_FFT ? 1024.0 : 512.0; }
inline double analyzerSize(const Node& n) {
    auto q = n.props.find("size");
    return (q != n.props.end() && q->second.isNumber()) ? q->second.num : analyzerDefaultSize(n.op);
}

} // namespace elemhip
