// event_fold.h — the event relay's decisions that touch neither HIP nor the engine (engine_relay.cpp, processQueuedEvents): which
// HOST block of a relay window an engine block belongs to, how the per-block readout logs of a meter / snapshot node fold into the
// readouts the reference would have queued per host block, which stretches of a scope's ring one relay fetches, and how much a
// capture ring holds.
//
// Plain C++, no HIP, like its neighbour event_replay.h: engine_relay.cpp and tests/native/event_fold_host.cpp compile the same text.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace evf {

// The reference's readout queue (SingleWriterSingleReaderQueue.h, capacity 32) cannot tell "32 x k pushes since the last relay"
// from "none": its write position is back on the read position, size() answers 0 and processEvents reports nothing — a meter
// polled every 32nd block, a snapshot that latches exactly 32 times per block (a 3 kHz train at 48 kHz and 512 frames). Kept.
inline bool wraps_to_empty(uint32_t pushes) { return pushes != 0u && (pushes & 31u) == 0u; }

// One relay window: `windowBlocks` engine blocks rendered since the last relay. A host block longer than the engine's renders as k
// slices, each an engine block with readouts of its own; the reference's nodes see ONE block (a meter reports min / max over all its
// frames, Analyzers.h:38-39; the relay runs once per host block): `hostEnds[h]` = slices of the window rendered when host block h
// ended (ascending; the last host block may be cut by the window's end). Unsliced, a host block is an engine block.
struct Window {
    bool sliced = false;
    uint64_t windowBlocks = 0;
    std::vector<uint64_t> hostEnds;
    uint64_t hostBlocks() const { return sliced ? (uint64_t)hostEnds.size() : windowBlocks; }      // host blocks in the window
    uint64_t lastBlock() const { const uint64_t h = hostBlocks(); return h ? h - 1 : 0; }
    // the HOST block (of this relay window) an engine block `fromEnd` blocks before the newest belongs to
    uint64_t block_of(uint64_t fromEnd) const {
        const uint64_t lastSlice = windowBlocks ? windowBlocks - 1 : 0;
        const uint64_t s = fromEnd > lastSlice ? 0 : lastSlice - fromEnd;
        return sliced ? (uint64_t)(std::upper_bound(hostEnds.begin(), hostEnds.end(), s) - hostEnds.begin()) : s;
    }
};

inline float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// ---- meter (Analyzers.h:23-62). `e`: the newest `take` entries of the node's readout log, oldest first, 4 dwords each
// (-, min, max, -); entry k was written by the engine block take - 1 - k blocks before the newest. One readout per HOST block: the
// slices of a host block folded into one min / max (unsliced: every group is one entry). A blockwise relay hands on every group;
// the plain relay the newest alone, unless the reference's queue of one readout per host block had wrapped to empty. ----
struct MeterOut { uint64_t block; float mn, mx; };
inline std::vector<MeterOut> fold_meter(const Window& w, const uint32_t* e, uint32_t take, bool blockwise) {
    std::vector<MeterOut> groups;
    for (uint32_t k = 0; k < take; ++k) {
        const float mn = as_float(e[4 * k + 1]), mx = as_float(e[4 * k + 2]);
        const uint64_t b = w.block_of(take - 1 - k);
        if (!groups.empty() && groups.back().block == b) { MeterOut& g = groups.back(); if (mn < g.mn) g.mn = mn; if (mx > g.mx) g.mx = mx; }
        else groups.push_back({b, mn, mx});
    }
    if (blockwise) return groups;
    if (groups.empty() || wraps_to_empty((uint32_t)groups.size())) return {};      // (the reference queued one readout per host block)
    return {groups.back()};
}

// ---- snapshot (Analyzers.h:83-131), blockwise. `e`: the newest `take` log entries, oldest first, 4 dwords each (engine block
// counter when it latched, value, pushes, -); `blk` = the node's block counter now. The log entries of one HOST block: its newest
// latch, its pushes summed — and the wrap rule on the pushes of that block alone, as a per-block relay would have met them. ----
struct SnapshotOut { uint64_t block; float value; };
inline std::vector<SnapshotOut> fold_snapshot(const Window& w, const uint32_t* e, uint32_t take, uint32_t blk) {
    std::vector<SnapshotOut> out;
    for (uint32_t k = 0; k < take;) {
        const uint64_t b = w.block_of((uint64_t)(blk - 1u - e[4 * k]));
        uint32_t pushes = 0, last = k;
        for (; k < take && w.block_of((uint64_t)(blk - 1u - e[4 * k])) == b; ++k) { pushes += e[4 * k + 2]; last = k; }
        if (wraps_to_empty(pushes)) continue;
        out.push_back({b, as_float(e[4 * last + 1])});
    }
    return out;
}

// ---- scope (Analyzers.h:192-245): the frames one relay hands on, as runs of absolute frame indices to fetch. Consecutive emits are
// contiguous until an overrun skips frames; a gap shorter than a copy is worth (kGap frames = 16 KB per channel) is fetched along
// rather than split off. add() per emitted frame in order, layout() once, then offset(emit) = where its `size` frames begin in a
// buffer of `span` frames per channel that holds the runs back to back. ----
struct ScopeRuns {
    static constexpr uint64_t kGap = 4096;
    struct Run { uint64_t first, frames; size_t at; };
    struct Emit { uint64_t block, first; size_t run; };
    std::vector<Run> runs;
    std::vector<Emit> emits;
    size_t span = 0;
    void add(uint64_t block, uint64_t first, uint64_t size) {
        if (runs.empty() || first < runs.back().first || first > runs.back().first + runs.back().frames + kGap) runs.push_back({first, 0, 0});
        Run& run = runs.back();
        run.frames = std::max<uint64_t>(run.frames, first + size - run.first);
        emits.push_back({block, first, runs.size() - 1});
    }
    void layout() { span = 0; for (Run& run : runs) { run.at = span; span += (size_t)run.frames; } }
    size_t offset(const Emit& e) const { return runs[e.run].at + (size_t)(e.first - runs[e.run].first); }
};

// ---- capture (Capture.h:60-95): entries between the read and the write position of a ring of mask + 1 entries ----
inline uint32_t capture_avail(uint32_t w, uint32_t r, uint32_t mask) { return w > r ? w - r : (((mask + 1u) - (r - w)) & mask); }

} // namespace evf
