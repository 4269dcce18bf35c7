// capture_replay.h — the events of a `capture` / `mc.capture` node (builtins/Capture.h:60-95, builtins/mc/Capture.h:103-146) as a relay
// after EVERY block (offline-renderer/index.ts:112-120) would have emitted them, replayed on the host after a launch set.
//
// Under such a relay processEvents drains everything in the node's ring into the relay buffer and, if a falling gate edge was seen
// since the previous relay, emits ONE event with the whole relay buffer and clears it; the ring of bitceil(sr) frames never overruns,
// a block being far smaller. So two facts per block b describe a run: F_b, the absolute count of frames handed to the ring by the
// end of block b (frames still in the mono node's 128-frame scratch belong to a later take), and E_b, whether the gate fell inside
// block b. An event follows every block with E_b set and carries the frames [F_prev, F_b), F_prev the F of the previous emission —
// a fall and a new rise inside one block included: what was flushed after the edge rides along, as in the reference. The kernels log
// {block, F_b mod 2^32, E_b, 0} per engine block (device.h CAP_LOGMASK); unlike a scope's reads (event_replay.h) none of this follows
// from positions alone, the gate's samples decide.
//
// Plain C++, no HIP: the relay (engine_relay.cpp) and tests/native/capture_replay_host.cpp compile the same text.
#pragma once
#include <stdint.h>

#include <vector>

#include "event_fold.h"

namespace cpr {

struct Entry { uint64_t block; uint32_t end; bool fell; };   // one HOST block of the window: F (mod 2^32) at its end, E
struct Take { uint64_t block; uint64_t end; };               // an event after host block `block` that carries the frames up to `end`

// the absolute count a device counter `f` (mod 2^32) stands for, given one it cannot be before (a window brings far fewer than 2^31
// frames); a counter that reads as earlier — logged before a plain relay drained past it — is `from`
inline uint64_t unwrap(uint64_t from, uint32_t f) {
    const uint32_t d = f - (uint32_t)from;
    return (int32_t)d < 0 ? from : from + d;
}

// `e`: the newest `take` entries of the node's per-block log, oldest first, 4 dwords each (block, F, E, -); entry k was written by the
// engine block take - 1 - k blocks before the newest. One entry per HOST block: its last slice's F, the OR of its slices' E.
inline std::vector<Entry> fold(const evf::Window& w, const uint32_t* e, uint32_t take) {
    std::vector<Entry> out;
    for (uint32_t k = 0; k < take; ++k) {
        const uint64_t b = w.block_of(take - 1 - k);
        const bool fell = e[4 * k + 2] != 0u;
        if (!out.empty() && out.back().block == b) { out.back().end = e[4 * k + 1]; out.back().fell = out.back().fell || fell; }
        else out.push_back({b, e[4 * k + 1], fell});
    }
    return out;
}

// The window's host blocks in order from `relayed`, the absolute count of frames drained so far; `pending`: the node carried a set
// ready flag into the window (the relay after its first block finds it). Appends the window's takes; returns the count drained by
// the window's end — frames behind the last take stay in the relay buffer for the next window.
inline uint64_t replay(const Entry* e, size_t n, uint64_t relayed, bool pending, std::vector<Take>& takes) {
    for (size_t k = 0; k < n; ++k) {
        relayed = unwrap(relayed, e[k].end);
        if (e[k].fell || (pending && k == 0)) takes.push_back({e[k].block, relayed});
    }
    return relayed;
}

} // namespace cpr
