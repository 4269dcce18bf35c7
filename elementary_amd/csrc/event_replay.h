// event_replay.h — the reference's analyzer ring (runtime/elem/MultiChannelRingBuffer.h:34-83) as the state machine it is, replayed
// on the host after a launch set: where a relay after EVERY block (offline-renderer/index.ts:112-120) would have read a `scope`
// or `fft` node's ring, and which frames each read would have handed on.
//
// The reference's ring holds 8192 frames. Its write (:34-59) moves the write position by the block and, when the block does not
// fit (`numSamples >= numFreeSlots`), nudges the read position to write + 1; its read (:61-86, behind `size() > size` for a scope,
// Analyzers.h:192-245, and `size() >= size` for an fft, wasm/FFT.h:96) hands on `size` frames at the read position and moves it.
// None of that depends on the samples: given the positions when a window of blocks begins, the block length, `size` and the
// comparison, every read of the window is known. The ring never holds more than 8191 frames, so the slots [read, read + size) of a
// permitted read are the CONTIGUOUS frames [written - full, written - full + size) of the node's input, `written` = frames written
// so far: an emitted frame is named by the absolute index of its first sample, and a device ring that keeps the last
// `window + 8191` frames (device.h SCP_MASK) has every one of them, overruns included.
//
// Plain C++, no HIP: the relay (engine_relay.cpp) and tests/native/event_replay_host.cpp compile the same text. Its neighbour
// event_fold.h holds the relay's other host-only decisions (host blocks of a sliced window, meter / snapshot folds, scope runs).
#pragma once
#include <stdint.h>

namespace evr {

constexpr uint32_t kRefRing = 8192;               // MultiChannelRingBuffer.h:17
constexpr uint32_t kRefMask = kRefRing - 1u;

// A node's ring as the reference would hold it: frames written so far, and the read position (mod 8192). The write position is
// `written & kRefMask`. A new node starts at {0, 0}.
struct Pos { uint64_t written = 0; uint32_t read = 0; };

enum Cmp : uint32_t { kMoreThan = 0, kAtLeast = 1 };   // scope: size() > size; fft: size() >= size

inline uint32_t full_slots(const Pos& p) {        // :99-110
    const uint32_t w = (uint32_t)(p.written & kRefMask), r = p.read;
    return w > r ? w - r : ((kRefRing - (r - w)) & kRefMask);
}
inline void write_block(Pos& p, uint32_t frames) {   // :34-59
    const uint32_t w = (uint32_t)(p.written & kRefMask), r = p.read;
    const uint32_t freeSlots = r > w ? r - w : kRefRing - (w - r);
    p.written += frames;
    if (frames >= freeSlots) p.read = ((uint32_t)(p.written & kRefMask) + 1u) & kRefMask;
}
// one read attempt; true: `first` = absolute index of the frame's first sample
inline bool read_frame(Pos& p, uint32_t size, Cmp cmp, uint64_t& first) {
    const uint32_t full = full_slots(p);
    if (!(cmp == kAtLeast ? full >= size : full > size)) return false;
    first = p.written - full;
    p.read = (p.read + size) & kRefMask;
    return true;
}

// `blocks` blocks of `block` frames from `p`, a read attempt after each: emit(block index in the window, first frame) per read that
// succeeds; returns the positions at the end of the window — the next window's start.
template <class Emit>
inline Pos replay(Pos p, uint32_t block, uint32_t size, Cmp cmp, uint32_t blocks, Emit&& emit) {
    for (uint32_t b = 0; b < blocks; ++b) {
        write_block(p, block);
        uint64_t first;
        if (read_frame(p, size, cmp, first)) emit(b, first);
    }
    return p;
}

} // namespace evr
