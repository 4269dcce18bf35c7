// flac_in_md5.h — the STREAMINFO MD5 of FLAC inputs and resources (option "flac_in_md5"; flac_in_md5.hip, engine_flac_in.cpp,
// engine_resource_load.cpp): RFC 1321 over the decoded samples as libFLAC hashes them (RFC 9639 §8.2) — for stream sample t, then
// channel g, the low B = (bits + 7) / 8 bytes of the two's-complement code, little-endian: B = 1 at 8 bits, 2 at 12 / 16, 3 at 20 / 24,
// the 12- and 20-bit codes sign-extended into their top byte (the int32 codes the decoder leaves are). The Record, the rounds and the
// chunk schedule are flac_md5.h's; what is the input side's own is the per-stream Job — input streams begin, end and are covered
// differently in every launch set — and the rule that says which decoded samples enter the digest (Slot, advance): a FLAC frame that two
// sets decode is hashed once.
//
// Plain C++ for host and device alike.
#ifndef ELEMHIP_FLAC_IN_MD5_H
#define ELEMHIP_FLAC_IN_MD5_H
#include "flac_md5.h"

namespace flac_in_md5 {

using flac_md5::Record;

PCM_CX bool bits_ok(uint32_t bits) { return bits == 8u || bits == 12u || bits == 16u || bits == 20u || bits == 24u; }
constexpr uint32_t kMaxChannels = 8;

// what one wave does for its stream in one launch: samples [first, first + count) of every channel row enter the stream's digest —
// channel g's at scratch[base + g * stride + ...] — and with `finish` the message ends: padded, chained, 16 bytes written
struct Job { uint32_t base, stride, first, count, finish, pad[3]; };
static_assert(sizeof(Job) == 32, "a multiple of 16 bytes");

// ---- the rule --------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kOff = 0, kRunning = 1, kComplete = 2, kBroken = 3;
struct Slot {
    uint32_t state, bits, channels, pad;
    uint64_t hashedTo, total;       // stream samples in the digest so far; the stream's (its table's closing entry)
};
// the stream's length: what the caller says it is (elemhip_flac_in's total_samples — the table may be a slice of the stream's), else the
// table's closing entry
inline uint64_t total_of(uint64_t totalSamples, uint64_t closing) { return totalSamples ? totalSamples : closing; }
// a stream is about to feed the slot: another total, sample size or channel count than the slot runs with breaks it
inline void identify(Slot& s, uint32_t bits, uint32_t channels, uint64_t total) {
    if ((s.state == kRunning || s.state == kComplete) && (s.bits != bits || s.channels != channels || s.total != total)) s.state = kBroken;
}
// Stream samples [c0, c1) were decoded (c1 <= total): [lo, c1) of them enter the digest — none where that is empty — and `finish` says
// that the stream's last sample is among them. A gap in front of c0 breaks the slot for good. Returns whether anything is to be done.
inline bool advance(Slot& s, uint32_t bits, uint32_t channels, uint64_t total, uint64_t c0, uint64_t c1, uint64_t& lo, bool& finish) {
    lo = c1; finish = false;
    identify(s, bits, channels, total);
    if (s.state == kBroken || c1 <= c0) return false;
    if (c1 > total) { s.state = kBroken; return false; }       // (a table that runs past the length it was announced with)
    if (s.state == kOff) { s.state = kRunning; s.bits = bits; s.channels = channels; s.total = total; s.hashedTo = 0; }
    if (c0 > s.hashedTo) { s.state = kBroken; return false; }
    if (c1 <= s.hashedTo) return false;
    lo = s.hashedTo; s.hashedTo = c1;
    if (s.hashedTo == s.total && s.state == kRunning) { s.state = kComplete; finish = true; }
    return true;
}

// ---- the scalar twin: the kernel's schedule walked serially -------------------------------------------------------------------------------
// (flac_md5::run at the input side's sample sizes.) `count` samples from `first` on of planar[g] enter the record; with `digest` the
// message ends here
inline void update_codes(Record& r, const int32_t* const* planar, uint32_t G, uint32_t first, uint64_t count, uint32_t bits, uint8_t* digest = nullptr) {
    flac_md5::run(r, [planar](uint32_t g, uint32_t f) { return planar[g][f]; }, G, first, count, bits, digest);
}
// a job as the kernel reads it, over the scratch
inline void run_job(Record& r, const int32_t* scratch, const Job& j, uint32_t G, uint32_t bits, uint8_t* digest) {
    if (j.count == 0u && !j.finish) return;
    const int32_t* rows = scratch + j.base;
    const uint32_t stride = j.stride;
    flac_md5::run(r, [rows, stride](uint32_t g, uint32_t f) { return rows[(size_t)g * stride + f]; }, G, j.first, j.count, bits, j.finish ? digest : nullptr);
}

} // namespace flac_in_md5
#endif
