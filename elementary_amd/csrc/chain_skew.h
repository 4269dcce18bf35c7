// chain_skew.h — the lane schedule of the quad-skewed recurrence loop of the specialised kernels (island_ops.inc, chain_loop_d).
//
// A recurrence task of up to 16 members gives every member FOUR lanes. All four run the member's whole chain with the same
// instructions on the same operand values, but lane 4m+k (skew k) runs it 4k frames late: at loop step s it computes frame
// s - 4k. After the 16 steps of group g the LAST four results of a lane are therefore frames 16g + 12 - 4k .. 16g + 15 - 4k:
// the four lanes of a quad hold the group's 16 frames between them, and ONE 16-byte store per lane writes the group where
// the unskewed loop issues four (a store costs the lone recurrence wave per INSTRUCTION, not per byte or per lane).
//
//   step of the block    0 ........ n-1
//   skew 0               frames 0 .. n-1
//   skew k               holds for 4k steps (head), then frames 0 .. n-1-4k
//
// Head: in group 0 a lane of skew k sits out the first 4k steps (its state is the block's initial state). The operands of
// step s are loaded per lane, 16 bytes at a time, 16k bytes in front of the unskewed address; in the head that address is
// clamped into the operand's block buffer (what a clamped load returns is never used: its steps are the ones the predicate
// switches off). After the last group every frame is stored and the lane of skew 0 holds the member's final state: every
// lane takes the state registers of state_lane(lane), the first lane of its quad. (Until r08 the lanes of skew k ran 4k more
// predicated steps there, the tail, on three more clamped loads per operand, to arrive at the same bits; kTailSteps and
// tail_active describe that schedule, and tests/native/chain_skew_host.cpp still emulates it as the reference for this one.)
//
// Written as plain index arithmetic for host and device alike: tests/native/chain_skew_host.cpp, chain_carry_host.cpp and
// chain_window_host.cpp emulate the loop with these functions and check frames, final states, load offsets and store windows
// without a GPU.
#ifndef ELEMHIP_CHAIN_SKEW_H
#define ELEMHIP_CHAIN_SKEW_H
#ifndef __HIPCC_RTC__        // (the run-time compiler has no host headers: jit.cpp declares the fixed-width names)
#include <stdint.h>
#endif

#if defined(__HIPCC__) || defined(__HIP__) || defined(__HIPCC_RTC__)
#define CSKEW_FD __host__ __device__ constexpr __forceinline__
#else
#define CSKEW_FD constexpr inline
#endif

namespace chain_skew {

constexpr uint32_t kGroup = 16;        // frames per group (chain_loop_d CHG)
constexpr uint32_t kQuad = 4;          // lanes per member = frames per 16-byte piece
constexpr uint32_t kMaxCount = 16;     // members of a task that fit a 64-lane wave
constexpr uint32_t kTailSteps = 12;    // steps of the former tail (skew 3 ran all of them)

// the task shapes the schedule covers
CSKEW_FD bool applies(uint32_t count) { return count >= 1u && count <= kMaxCount; }

// lane -> member of the task (lanes at or beyond 4 * count mirror the last member)
CSKEW_FD uint32_t lane_member(uint32_t lane, uint32_t count) {
    return lane / kQuad < count ? lane / kQuad : count - 1u;
}
// lane -> skew (mirror lanes run unskewed: they neither store nor own a frame)
CSKEW_FD uint32_t lane_skew(uint32_t lane, uint32_t count) { return lane < kQuad * count ? lane % kQuad : 0u; }
// lanes that store: bit l set = lane l writes its piece of every group
CSKEW_FD unsigned long long store_mask(uint32_t count) { return count >= kMaxCount ? ~0ull : ((1ull << (kQuad * count)) - 1ull); }

// first of the four frames that y[12..15] of a lane of skew k hold after the 16 steps of group g
CSKEW_FD uint32_t stored_frame(uint32_t g, uint32_t k) { return kGroup * g + (kGroup - kQuad) - kQuad * k; }
// ... and the byte offset of that piece inside its group (the rest of the address is the unskewed loop's)
CSKEW_FD uint32_t store_bias(uint32_t k) { return 4u * ((kGroup - kQuad) - kQuad * k); }

// head: does a lane of skew k execute step j (0 .. 15) of group 0?
CSKEW_FD bool head_active(uint32_t k, uint32_t j) { return j >= kQuad * k; }
// the former tail: the steps j (0 .. 11) after the last group that a lane of skew k was still short of. Skew 0: none.
CSKEW_FD bool tail_active(uint32_t k, uint32_t j) { return j < kQuad * k; }
// after the last group: the lane whose state registers a lane takes (a mirror quad is four copies of one state)
CSKEW_FD uint32_t state_lane(uint32_t lane) { return lane - lane % kQuad; }
constexpr int kStateQuadPerm = 0x00;   // the DPP control that reads state_lane: quad_perm:[0,0,0,0]

// Byte offset, inside the operand's block buffer of n frames, of the 16-byte piece q (0 .. 3) of group g that a lane of skew k
// loads: frames 16g + 4q - 4k .. +3. Clamped into [0, 4n - 16]; only head pieces (g = 0) ever hit a bound, and exactly those
// whose steps head_active switches off. (Group n / 16 was the former tail's, clamped at the upper bound.)
CSKEW_FD uint32_t load_offset(uint32_t g, uint32_t q, uint32_t k, uint32_t n) {
    return 4u * (kGroup * g + kQuad * q) < 16u * k ? 0u
         : (4u * (kGroup * g + kQuad * q) - 16u * k > 4u * n - 16u ? 4u * n - 16u : 4u * (kGroup * g + kQuad * q) - 16u * k);
}
// Steady groups (1 .. n / 16 - 1) need no clamp: the lane's offset is the unskewed one plus this bias, taken from a VGPR offset
// that carries store_bias(0) = 48 bytes extra — so that it never goes below the buffer's own offset, whatever that is — with the
// 48 bytes taken off the instruction's immediate again.
CSKEW_FD uint32_t load_bias(uint32_t k) { return store_bias(0u) - 16u * k; }
constexpr int kLoadImmBias = -48;

// Store windows. A store runs with EXEC cut to store_mask, and the switch costs the lone wave four scalar issue slots (save, narrow,
// restore, one wait state) however many stores stand between: the loop keeps the result pieces of W consecutive groups in registers
// (4 VGPRs per deferred group) and the group that closes a window issues all W stores under ONE switch, in group order, each at the
// offset it always had. The groups of a span are d = 0 .. depth - 1; a window never leaves its span (window_fits), so its stores share
// the span's scalar offset, the last window of a block closes with the block's last group — every store is issued before the state
// hand-over and before the next block's first loads, which the deferred publish counts on — and a window of 1 is the former schedule.
constexpr uint32_t kWindowStreamed = 4;   // loops with a streamed operand (depth 8, 4 or 2)
constexpr uint32_t kWindowPlain = 4;      // loops without one (depth 4)
CSKEW_FD bool window_fits(uint32_t w, uint32_t depth) { return w >= 1u && w <= depth && depth % w == 0u; }
CSKEW_FD uint32_t window(bool streamed, uint32_t depth) {
    return (streamed ? kWindowStreamed : kWindowPlain) < depth ? (streamed ? kWindowStreamed : kWindowPlain) : depth;
}
// does group d of a span close a window of w groups? ...
CSKEW_FD bool window_closes(uint32_t d, uint32_t w) { return (d + 1u) % w == 0u; }
// ... and the first group of that window: the closing group d stores the pieces of groups window_first(d, w) .. d
CSKEW_FD uint32_t window_first(uint32_t d, uint32_t w) { return d + 1u - w; }

} // namespace chain_skew

#endif // ELEMHIP_CHAIN_SKEW_H
