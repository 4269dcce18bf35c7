// flac_decode.h — the arithmetic and the lane schedule of FLAC input (flac_decode.hip, engine_flac_in.cpp): flac_encode.h backwards, and wider.
//
// An offline render's input arrives as RFC 9639 FLAC frames of a fixed block size. For every launch set the frames that cover the
// set's input frames are decoded on the GPU into the image an interleaved PCM stream of the same samples would leave in the packed
// input half (pcm_pack::stream_stride strides; s16 for samples of up to 16 bits, packed s24 above), so that the unpack kernel or the
// input-rate converter runs behind it unchanged. Decoding is stateless per FLAC frame: a frame that straddles two sets or two calls
// is decoded in both and only the part inside the range is stored — the result does not depend on how a render is cut.
//
// What is read: CONSTANT, VERBATIM, FIXED 0..4 and LPC 1..32 subframes (precision 1..15, shift 0..31, sums in 64 bits), wasted bits,
// both residual coding methods with partition orders 0..15 where they divide the block, escaped partitions (zero raw bits included),
// all four channel assignments (the 25-bit side channel of 24-bit streams included), 8 / 12 / 16 / 20 / 24 bits, 1..8 channels, blocks
// of up to 16384 samples, every block-size and sample-rate code, frame numbers on 1..6 bytes. Refused ("unsupported"): variable block
// size, 32-bit samples, blocks above 16384.
//
// The kernels (flac_decode.hip):
//   parse    one lane per (stream, FLAC frame): header, then the subframes in bit order through a bounded 64-bit window (BitReader);
//            per subframe a descriptor (Sub) and, at their sample positions in an int32 scratch [stream][channel][covered samples],
//            the warm-up samples and the residuals (parse_lane)
//   restore  one workgroup per (stream, FLAC frame), one wave per channel: FIXED order n as n prefix sums across the wave in 32-bit
//            wrap-around arithmetic, seeded by fixed_seed, in chunks of 64 with carry; LPC as lane 0's serial loop (the floor shift makes
//            it non-linear); CONSTANT a fill, VERBATIM as it is; the wasted-bit shift. Then all lanes: the frame's CRC-16 from lane
//            chunks combined with crc16_advance (lane_crc), the stereo undo in place (stereo_pair) and the range check
//   store    thread <-> 16-byte piece of a stream's image: the bytes of the samples inside [first input frame, first + valid) from the
//            scratch (image_piece), one 16-byte store each; frames past the stream's end, and frames that failed, are zeros
// An error record — count and the first (stream, frame, reason) — comes back with the set.
//
// Every read is clamped to the frame's bytes and every store to the frame's samples: a malformed frame ends in a reason, never in
// an access outside its buffers. A frame's bytes are those between its table entry and the next, the CRC-16 the last two of them.
//
// Plain C++ for host and device alike: tests/native/flac_decode_host.cpp runs the lane functions lane by lane against decode_host(),
// the scalar twin — which is also the production path where a render's inputs are needed on the host (taps under a sliced host block).
#ifndef ELEMHIP_FLAC_DECODE_H
#define ELEMHIP_FLAC_DECODE_H
#include "flac_encode.h"

namespace flac_decode {

using flac_encode::crc8_update;
using flac_encode::crc16_update;
using flac_encode::crc16_advance;

constexpr uint32_t kMinBlock = 16;             // (a shorter block only as a stream's last frame)
constexpr uint32_t kMaxBlock = 16384;
constexpr uint32_t kMaxChannels = 8;
constexpr uint32_t kMaxLpcOrder = 32;
constexpr uint32_t kFormat = 4;                // the input format code of a FLAC source (elemhip_pcm_in_spec)
// why a frame was refused
constexpr uint32_t OK = 0, BAD_CRC = 1, RESERVED = 2, BITS_MISSING = 3, PADDING = 4, OUT_OF_RANGE = 5, UNSUPPORTED = 6;
constexpr uint32_t CONSTANT = 0, VERBATIM = 1, FIXED = 2, LPC = 3;
constexpr uint32_t INDEPENDENT = 0, LEFT_SIDE = 8, SIDE_RIGHT = 9, MID_SIDE = 10;      // channel assignments (below 8: channels - 1)

PCM_CX bool bits_ok(uint32_t bits) { return bits == 8u || bits == 12u || bits == 16u || bits == 20u || bits == 24u; }
// ---- the image: what the H2D copy of a PCM stream of the same samples leaves ----------------------------------------------------------
PCM_CX uint32_t image_format(uint32_t bits) { return bits <= 16u ? pcm_pack::S16 : pcm_pack::S24; }
// the sample's bytes, little-endian in the low bits: exact under pcm_unpack::decode
PCM_FD uint32_t image_raw(uint32_t bits, int32_t code) {
    return bits <= 16u ? ((uint32_t)code << (16u - bits)) & 0xFFFFu : ((uint32_t)code << (24u - bits)) & 0xFFFFFFu;
}

// ---- frame header -----------------------------------------------------------------------------------------------------------------------
struct Header { uint32_t blockSize, rateCode, rate /* 0: STREAMINFO's */, channels, assignment, bps, number, bytes; };
// `avail` bytes at p. OK, or why not; a header whose CRC-8 holds but that this decoder does not read answers UNSUPPORTED.
PCM_FD uint32_t parse_header(const uint8_t* p, uint32_t avail, uint32_t streamBps, Header& h) {
    if (avail < 6u) return BITS_MISSING;
    if (p[0] != 0xFFu || (p[1] & 0xFEu) != 0xF8u) return RESERVED;
    const bool variable = (p[1] & 1u) != 0u;
    const uint32_t bc = p[2] >> 4, rc = p[2] & 15u, ca = p[3] >> 4, sc = (p[3] >> 1) & 7u;
    uint32_t at = 4u, nb = 1u;
    uint64_t number = p[4];
    if (number >= 0x80u) {
        nb = 0u;
        while (nb < 8u && ((p[4] << nb) & 0x80u)) ++nb;
        if (nb < 2u || nb > 7u) return RESERVED;
        if (at + nb > avail) return BITS_MISSING;
        number = p[4] & (0x7Fu >> nb);
        for (uint32_t k = 1; k < nb; ++k) {
            if ((p[4u + k] & 0xC0u) != 0x80u) return RESERVED;
            number = (number << 6) | (p[4u + k] & 0x3Fu);
        }
    }
    at += nb;
    const uint32_t tail = (bc == 6u ? 1u : bc == 7u ? 2u : 0u) + (rc == 12u ? 1u : rc == 13u || rc == 14u ? 2u : 0u);
    if (at + tail + 1u > avail) return BITS_MISSING;
    uint32_t n;
    if (bc == 6u) { n = (uint32_t)p[at] + 1u; at += 1u; }
    else if (bc == 7u) { n = (((uint32_t)p[at] << 8) | p[at + 1u]) + 1u; at += 2u; }
    else n = bc == 0u ? 0u : bc == 1u ? 192u : bc <= 5u ? 576u << (bc - 2u) : 256u << (bc - 8u);      // (bc 0 is reserved: refused below)
    uint32_t rate = 0u;
    if (rc == 12u) { rate = (uint32_t)p[at] * 1000u; at += 1u; }
    else if (rc == 13u || rc == 14u) { rate = (((uint32_t)p[at] << 8) | p[at + 1u]) * (rc == 13u ? 1u : 10u); at += 2u; }
    uint8_t crc = 0;
    for (uint32_t i = 0; i < at; ++i) crc = crc8_update(crc, p[i]);
    if (crc != p[at]) return BAD_CRC;
    if ((p[3] & 1u) || bc == 0u || rc == 15u || sc == 3u || ca > 10u) return RESERVED;
    if (variable || nb > 6u || sc == 7u || n > kMaxBlock) return UNSUPPORTED;
    h.blockSize = n; h.rateCode = rc; h.rate = rate;
    h.channels = ca < 8u ? ca + 1u : 2u; h.assignment = ca < 8u ? INDEPENDENT : ca;
    h.bps = sc == 0u ? streamBps : sc == 1u ? 8u : sc == 2u ? 12u : sc == 4u ? 16u : sc == 5u ? 20u : 24u;
    h.number = (uint32_t)number; h.bytes = at + 1u;
    return OK;
}

// ---- the index ----------------------------------------------------------------------------------------------------------------------------
// A stream's bytes behind its metadata -> frame byte offsets and first samples, one closing entry (offset = `bytes`, first sample = the
// samples in all) behind them. `blockSize` 0: the first frame's. A sync candidate is the next frame only where its header CRC-8 holds,
// its number is the previous one plus one, its fixed fields agree with the stream and its block size is the stream's — a shorter block
// closes the stream. The frames' CRC-16 is not looked at: the GPU checks it. *entries = the entries in all (frames + 1); the tables
// receive the first `cap` of them. OK, UNSUPPORTED where the first frame-like header is one this decoder does not read, RESERVED where
// bytes hold no frame at all.
inline uint32_t index_host(const uint8_t* d, size_t bytes, uint32_t channels, uint32_t bps, uint32_t blockSize, uint64_t* off, uint64_t* first,
                           size_t cap, size_t* entries) {
    *entries = 0;
    if (!bits_ok(bps) || channels == 0u || channels > kMaxChannels || blockSize > kMaxBlock || (blockSize && blockSize < kMinBlock)) return UNSUPPORTED;
    size_t count = 0;
    uint64_t samples = 0;
    bool have = false, closed = false, unsupported = false;
    Header prev{};
    for (size_t pos = 0; pos + 6u <= bytes && !closed;) {
        if (d[pos] != 0xFFu || (d[pos + 1u] & 0xFEu) != 0xF8u) { ++pos; continue; }
        Header h{};
        const uint32_t r = parse_header(d + pos, (uint32_t)(bytes - pos < 32u ? bytes - pos : 32u), bps, h);
        if (r == UNSUPPORTED && !have) unsupported = true;
        bool ok = r == OK && h.channels == channels && h.bps == bps && (blockSize == 0u || h.blockSize <= blockSize);
        if (ok && have) ok = h.number == prev.number + 1u && h.rateCode == prev.rateCode && h.rate == prev.rate;
        if (!ok) { ++pos; continue; }
        if (blockSize == 0u) blockSize = h.blockSize;
        if (count < cap) { off[count] = pos; first[count] = samples; }
        ++count; samples += h.blockSize; prev = h; have = true;
        closed = h.blockSize < blockSize;
        pos += h.bytes + 3u;                       // (a subframe header, a sample and the CRC-16 at least)
    }
    if (count < cap) { off[count] = bytes; first[count] = samples; }
    *entries = count + 1u;
    if (count == 0u && bytes) return unsupported ? UNSUPPORTED : RESERVED;
    return OK;
}

// ---- bits -----------------------------------------------------------------------------------------------------------------------------------
// A 64-bit window over the frame's bytes [0, bytes): the next bit is the window's top one. Reads behind the last byte set `over` and
// answer zeros; nothing outside [p, p + bytes) is touched.
struct BitReader {
    const uint8_t* p; uint32_t bytes, pos; uint64_t win; uint32_t fill; bool over;
    PCM_FD BitReader(const uint8_t* data, uint32_t n, uint32_t from) : p(data), bytes(n), pos(from < n ? from : n), win(0), fill(0), over(false) {}
    PCM_FD void refill() {
        while (fill <= 56u && pos < bytes) { win |= (uint64_t)p[pos++] << (56u - fill); fill += 8u; }
    }
    PCM_FD uint32_t read(uint32_t nb) {            // nb <= 32
        if (nb == 0u) return 0u;
        refill();
        if (nb > fill) { over = true; win = 0; fill = 0; return 0u; }
        const uint32_t v = (uint32_t)(win >> (64u - nb));
        win <<= nb; fill -= nb;
        return v;
    }
    PCM_FD uint32_t unary() {                      // zero bits in front of the next one bit, which is consumed
        uint32_t q = 0;
        for (;;) {
            refill();
            if (fill == 0u) { over = true; return q; }
            if (win == 0u) { q += fill; fill = 0; continue; }      // (the bits under `fill` are zero by construction)
            const uint32_t lz = (uint32_t)__builtin_clzll(win);
            q += lz;
            if (lz + 1u >= 64u) { win = 0; } else win <<= lz + 1u;
            fill -= lz + 1u;
            return q;
        }
    }
    PCM_FD uint32_t bit_pos() const { return pos * 8u - fill; }
};
PCM_FD int32_t sign_extend(uint32_t v, uint32_t nb) { return nb == 0u ? 0 : (int32_t)(v << (32u - nb)) >> (32u - nb); }

// ---- subframes --------------------------------------------------------------------------------------------------------------------------------
struct Sub { uint8_t kind, order, bps /* of the coded samples: wasted bits taken off */, wasted, shift, precision; int16_t coef[kMaxLpcOrder]; };

// the residual's partitions -> out[order .. n)
PCM_FD uint32_t parse_residual(BitReader& br, uint32_t n, uint32_t order, int32_t* out) {
    const uint32_t method = br.read(2u);
    if (br.over) return BITS_MISSING;
    if (method > 1u) return RESERVED;
    const uint32_t pb = 4u + method, porder = br.read(4u);
    if ((n & ((1u << porder) - 1u)) != 0u || (n >> porder) < order) return RESERVED;
    const uint32_t part = n >> porder;
    uint32_t i = order;
    for (uint32_t p = 0; p < (1u << porder); ++p) {
        const uint32_t cnt = part - (p == 0u ? order : 0u), k = br.read(pb);
        if (br.over) return BITS_MISSING;
        if (k == (1u << pb) - 1u) {
            const uint32_t raw = br.read(5u);
            for (uint32_t j = 0; j < cnt; ++j, ++i) {
                const int32_t r = sign_extend(br.read(raw), raw);
                if (br.over) return BITS_MISSING;
                if (i < n) out[i] = r;
            }
            continue;
        }
        for (uint32_t j = 0; j < cnt; ++j, ++i) {
            const uint32_t q = br.unary(), low = br.read(k);
            if (br.over) return BITS_MISSING;
            const uint64_t u = ((uint64_t)q << k) | low;
            if (u > 0xFFFFFFFFull) return OUT_OF_RANGE;
            if (i < n) out[i] = (int32_t)(((uint32_t)u >> 1) ^ (0u - ((uint32_t)u & 1u)));
        }
    }
    return OK;
}
// One subframe of `n` samples of `bps` bits: the descriptor, and in out[0, n) the warm-up samples (the value of a CONSTANT, the
// samples of a VERBATIM) with the residuals behind them.
PCM_FD uint32_t parse_subframe(BitReader& br, uint32_t n, uint32_t bps, Sub& sub, int32_t* out) {
    const uint32_t head = br.read(8u);
    if (br.over) return BITS_MISSING;
    if (head & 0x80u) return RESERVED;
    const uint32_t type = (head >> 1) & 63u;
    uint32_t wasted = 0u;
    if (head & 1u) {
        wasted = br.unary() + 1u;
        if (br.over) return BITS_MISSING;
        if (wasted >= bps) return RESERVED;
        bps -= wasted;
    }
    sub.bps = (uint8_t)bps; sub.wasted = (uint8_t)wasted; sub.order = 0; sub.shift = 0; sub.precision = 0;
    if (type == 0u) {
        sub.kind = CONSTANT;
        const int32_t v = sign_extend(br.read(bps), bps);
        if (n) out[0] = v;
        return br.over ? BITS_MISSING : OK;
    }
    if (type == 1u) {
        sub.kind = VERBATIM;
        for (uint32_t i = 0; i < n; ++i) {
            out[i] = sign_extend(br.read(bps), bps);
            if (br.over) return BITS_MISSING;
        }
        return OK;
    }
    uint32_t order;
    if (type >= 8u && type <= 12u) { sub.kind = FIXED; order = type - 8u; }
    else if (type >= 32u) { sub.kind = LPC; order = type - 31u; }
    else return RESERVED;
    if (order > n) return RESERVED;
    sub.order = (uint8_t)order;
    for (uint32_t i = 0; i < order; ++i) out[i] = sign_extend(br.read(bps), bps);
    if (br.over) return BITS_MISSING;
    if (sub.kind == LPC) {
        const uint32_t prec = br.read(4u) + 1u;
        if (prec == 16u) return RESERVED;
        const int32_t shift = sign_extend(br.read(5u), 5u);
        if (br.over) return BITS_MISSING;
        if (shift < 0) return RESERVED;
        sub.precision = (uint8_t)prec; sub.shift = (uint8_t)shift;
        for (uint32_t j = 0; j < order; ++j) sub.coef[j] = (int16_t)sign_extend(br.read(prec), prec);
        if (br.over) return BITS_MISSING;
    }
    return parse_residual(br, n, order, out);
}

// ---- the parse kernel's lane: one frame ------------------------------------------------------------------------------------------------------------
// `f`: the frame's `len` bytes, CRC-16 included. The frame has to be one of the stream (`channels`, `bps`) with `n` samples (what the
// table says). subs[c] and scratch[c * stride + [0, n)] are written for every channel; *assignment receives the channel assignment.
PCM_FD uint32_t parse_lane(const uint8_t* f, uint32_t len, uint32_t channels, uint32_t bps, uint32_t n, Sub* subs, int32_t* scratch, size_t stride,
                           uint32_t* assignment) {
    *assignment = INDEPENDENT;
    for (uint32_t c = 0; c < channels; ++c) { subs[c].kind = CONSTANT; subs[c].order = 0; subs[c].bps = (uint8_t)bps; subs[c].wasted = 0; subs[c].shift = 0; subs[c].precision = 0; }
    if (len < 2u) return BITS_MISSING;
    const uint32_t body = len - 2u;
    Header h{};
    const uint32_t r = parse_header(f, body, bps, h);
    if (r != OK) return r;
    if (h.channels != channels || h.bps != bps || h.blockSize != n) return RESERVED;
    *assignment = h.assignment;
    BitReader br(f, body, h.bytes);
    for (uint32_t c = 0; c < channels; ++c) {
        const bool side = (h.assignment == LEFT_SIDE && c == 1u) || (h.assignment == SIDE_RIGHT && c == 0u) || (h.assignment == MID_SIDE && c == 1u);
        const uint32_t rs = parse_subframe(br, n, bps + (side ? 1u : 0u), subs[c], scratch + c * stride);
        if (rs != OK) return rs;
    }
    const uint32_t pad = (8u - (br.bit_pos() & 7u)) & 7u;
    if (br.read(pad) != 0u) return PADDING;
    if (br.over) return BITS_MISSING;
    if (br.bit_pos() != body * 8u) return PADDING;          // bytes between the subframes' end and the CRC-16
    return OK;
}

// ---- the restore kernel's functions ----------------------------------------------------------------------------------------------------------------
// FIXED order n as n inclusive prefix sums (mod 2^32): pass p = n .. 1 puts fixed_seed(s, p) — the (p - 1)th difference at sample
// p - 1, from the warm-up samples — at position p - 1 and sums positions [p - 1, N); what was the pth difference behind it becomes
// the (p - 1)th. After pass 1 the positions hold the samples.
PCM_FD uint32_t fixed_seed(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, uint32_t p) {      // s0 .. s3: the warm-up samples (those the order has)
    switch (p) {
        case 1: return s0;
        case 2: return s1 - s0;
        case 3: return s2 - 2u * s1 + s0;
        default: return s3 - 3u * s2 + 3u * s1 - s0;
    }
}
// sample i >= order of an LPC subframe from its residual and the samples in front of it
PCM_FD int32_t lpc_sample(const Sub& sub, const int32_t* s, uint32_t i) {
    int64_t sum = 0;
    for (uint32_t j = 0; j < sub.order; ++j) sum += (int64_t)sub.coef[j] * (int64_t)s[i - 1u - j];
    return (int32_t)((uint32_t)s[i] + (uint32_t)(uint64_t)(sum >> sub.shift));
}
PCM_FD int32_t unwaste(int32_t v, uint32_t wasted) { return (int32_t)((uint32_t)v << wasted); }
// the scalar restore of one subframe, in place (wasted bits included)
PCM_FD void restore_serial(const Sub& sub, int32_t* s, uint32_t n) {
    uint32_t* u = reinterpret_cast<uint32_t*>(s);
    if (sub.kind == CONSTANT) { for (uint32_t i = 1; i < n; ++i) s[i] = s[0]; }
    else if (sub.kind == FIXED) {
        for (uint32_t i = sub.order; i < n; ++i) {
            switch (sub.order) {
                case 0: break;
                case 1: u[i] += u[i - 1]; break;
                case 2: u[i] += 2u * u[i - 1] - u[i - 2]; break;
                case 3: u[i] += 3u * u[i - 1] - 3u * u[i - 2] + u[i - 3]; break;
                default: u[i] += 4u * u[i - 1] - 6u * u[i - 2] + 4u * u[i - 3] - u[i - 4]; break;
            }
        }
    } else if (sub.kind == LPC) { for (uint32_t i = sub.order; i < n; ++i) s[i] = lpc_sample(sub, s, i); }
    if (sub.wasted) for (uint32_t i = 0; i < n; ++i) s[i] = unwaste(s[i], sub.wasted);
}
// the CRC of lane `lane`'s chunk of the frame's `total` bytes in front of the CRC-16, advanced to the end: the lanes' values XORed
// are the frame's CRC
PCM_FD uint16_t lane_crc(const uint8_t* f, uint32_t total, uint32_t lane, uint32_t lanes) {
    const uint32_t c = (total + lanes - 1u) / lanes, b = lane * (uint64_t)c < total ? lane * c : total, e = b + c < total ? b + c : total;
    if (b == e) return 0u;
    uint16_t crc = 0;
    for (uint32_t i = b; i < e; ++i) crc = crc16_update(crc, f[i]);
    return crc16_advance(crc, total - e);
}
// the stereo undo of one sample pair; false where a result leaves the stream's range
PCM_FD bool in_range(int64_t v, uint32_t bps) { const int64_t lim = (int64_t)1 << (bps - 1u); return v >= -lim && v < lim; }
PCM_FD bool stereo_pair(uint32_t assignment, uint32_t bps, int32_t& a, int32_t& b) {
    int64_t l = a, r = b;
    if (assignment == LEFT_SIDE) r = l - r;
    else if (assignment == SIDE_RIGHT) l = l + r;
    else if (assignment == MID_SIDE) {
        const int64_t m = a, s = b;
        l = (((m * 2) | (s & 1)) + s) >> 1;
        r = l - s;
    }
    a = (int32_t)(uint32_t)(uint64_t)l; b = (int32_t)(uint32_t)(uint64_t)r;
    return in_range(l, bps) && in_range(r, bps);
}

// ---- the store kernel's thread: one 16-byte piece of a stream's image -----------------------------------------------------------------------------
// Piece `piece` of the image of `valid` frames x G channels: sample (frame, g) comes from chan(g, frame) where frame < have (the
// frames the stream still holds), zero behind. out[16] receives the bytes; bytes behind the image's end are zero.
template <class Chan>
PCM_FD void image_piece(uint32_t bits, uint32_t G, uint32_t valid, uint32_t have, uint32_t piece, Chan chan, uint8_t* out) {
    const uint32_t B = bits <= 16u ? 2u : 3u;
    const uint64_t end = (uint64_t)valid * G * B;
    uint64_t at = (uint64_t)piece * 16u;
    uint64_t j = at / B;
    uint32_t k = (uint32_t)(at % B), g = (uint32_t)(j % G);
    uint64_t frame = j / G;
    uint32_t raw = 0u;
    bool loaded = false;
    for (uint32_t i = 0; i < 16u; ++i, ++at) {
        if (at >= end) { out[i] = 0u; continue; }
        if (!loaded) { raw = frame < have ? image_raw(bits, chan(g, (uint32_t)frame)) : 0u; loaded = true; }
        out[i] = (uint8_t)(raw >> (8u * k));
        if (++k == B) { k = 0u; loaded = false; if (++g == G) { g = 0u; ++frame; } }
    }
}

// ---- a launch set's records: what the host tells the kernels ----------------------------------------------------------------------------------------
struct FrameRec {                   // one FLAC frame that covers part of the set's input frames; ordered by stream, then by frame
    uint32_t byteOff, len;          // its bytes in the staged half (CRC-16 included)
    uint32_t stream, index;         // whose it is, and its index in that stream's table
    uint32_t n;                     // its samples (what the table says)
    uint32_t scratchOff, chStride;  // channel c's samples at scratch[scratchOff + c * chStride + [0, n))
    uint32_t pad;
};
struct StreamRec {
    uint32_t firstFrame, frames;    // its FrameRec records
    uint32_t blockSize;             // of all its frames but a shorter last one
    uint32_t skip;                  // samples of its first covering frame in front of the set's first input frame
    uint32_t have;                  // input frames of the set the stream still holds (behind them: silence)
    uint32_t scratchBase, covered;  // channel c's covered samples at scratch[scratchBase + c * covered + ...]
    uint32_t pad;
};
struct ErrorRec { uint32_t count, pad; unsigned long long first; };      // first: ~((FrameRec index << 8) | reason) of the smallest index; 0: none

// ---- the scalar twin (host) ------------------------------------------------------------------------------------------------------------------------
// One frame -> out[c * stride + [0, n)], stereo undone, range checked. The checks in the kernels' order: CRC-16, parse, range.
inline uint32_t decode_frame_host(const uint8_t* f, uint32_t len, uint32_t channels, uint32_t bps, uint32_t n, int32_t* out, size_t stride) {
    if (len < 2u) return BITS_MISSING;
    uint16_t crc = 0;
    for (uint32_t i = 0; i + 2u < len; ++i) crc = crc16_update(crc, f[i]);
    if (crc != (uint16_t)(((uint32_t)f[len - 2u] << 8) | f[len - 1u])) return BAD_CRC;
    Sub subs[kMaxChannels];
    uint32_t assignment;
    const uint32_t r = parse_lane(f, len, channels, bps, n, subs, out, stride, &assignment);
    if (r != OK) return r;
    for (uint32_t c = 0; c < channels; ++c) restore_serial(subs[c], out + c * stride, n);
    bool ok = true;
    if (assignment != INDEPENDENT) { for (uint32_t i = 0; i < n; ++i) ok = stereo_pair(assignment, bps, out[i], out[stride + i]) && ok; }
    else for (uint32_t c = 0; c < channels; ++c) for (uint32_t i = 0; i < n; ++i) ok = in_range(out[c * stride + i], bps) && ok;
    return ok ? OK : OUT_OF_RANGE;
}
// the frame that holds stream sample `t` (t < first[frames]): the last entry whose first sample is <= t
inline size_t frame_of(const uint64_t* first, size_t frames, uint64_t t) {
    size_t lo = 0, hi = frames;
    while (hi - lo > 1u) { const size_t mid = lo + (hi - lo) / 2u; if (first[mid] <= t) lo = mid; else hi = mid; }
    return lo;
}
// Stream samples [position, position + count) -> planar[c][0, count): every frame that covers part of the range is decoded whole and
// the part inside stored; samples past the stream's end are zeros. `off` / `first`: the table, frames + 1 entries. OK, or the first
// failing frame's reason and (in *badFrame) its index.
inline uint32_t decode_host(const uint8_t* data, const uint64_t* off, const uint64_t* first, size_t frames, uint32_t channels, uint32_t bps,
                            uint64_t position, size_t count, int32_t* const* planar, size_t* badFrame) {
    const uint64_t total = frames ? first[frames] : 0u;
    for (uint32_t c = 0; c < channels; ++c) for (size_t i = 0; i < count; ++i) planar[c][i] = 0;
    if (position >= total || count == 0u) return OK;
    const uint64_t end = position + count < total ? position + count : total;
    std::vector<int32_t> tmp;
    for (size_t j = frame_of(first, frames, position); j < frames && first[j] < end; ++j) {
        const uint64_t n64 = first[j + 1u] - first[j], len64 = off[j + 1u] - off[j];
        if (badFrame) *badFrame = j;
        if (n64 == 0u || n64 > kMaxBlock || off[j + 1u] < off[j] || len64 > 0x7FFFFFFFull) return UNSUPPORTED;
        const uint32_t n = (uint32_t)n64;
        tmp.assign((size_t)channels * n, 0);
        const uint32_t r = decode_frame_host(data + off[j], (uint32_t)len64, channels, bps, n, tmp.data(), n);
        if (r != OK) return r;
        const uint64_t lo = first[j] > position ? first[j] : position, hi = first[j + 1u] < end ? first[j + 1u] : end;
        for (uint32_t c = 0; c < channels; ++c)
            for (uint64_t t = lo; t < hi; ++t) planar[c][t - position] = tmp[(size_t)c * n + (size_t)(t - first[j])];
    }
    return OK;
}
// planar codes -> the interleaved image (count frames x channels samples of 2 or 3 bytes)
inline void image_host(uint32_t bits, uint32_t channels, const int32_t* const* planar, size_t count, uint8_t* out) {
    const uint32_t B = bits <= 16u ? 2u : 3u;
    for (size_t f = 0; f < count; ++f)
        for (uint32_t g = 0; g < channels; ++g) {
            const uint32_t raw = image_raw(bits, planar[g][f]);
            for (uint32_t k = 0; k < B; ++k) out[(f * channels + g) * B + k] = (uint8_t)(raw >> (8u * k));
        }
}

} // namespace flac_decode

#endif // ELEMHIP_FLAC_DECODE_H
