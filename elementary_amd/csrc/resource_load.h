// resource_load.h — the arithmetic and the lane schedule of the resource loader (resource_load.hip, Engine::addSharedResourcePcm): a
// shared resource — the samples behind sample / table / sampleseq and their mc. forms, the impulse responses behind convolve — made on
// the GPU from the file's own bytes instead of from floats the host decoded.
//
// A source is ONE interleaved stream of G channels (1 .. 32) and N frames at `rate` Hz: 16-bit, packed 24-bit or float32 samples
// (pcm_pack.h's format codes), or FLAC, which flac_decode.hip first turns into the s16 / s24 image a PCM file of the same samples would
// be (flac_decode::image_format). The resource is planar: channel g is a row of floats of its own.
//
// Same rate.  Row g, frame f = pcm_unpack::decode(fmt, sample(f, g)): exact, the bits of add_shared_resource(decoded floats).
//
// Other rate.  A resample::Plan with fin = the file's rate and fout = the engine's; make_plan, make_tables and tap_sum<> unchanged. The
// resource holds outputs_before(plan, N) = ceil(N L / M) frames, and frame n is the delivery-side programme's output n + Do for the
// programme x[0 .. N) followed by silence: a = n M, i0 = floor(a / L), p = a - i0 L, y[n] = sum_k h[p][k] x[i0 - Wc + 1 + k], x = 0
// outside [0, N). The filter is centred: frame 0 of the file lies at frame 0 of the resource and there is no latency to take out. In the
// tables' terms output n is column (n + Do) mod L with centre(plan, rowBase, n + Do) = floor(n M / L).
//
// Pieces.  The source goes up through pinned staging in pieces of P source frames (Engine option "resource_load_frames"). Piece j owns
// the source frames [j P, min((j + 1) P, N)) and writes the resource frames whose centre i0 lies among them: [outputs_before(j P),
// outputs_before(end)) (i0 >= t <=> n >= ceil(t L / M)). Those read the source frames [j P - Wc + 1, end - 1 + Wc], so a piece stages that
// stretch cut to the file — T - 1 frames of overlap, no state carried from piece to piece: outside the file is silence, inside it is in
// the file. However the file is cut, the same bits. At the same rate a piece stages and writes its own frames.
// The staged bytes start at the 16-byte line of the FILE below the stretch's first byte (piece_head), so the staging copy is aligned
// like the stream and every 16-byte load of the kernels is aligned; the buffer is padded to whole lines behind.
//
// Same-rate kernel: pcm_unpack.h's three stages with rows of the resource as the destination. A tile is tile_frames(G) frames x G of a
// piece: A aligned 16-byte loads into the LDS image, B thread <-> sample in stream order, decoded, transposed into row_bases' skewed
// rows (a half-wave's 32 writes hit 32 banks for every G up to 32), C a wave per (row, 64 quads), quad_slot's conflict-free reads, one
// 16-byte store per whole quad and dword stores at a row's two ends.
// Converting kernel: resample.h's input-side tile — kTile outputs x C channels (C = kGroup; 1 for one channel and where four rows do not
// fit), the tile's input stretch decoded once into skew()ed LDS rows (a narrow stream, G <= C, through the aligned image; a wide one
// sample by sample), coefficients in output order, the sums from tap_sum.
//
// Plain C++ for host and device alike: tests/native/resource_load_host.cpp runs both kernels' stages lane by lane against load_host(),
// the scalar loop — the yardstick, and the production path of a handle without a device.
#ifndef ELEMHIP_RESOURCE_LOAD_H
#define ELEMHIP_RESOURCE_LOAD_H
#include "pcm_unpack.h"
#include "resample.h"

namespace resource_load {

namespace pp = pcm_pack;
namespace pu = pcm_unpack;
namespace rs = resample;

constexpr uint32_t kMaxChannels = 32;
constexpr uint32_t kMinPiece = 64, kDefaultPiece = 1u << 20, kMaxPiece = 1u << 24;      // source frames ("resource_load_frames")
constexpr uint64_t kMaxFrames = 0x7FFFFFFFull;                                          // of a resource

// frames of the resource made of N source frames (plan null: the same rate)
RS_FD uint64_t out_frames(const rs::Plan* plan, uint64_t N) { return plan ? rs::outputs_before(*plan, N) : N; }

// ---- pieces ---------------------------------------------------------------------------------------------------------------------------
struct Piece { uint64_t in0, in1, out0, out1; };      // source frames staged [in0, in1), resource frames written [out0, out1)
RS_FD uint64_t piece_count(uint64_t N, uint32_t P) { return (N + P - 1u) / P; }
RS_FD Piece piece_of(const rs::Plan* plan, uint64_t N, uint32_t P, uint64_t j) {
    const uint64_t p0 = j * P, p1 = p0 + P < N ? p0 + P : N;
    Piece pc;
    if (!plan) { pc.in0 = pc.out0 = p0; pc.in1 = pc.out1 = p1; return pc; }
    pc.in0 = p0 + 1u > plan->Wc ? p0 + 1u - plan->Wc : 0u;
    pc.in1 = p1 + plan->Wc < N ? p1 + plan->Wc : N;
    pc.out0 = rs::outputs_before(*plan, p0); pc.out1 = rs::outputs_before(*plan, p1);
    return pc;
}
// the staged copy of a piece of a PCM file: bytes [piece_begin - piece_head, ...) of the file, whole 16-byte lines
RS_FD uint64_t piece_begin(uint64_t in0, uint32_t G, uint32_t fmt) { return in0 * G * pp::sample_bytes(fmt); }
RS_FD uint32_t piece_head(uint64_t in0, uint32_t G, uint32_t fmt) { return (uint32_t)(piece_begin(in0, G, fmt) & 15u); }
RS_FD uint64_t piece_bytes(uint32_t head, uint64_t frames, uint32_t G, uint32_t fmt) { return (head + frames * G * pp::sample_bytes(fmt) + 15u) & ~(uint64_t)15u; }
// the largest staged copy of any piece
RS_FD uint64_t staging_bytes(const rs::Plan* plan, uint32_t P, uint32_t G, uint32_t fmt) {
    return piece_bytes(15u, (uint64_t)P + (plan ? 2u * plan->Wc : 0u), G, fmt);
}

// ---- the same-rate tile -----------------------------------------------------------------------------------------------------------------
// tile ti of a piece of `frames` frames: its first frame (piece-relative) and how many it holds
RS_FD uint32_t copy_tiles(uint32_t frames, uint32_t G) { const uint32_t t = pp::tile_frames(G); return (frames + t - 1u) / t; }
RS_FD uint32_t copy_tile_first(uint32_t ti, uint32_t G) { return ti * pp::tile_frames(G); }
RS_FD uint32_t copy_tile_frames(uint32_t frames, uint32_t G, uint32_t ti) {
    const uint32_t t = pp::tile_frames(G), f0 = ti * t;
    return f0 >= frames ? 0u : (frames - f0 < t ? frames - f0 : t);
}
// the tile's stretch in the staged copy: its first byte there
RS_FD uint64_t copy_stretch_begin(uint32_t head, uint32_t f0, uint32_t G, uint32_t fmt) { return (uint64_t)head + (uint64_t)f0 * G * pp::sample_bytes(fmt); }
// chunks of 64 quads of a row of n frames, whatever its address
RS_FD uint32_t copy_row_chunks(uint32_t n) { return (pp::row_quads(n, 3u) + 63u) / 64u; }

// ---- the converting tile ------------------------------------------------------------------------------------------------------------------
// resample.h's tile_of / lane_base / stream_part / skew / row_floats / in_lds_bytes with n0 = the piece's first output + Do: the
// centre of resource frame n is floor(n M / L)
RS_FD uint64_t programme_output(const rs::Plan& p, uint64_t n) { return n + p.Do; }
RS_FD uint32_t convert_channels(const rs::Plan& p, uint32_t G) {      // C of the launch; 0: not even one row fits
    if (G > 1u && rs::in_lds_bytes(p, rs::kGroup) <= 65536u) return rs::kGroup;
    return rs::in_lds_bytes(p, 1u) <= 65536u ? 1u : 0u;
}

// ---- one sample of the source -------------------------------------------------------------------------------------------------------------
RS_FD float source_at(uint32_t fmt, const unsigned char* data, uint32_t G, uint64_t N, int64_t f, uint32_t g) {
    if (f < 0 || (uint64_t)f >= N) return 0.0f;
    return pu::decode(fmt, pu::load_raw(fmt, data + ((size_t)f * G + g) * pp::sample_bytes(fmt)));
}

// ---- the scalar loop ------------------------------------------------------------------------------------------------------------------------
// rows[g] receives out_frames(plan, N) floats. `table` / `rowBase`: resample::make_tables of the plan (unused at the same rate).
inline void load_host(uint32_t fmt, uint32_t G, uint64_t N, const unsigned char* data, const rs::Plan* plan, const float* table,
                      const int32_t* rowBase, float* const* rows) {
    if (!plan) {
        for (uint32_t g = 0; g < G; ++g)
            for (uint64_t f = 0; f < N; ++f) {
                const uint32_t u = pu::decode_bits(fmt, pu::load_raw(fmt, data + ((size_t)f * G + g) * pp::sample_bytes(fmt)));
                memcpy(rows[g] + f, &u, 4);
            }
        return;
    }
    const rs::Plan& p = *plan;
    const uint64_t outN = rs::outputs_before(p, N);
    for (uint32_t g = 0; g < G; ++g)
        for (uint64_t n = 0; n < outN; ++n) {
            const uint64_t m = programme_output(p, n);
            const int64_t j0 = rs::centre(p, rowBase, m) - (int64_t)p.Wc + 1;
            rs::tap_sum<1>(table + m % p.L, p.L, p.T, [&](int, uint32_t k) { return source_at(fmt, data, G, N, j0 + (int64_t)k, g); }, rows[g] + n);
        }
}

} // namespace resource_load

#endif // ELEMHIP_RESOURCE_LOAD_H
