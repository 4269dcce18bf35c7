/* elemhip.h — C-ABI of the MI355X block-render engine (libelemhip.so).
 *
 * Drop-in boundary for ONE path of elemaudio/elementary: elem::Runtime<float>::process() and the
 * graph-mutation calls that feed it.  Every entry point replaces one member of
 * `elem::Runtime<float>` (runtime/elem/Runtime.h:39-153); the reference line it stands in for is
 * cited next to it.  Plain pointers and sizes only; the caller owns every pointer it passes and
 * the engine copies whatever it keeps.  Integer return codes 0..8 are the reference's
 * `elem::ReturnCode` (runtime/elem/Types.h:51-86); codes >= 100 are HIP-side failures.
 *
 * Threading contract: one mutator thread (apply/add/gc) + one render thread (process*) per
 * handle; mutations become visible atomically at the next process call (reference: SPSC queue of
 * render sequences, Runtime.h:133,204,277-285).  Two locks inside the engine: a control lock
 * serialises the mutator-side calls and owns the node table; a render lock guards what process*
 * touches.  process* take the render lock only, and a commit releases it while it plans the new
 * render sequence, so a render call never waits for a plan build; the mutator can
 * wait for a render call in flight (at most one launch set), never the other way round.
 *
 * The engine has NO CPU fallback: every block is rendered by HIP kernels for gfx950 — the
 * ahead-of-time island kernels (elementary_amd/csrc/kernels.hip, kernels_rt.hip: island.inc +
 * island_ops.inc), the convolve kernels (conv.hip) and the per-island-shape kernels compiled at run
 * time from island_spec.inc + generated text (codegen.cpp, jit.cpp); elemhip_create fails (NULL)
 * when no gfx950 device is usable.
 *
 * Block size: the reference sizes its buffers to any blockSize (Runtime.h:44); this engine keeps a
 * block's buffers in LDS slots of at most 512 frames. blockSize <= 512: as given. Above 512 (up to 32768): accepted when the block
 * splits into k EQUAL slices of 64 .. 512 frames (1024 = 2 x 512, 700 = 2 x 350, 1023 = 3 x 341; the smallest such k is taken):
 * elemhip_process / elemhip_process_blocks_host render such a block slice by slice — the same samples for every node that works at
 * the sample rate; tapIn / tapOut, whose delay IS the host's block (Feedback.h:29-31, 88-109), keep tap buffers of the HOST's block
 * size and every slice reads / promotes its own stretch of them (r04 refused such graphs with code 104);
 * `meter` reports the last slice of a block, and the device-resident elemhip_process_blocks (whose layout is in blocks) answers
 * 102. A size above 512 that no such k divides (a prime: 521, 1031): slices of 512 frames and a shorter last one. Above 32768:
 * elemhip_create fails (code 102). Nodes that size themselves by the block (`delay` / `sdelay` without a `size`, tap buffers) use
 * the HOST's block size, as in the reference (Delays.h:56, 183; Feedback.h:29-31).
 */
#ifndef ELEMHIP_H
#define ELEMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct elemhip_s elemhip_t;

typedef struct elemhip_stats {
    uint64_t blocks_rendered;
    uint64_t plans_built;
    double   last_plan_build_ms;
    uint32_t num_islands, num_levels, num_tasks, num_nodes_in_plan, max_lds_bytes, num_hbm_buffers;
    uint64_t graph_replays, graph_captures;
    uint64_t batch_launches;      /* multi-block launch groups issued by elemhip_process_blocks */
    uint64_t spec_launches;       /* launches of run-time specialised island kernels */
    uint32_t spec_shapes, spec_islands;   /* distinct specialised island shapes / islands they cover in the current plan */
    double   last_jit_wait_ms;    /* time the last commit waited for kernel compilation (option "specialize" = 2) */
    double   last_graph_capture_ms; /* hipGraph capture + instantiate of the current plan's per-block launch sequence */
    uint64_t resident_launches, resident_blocks;   /* option "resident": launches of the resident kernel / blocks it rendered */
    uint64_t fft_launches, fft_frames;             /* `fft` nodes: launches of the relay's transform kernel / frames they transformed */
} elemhip_stats;

/* Runtime(double sampleRate, int blockSize)                      runtime/elem/Runtime.h:44,157-166
 * blockSize is the MAX frames per process call (see "Block size" above). Returns NULL on failure; the reason is
 * available from elemhip_last_create_error(). */
elemhip_t* elemhip_create(double sampleRate, int blockSize, int deviceOrdinal);
void       elemhip_destroy(elemhip_t*);
int        elemhip_last_create_error(void);

/* int applyInstructions(js::Array const& batch)                  Runtime.h:48,170-218
 * `utf8_json` is the same JSON text the cli host hands to elem::js::parseJSON
 * (cli/Benchmark.cpp:40-43): [[0,id,"type"],[2,parent,child,outCh],[3,id,"key",value],[4,[roots]],[5]] */
int elemhip_apply_instructions_json(elemhip_t*, const char* utf8_json, size_t len);

/* Typed fast path for the same five instructions                 Runtime.h:123-126,293-433 */
int elemhip_create_node(elemhip_t*, int32_t id, const char* type);
int elemhip_append_child(elemhip_t*, int32_t parent, int32_t child, int32_t childOutputChannel);
int elemhip_set_property_json(elemhip_t*, int32_t id, const char* key, const char* json_value, size_t len);
int elemhip_activate_roots(elemhip_t*, const int32_t* ids, size_t n);
int elemhip_commit(elemhip_t*);

/* void process(const F** in, size_t nIn, F** out, size_t nOut, size_t numSamples, void* userData)
 *                                                                Runtime.h:51-57,274-290
 * Planar host buffers; outputs are overwritten. `sampleTime` is the one thing the reference's
 * hosts pass as userData (wasm/Main.cpp:206-215, consumed by wasm/SampleTime.h, wasm/Metro.h). */
int elemhip_process(elemhip_t*, const float* const* in, size_t nIn, float* const* out, size_t nOut,
                    size_t numSamples, int64_t sampleTime);

/* Offline rendering (js/packages/offline-renderer/index.ts:87-133 block loop): `numBlocks`
 * consecutive full blocks in one call, buffers resident in HBM.
 *   in_dev  : device pointer [numBlocks][nIn][blockSize] or NULL when nIn == 0
 *   out_dev : device pointer [numBlocks][nOut][blockSize], or NULL to render without copying out */
int elemhip_process_blocks(elemhip_t*, const float* in_dev, size_t nIn, float* out_dev, size_t nOut,
                           size_t numBlocks, int64_t sampleTime);

/* The same block loop over HOST buffers: what OfflineRenderer.process(inputs, outputs) does with the reference engine
 * (js/packages/offline-renderer/index.ts:87-133: ceil(numFrames / blockSize) FULL blocks, a short input tail zero-padded,
 * every block copied to the caller's arrays) and what a host gets from calling Runtime::process (Runtime.h:51-57) in a loop.
 *   in  : nIn planar channel arrays of numFrames frames each (caller-owned, pageable is fine), NULL when nIn == 0
 *   out : nOut planar channel arrays of numFrames frames each; overwritten
 * No HIP types cross the boundary. Launch sets of `batch_blocks` blocks go through pinned double buffers: the D2H of set k
 * and the H2D of set k + 1 run on a copy stream while set k + 1 renders, so the samples land in host memory at the
 * device-resident rate. `sampleTime` = sample time of the first frame (userData of the reference hosts). */
int elemhip_process_blocks_host(elemhip_t*, const float* const* in, size_t nIn, float* const* out, size_t nOut,
                                size_t numFrames, int64_t sampleTime);

/* EXTENSION (no counterpart in the reference): the same render delivered as interleaved PCM, packed on the GPU behind the last
 * render level of every launch set (elementary_amd/csrc/pcm_pack.hip; the arithmetic: pcm_pack.h). The nStreams * channels_per_stream
 * output channels leave as nStreams streams; sample (frame, g) of stream s is output channel s * channels_per_stream + g.
 *   format  1: little-endian int16   2: 3 bytes per sample, little-endian two's complement, packed   3: float32, bits unchanged
 *   dither  0: none   1: TPDF, 2 LSB peak to peak, keyed on `seed`, the channel and the ABSOLUTE frame time (sampleTime + frame):
 *           the bytes do not depend on how a render is cut into calls. Integer formats round to nearest even and clamp; a non-finite
 *           sample is delivered as 0 and counted.
 *   streams nStreams buffers of numFrames * channels_per_stream samples each; overwritten
 *   planar  NULL, or nStreams * channels_per_stream planar float arrays of numFrames frames: the very samples that were packed
 *   stats   NULL, or one per channel over the delivered frames: peak = max |x| of the finite samples, over = finite |x| > 1.0,
 *           nonfinite — the same in every format
 * Launch sets, double buffering and block-size rules are those of elemhip_process_blocks_host. Codes: 103 when nStreams *
 * channels_per_stream exceeds the output bus (1024), 8 for an unknown format, channels_per_stream == 0 or NULL streams / spec, 101 on
 * a dry handle. */
typedef struct elemhip_pcm_spec { uint32_t format, channels_per_stream, dither /*0 none, 1 TPDF*/, seed; } elemhip_pcm_spec;
typedef struct elemhip_pcm_channel_stats { float peak; uint32_t reserved; uint64_t over, nonfinite; } elemhip_pcm_channel_stats;
int elemhip_process_blocks_pcm(elemhip_t*, const float* const* in, size_t nIn,
                               void* const* streams, size_t nStreams,   /* nStreams buffers of numFrames * channels_per_stream samples */
                               float* const* planar,                    /* NULL, or nStreams*channels_per_stream planar float arrays: the very samples that were packed */
                               size_t numFrames, int64_t sampleTime, const elemhip_pcm_spec*, elemhip_pcm_channel_stats* stats /* NULL or one per channel */);

/* EXTENSION (no counterpart in the reference): the same render FED with interleaved PCM, unpacked on the GPU in front of the first
 * render level of every launch set (elementary_amd/csrc/pcm_unpack.hip; the arithmetic: pcm_unpack.h). The nInStreams *
 * channels_per_stream input channels arrive as nInStreams streams of numFrames * channels_per_stream samples; sample (frame, g) of
 * stream s is input channel s * channels_per_stream + g. The layout is that of the output streams above.
 *   format  1: little-endian int16, value * 2^-15   2: 3 bytes per sample, little-endian two's complement, packed, value * 2^-23
 *           3: float32, bits unchanged (NaN payloads and infinities included). Both integer conversions are exact in float32, and
 *           packing the result without dither gives the codes back.
 *   a short tail (numFrames no multiple of the block size) is zero-padded, as for planar input
 *   outSpec NULL: the output as planar floats only — `planar` = nPlanar arrays of numFrames frames, as elemhip_process_blocks_host
 *           fills them; outStreams / nOutStreams / stats are ignored
 *   outSpec set:  the delivery of elemhip_process_blocks_pcm — outStreams, nOutStreams, stats as there, `planar` NULL or nOutStreams *
 *           outSpec->channels_per_stream arrays that receive the very samples that were packed (nPlanar is ignored)
 * The floats a graph sees, and so every output sample, are bit for bit those of the planar entry points given the decoded input.
 * Codes: 8 for an unknown input (or output) format, channels_per_stream == 0, NULL streams / spec with nInStreams > 0; 103 when
 * nInStreams * channels_per_stream exceeds 32 host inputs or the output side exceeds the output bus (1024); 101 on a dry handle. A
 * failing call renders nothing. */
typedef struct elemhip_pcm_in_spec { uint32_t format, channels_per_stream; } elemhip_pcm_in_spec;
int elemhip_process_blocks_pcm_io(elemhip_t*, const void* const* inStreams, size_t nInStreams, const elemhip_pcm_in_spec* inSpec,
                                  void* const* outStreams, size_t nOutStreams, const elemhip_pcm_spec* outSpec, /* NULL: planar floats only */
                                  float* const* planar, size_t nPlanar,    /* with outSpec NULL: the nPlanar output channels */
                                  size_t numFrames, int64_t sampleTime, elemhip_pcm_channel_stats* stats);

/* EXTENSION (no counterpart in the reference): ITU-R BS.1770-4 / EBU R 128 metering of offline renders on the GPU
 * (elementary_amd/csrc/loudness.hip; the arithmetic: loudness.h). After elemhip_set_option(h, "loudness_meter", 1) every launch set of
 * elemhip_process_blocks_host, elemhip_process_blocks_pcm and elemhip_process_blocks_pcm_io is metered behind its last render level,
 * float or PCM delivery alike: per output channel the K-weighted mean square of every 100 ms sub-block (hop = round(sampleRate / 10)
 * frames) and the 4x-oversampled true peak. elemhip_process and the device-resident elemhip_process_blocks are NOT metered.
 * The programme is the frames those calls DELIVERED (numFrames each, not the zero padding of a last block), in call order, since the
 * option was turned on or elemhip_loudness_reset; its channel count is that of the first metered call (a call with another count
 * starts a new programme, and so does a metered call that fails). The state is carried on the device from set to set and call to call; a non-finite sample meters as 0.
 *   elemhip_loudness_read   info: channels, completed sub-blocks, hop, programme frames. meanSquares (NULL, or `capacity` doubles):
 *                           the series [channel][sub_blocks]; code 6 when capacity < channels * sub_blocks (info is filled: call
 *                           again). truePeak (NULL or one per channel): max |y| over the whole oversampled programme INCLUDING its
 *                           zero-padded tail, linear; the tail is evaluated on the host from a copy of the carried state, so a
 *                           programme may go on after a read. samplePeak (NULL or one per channel): max |x|. Codes: 101 on a dry
 *                           handle, 6 while the option is off.
 *   elemhip_loudness_reset  a new programme: time 0, zero filter state, no peaks
 *   elemhip_loudness_gate   pure host arithmetic, no handle: 400 ms blocks (4 sub-blocks, hop 1), block loudness -0.691 + 10 log10
 *                           sum_c weights[c] * ms_c (weights NULL: 1.0 each), absolute gate -70 LUFS, relative gate -10 LU under the
 *                           mean of the absolutely gated blocks. integrated is -inf when no block passes; momentary_max over the
 *                           400 ms blocks, short_term_max over windows of 30 sub-blocks (-inf when there is none). */
typedef struct elemhip_loudness_info { uint32_t channels, hop; uint64_t sub_blocks, frames; } elemhip_loudness_info;
typedef struct elemhip_loudness_result { double integrated, momentary_max, short_term_max; uint64_t blocks, gated_blocks; } elemhip_loudness_result;
int elemhip_loudness_read(elemhip_t*, elemhip_loudness_info* info, double* meanSquares, size_t capacity, double* truePeak, float* samplePeak);
int elemhip_loudness_reset(elemhip_t*);
int elemhip_loudness_gate(const double* meanSquares, size_t channels, size_t subBlocks, const double* weights, elemhip_loudness_result* out);

/* EXTENSION (no counterpart in the reference): delivery at another sample rate, converted on the GPU (elementary_amd/csrc/resample.hip;
 * the arithmetic: resample.h). After elemhip_set_option(h, "resample_rate", hz) — hz integral like the engine's rate; 0 or the engine's
 * own rate: off, the default — elemhip_process_blocks_host, elemhip_process_blocks_pcm and elemhip_process_blocks_pcm_io deliver the
 * render converted from the engine's rate fin to hz by a Kaiser-windowed sinc (32 zero crossings a side at the lower rate, pass band
 * +-0.001 dB to 0.9 of the lower Nyquist, -96 dB from 1.1 of it), behind every launch set's last render level: planar floats, packed
 * streams (the dither is keyed on the programme's OUTPUT frame index then, not on sampleTime) and what the loudness meter meters, whose
 * hop follows the delivery rate. numFrames stays the RENDERED count; the arrays and streams of such a call must hold
 * elemhip_resample_frames(numFrames) frames. With up / down = hz / fin in lowest terms, the programme — the frames those calls rendered,
 * in call order, since the option was set or elemhip_resample_reset — delivers exactly ceil(t * up / down) frames for its first t, so a
 * call that renders [t0, t1) delivers [ceil(t0 up / down), ceil(t1 up / down)): however a render is cut into calls and launch sets, the
 * same bytes. Output n is the render at time (n - latency_frames) * down / up; frames in front of the programme are silence.
 * elemhip_process and the device-resident elemhip_process_blocks are NOT converted. The programme's channel count is that of its first
 * call; a call with another count returns 6 (reset first); a call that fails starts a new programme. Code 6 for a rate without a plan:
 * not integral, up > 1024, more than 1024 taps (down / up > 16), or up / down > 8.
 *   elemhip_resample_frames  frames the next host-buffer call of numFrames will deliver (numFrames while the option is off)
 *   elemhip_resample_read    the plan and the programme's clock; code 6 while the option is off
 *   elemhip_resample_reset   a new programme: time 0, silence in front of it; code 6 while the option is off */
typedef struct elemhip_resample_info { uint32_t up, down, taps, latency_frames; uint64_t frames_in, frames_out; } elemhip_resample_info;
int elemhip_resample_frames(elemhip_t*, size_t numFrames, size_t* out);
int elemhip_resample_read(elemhip_t*, elemhip_resample_info* info);
int elemhip_resample_reset(elemhip_t*);

/* EXTENSION (no counterpart in the reference): inputs at another sample rate, converted on the GPU (elementary_amd/csrc/resample_in.hip;
 * the arithmetic: resample.h, the same prototype and tables as above with fin = hz and fout = the engine's rate). After
 * elemhip_set_option(h, "input_rate", hz) — hz integral; 0 or the engine's own rate: off, the default — the inputs of
 * elemhip_process_blocks_host, elemhip_process_blocks_pcm and elemhip_process_blocks_pcm_io, planar floats or interleaved PCM, arrive
 * at hz: a kernel in front of every launch set's first render level decodes and converts them where the host-to-device copy left
 * them, so only input-rate bytes cross the host link. numFrames stays in ENGINE frames; the input arrays and streams of such a call
 * must hold elemhip_input_resample_frames(numFrames) frames. The engine pulls: with up / down = engine rate / hz in lowest terms, a
 * call that renders the programme's engine frames [n0, n1) consumes the input frames [need(n0), need(n1)), need(0) = 0 and
 * need(n) = floor((n - 1) down / up) + 1 — however a render is cut into calls and launch sets, the same bits. Engine frame n is the
 * input at time (n - latency_frames) * down / up; frames in front of the programme are silence. The programme is the engine frames
 * those calls rendered with inputs, in call order, since the option was set or elemhip_input_resample_reset; its channel count is that
 * of its first call, a call with another count returns 6 (reset first), a call that fails starts a new programme. Code 6 for a rate
 * without a plan, and nothing changes: not integral, up > 1024, more than 1024 taps, up / down > 8 or down / up > 8. Independent of
 * "resample_rate", "limiter" and "loudness_meter": the frames delivered for a call are still elemhip_resample_frames(numFrames).
 * elemhip_process and the device-resident elemhip_process_blocks take their inputs at the engine's rate as before.
 *   elemhip_input_resample_frames  input frames the next host-buffer call of numFrames consumes (numFrames while the option is off)
 *   elemhip_input_resample_read    the plan and the programme's clock (latency_frames and frames_out in engine frames); code 6 while off
 *   elemhip_input_resample_reset   a new programme: time 0, silence in front of it; code 6 while the option is off */
int elemhip_input_resample_frames(elemhip_t*, size_t numFrames, size_t* out);
int elemhip_input_resample_read(elemhip_t*, elemhip_resample_info* info);
int elemhip_input_resample_reset(elemhip_t*);

/* EXTENSION (no counterpart in the reference): a static gain and a look-ahead true-peak limiter on the GPU (elementary_amd/csrc/limiter.hip;
 * the arithmetic: limiter.h). After elemhip_set_option(h, "limiter", 1) what elemhip_process_blocks_host, elemhip_process_blocks_pcm and
 * elemhip_process_blocks_pcm_io deliver — planar floats, packed streams, what the loudness meter meters — has passed, behind the
 * delivery-rate converter, through y[n] = g[n] G x[n - D - 6]: G = 10^(limiter_gain_db / 20), D = round(limiter_lookahead_ms * rate /
 * 1000) with 1 <= D <= 1024, and a gain g <= 1 per group of "limiter_link" consecutive channels (0: all) that holds the 4x-interpolated
 * peak of G x (the meter's interpolator) under C = 10^(limiter_ceiling_dbtp / 20): the reduction each peak asks for, held over D + 7
 * frames, released linearly in gain over limiter_release_ms for a full-scale reduction, smoothed by a mean over D + 1 frames. Frames
 * in = frames out; latency_frames = D + 6 frames of silence come first. The delivered SAMPLE peak stays under C; the metered true peak
 * of the output may exceed it slightly (the gain moves inside the interpolator's span: about 0.1 dB at D = 1, 0.004 dB at D = 66).
 * The programme — the frames those calls delivered, in call order, since the option was turned on, a parameter changed while it is on,
 * "resample_rate" was set or elemhip_limiter_reset — is limited the same however it is cut into calls and launch sets: the same bytes.
 * Its channel count is that of its first call and a multiple of limiter_link, else code 6; a call that fails starts a new programme.
 * Parameters (code 6 outside their range, or where they leave no plan at the delivery rate): limiter_ceiling_dbtp -40 .. 0 (-1),
 * limiter_gain_db -60 .. 60 (0), limiter_lookahead_ms (1.5), limiter_release_ms (500; at least one frame), limiter_link (0).
 *   elemhip_limiter_read   the plan and the programme's frame count; per group (`capacity` entries each, either may be null) the largest
 *                          reduction d behind a delivered gain (0 .. 1) and the frames with g < 1; code 6 while the option is off
 *   elemhip_limiter_reset  a new programme: frame 0, silence in front of it, statistics zero; code 6 while the option is off */
typedef struct elemhip_limiter_info { uint32_t lookahead_frames, latency_frames, release_frames, link, groups, reserved; uint64_t frames; } elemhip_limiter_info;
int elemhip_limiter_read(elemhip_t*, elemhip_limiter_info* info, double* maxReduction, uint64_t* limitedFrames, size_t capacity);
int elemhip_limiter_reset(elemhip_t*);

/* EXTENSION (no counterpart in the reference): noise-shaped requantisation on the GPU (elementary_amd/csrc/noise_shape.hip; the
 * arithmetic: noise_shape.h). With coefficients c_1 .. c_K set (1 <= K <= 12), the s16 / s24 codes that elemhip_process_blocks_pcm,
 * elemhip_process_blocks_pcm_io and elemhip_process_blocks_flac deliver come from an error-feedback quantiser behind the limiter, whose
 * requantisation error has the spectrum of plain TPDF dither times the noise transfer function 1 - sum c_k z^-k. The dither (the call's
 * dither flag and seed) is the pack kernel's, keyed on the absolute frame and the channel, at 8 fraction bits; without it the shaping is
 * deterministic and idle tones are possible. Coefficients are quantised once, cq_k = floor(c_k * 2048 + 0.5); code 6, and nothing
 * changes, for K > 12, a non-finite c_k or sum |cq_k| > 131071. Errors are clamped to 64 LSB, and every clamp is counted per channel.
 * count = 0, the default, turns it off: no launch, no buffer, not one byte differs. Float delivery is never touched; the statistics and
 * the loudness meter keep reading the floats. FLAC frames decode to the PCM path's codes and the STREAMINFO MD5 is that of its bytes, as
 * without shaping; a FLAC call's `drop` discards codes, not state.
 * The programme — the frames those calls quantised, in call order, since the coefficients were set or elemhip_noise_shape_reset — gives
 * the same bytes however it is cut into calls and launch sets. A call of another channel count, and a call that fails, start a new one.
 *   elemhip_noise_shape_read   taps (0: off), the programme's channels and frames; cq (the quantised coefficients) and saturated (the
 *                              clamps per channel), `capacity` entries each, either may be null
 *   elemhip_noise_shape_reset  a new programme: errors zero, counts zero
 *   elemhip_noise_shape_host   the scalar twin, without a handle: rows of `planar` (`stride` floats apart, row c = channel channel0 + c
 *                              of the dither's key) at absolute frame time0 -> codes (the same layout); state: null, or
 *                              channels * elemhip_noise_shape_state_bytes() bytes, in-out, zero at a programme's start
 *                              (int32 e[12], newest first; uint64 saturated; 8 bytes reserved) */
typedef struct elemhip_noise_shape_info { uint32_t taps, channels; uint64_t frames; } elemhip_noise_shape_info;
int elemhip_noise_shape_set(elemhip_t*, const float* coeffs, uint32_t count);
int elemhip_noise_shape_read(elemhip_t*, elemhip_noise_shape_info* info, int32_t* cq, uint64_t* saturated, size_t capacity);
int elemhip_noise_shape_reset(elemhip_t*);
size_t elemhip_noise_shape_state_bytes(void);
int elemhip_noise_shape_host(const float* coeffs, uint32_t count, uint32_t bits, int dither, uint32_t seed, uint32_t channel0, int64_t time0,
                             const float* planar, uint32_t channels, size_t stride, size_t frames, uint8_t* state, int32_t* codes);

/* EXTENSION (no counterpart in the reference): a spectrum analyser on what elemhip_process_blocks_host / _pcm / _pcm_io / _flac deliver,
 * on the GPU (elementary_amd/csrc/spectrum.hip; the arithmetic: spectrum.h) — behind the delivery-rate converter and the limiter, on the
 * floats the loudness meter reads, before any quantisation. Per channel, frame j covers the delivered programme frames
 * [j hop - P, j hop - P + size), zeros outside the programme: size 256, 512, 1024, 2048 or 4096, hop 1 .. size, P = size / 2 with
 * `center`, else 0. A sample times window[i] (`size` doubles, the caller's) is rounded once, in double; the real FFT runs in double;
 * the power is re^2 + im^2. bands = 0: size / 2 + 1 power columns per frame, rounded to float once. bands = 1 .. 512: band_first[b],
 * band_count[b] (0 allowed; first + count <= size / 2 + 1) and the rows' float weights behind one another in `weights`; a column is
 * the weighted sum of the row's bin powers, in double, in ascending bin order, rounded to float once. No logarithm is taken. The bits
 * do not depend on how the programme is cut into calls and launch sets. Code 6, and nothing changes, for a spec out of these ranges
 * (dry handles validate too); a NULL spec, the default, turns the analyser off: no launch, no buffer, not one byte differs.
 * A frame is emitted once its last sample was delivered: after n frames, elemhip_spectrum_frames(size, hop, center, n, 0) are out.
 * The programme is the frames those calls delivered since the spec was set, elemhip_spectrum_reset or a flush; a call of another
 * channel count, and a call that fails, start a new one; a new programme drops the frames nobody read.
 *   elemhip_spectrum_read    info: channels, columns, the spec, `queued` frames waiting from index first_frame on, the frames emitted
 *                            and the frames delivered so far. out (NULL: nothing is drained; else `capacity` floats, code 6 when too
 *                            few): [channel][queued][columns], and the queue is emptied. sums (NULL, or sumCapacity doubles):
 *                            [channel][columns], the float64 sum of every column over the frames emitted so far, in frame order —
 *                            the long-term average spectrum times `frames`. The programme is not disturbed.
 *   elemhip_spectrum_flush   pads with zeros and ends the programme: the total becomes elemhip_spectrum_frames(size, hop, center, n, 1)
 *                            — centred 1 + n / hop, else the least count that covers every sample; n = 0 emits nothing. The next
 *                            analysed call starts a new programme.
 *   elemhip_spectrum_reset   a new programme; what was pending is dropped
 *   elemhip_spectrum_host    the scalar twin on plain arrays, no handle: `planar` [channels] rows `stride` floats apart, `frames` frames
 *                            delivered behind programme frame n0; tail: [channels][size - 1] floats in-out (zero at a programme's
 *                            start); sums: [channels][columns] doubles in-out; frames [j0, j1) go to out [channels][j1 - j0][columns]
 *   elemhip_spectrum_launches  analyser kernels this process has launched so far */
typedef struct elemhip_spectrum_spec { uint32_t size, hop, center, bands; const double* window; const uint32_t* band_first; const uint32_t* band_count;
                                       const float* weights; } elemhip_spectrum_spec;
typedef struct elemhip_spectrum_info { uint32_t channels, columns, size, hop, center, bands, flushed, reserved;
                                       uint64_t first_frame, queued, frames, delivered; } elemhip_spectrum_info;
int elemhip_spectrum_set(elemhip_t*, const elemhip_spectrum_spec* spec);
int elemhip_spectrum_read(elemhip_t*, elemhip_spectrum_info* info, float* out, size_t capacity, double* sums, size_t sumCapacity);
int elemhip_spectrum_flush(elemhip_t*);
int elemhip_spectrum_reset(elemhip_t*);
uint64_t elemhip_spectrum_frames(uint32_t size, uint32_t hop, int center, uint64_t deliveredFrames, int flushed);
int elemhip_spectrum_host(const elemhip_spectrum_spec* spec, const float* planar, uint32_t channels, size_t stride, size_t frames, uint64_t n0,
                          uint64_t j0, uint64_t j1, float* tail, double* sums, float* out);
uint64_t elemhip_spectrum_launches(void);

/* EXTENSION (no counterpart in the reference): breakpoint automation for elemhip_process_blocks_host / _pcm / _pcm_io / _flac, expanded
 * on the GPU (elementary_amd/csrc/automation.hip; the arithmetic: automation.h). A lane is a list of points {frame, value, curve}
 * sorted by frame and bound to one engine input channel (0 .. 31); `el.in({channel})` reads it like any input. Only the points cross
 * the host link, once, when the lane is set: a kernel in front of every launch set's first level writes the channel's float32 rows
 * where the copy of a dense control signal would have put them, and no byte of a lane channel is staged or copied per call.
 * The value at ABSOLUTE engine frame t, with i the last point whose frame is <= t:
 *   t before the first point: the first value; i the last point: its value; curve 0 (hold), or t == frame_i: value_i bit for bit;
 *   curve 1 (linear): in double u = (double)(t - f_i) / (double)(f_{i+1} - f_i), y = a + (b - a) * u with the two values widened,
 *   these operations in this order, never fused, rounded once to float32.
 * Several points on one frame make a jump: the last of them is the value from that frame on, the first of them is what a ramp into
 * that frame aims at, any between the two have no effect.
 * Frame f of a call is evaluated at sampleTime + f, so a render does not depend on how it is cut into calls and launch sets and
 * nothing is carried; behind a call's last frame a lane channel is zero, as every input is. With option "input_rate" on, lanes are
 * not inputs at that rate: they are generated at the engine's rate and bypass the converter, and sampleTime keeps counting ENGINE
 * frames — frame f of a call of numFrames engine frames is evaluated at sampleTime + f, whatever the input frames it pulls.
 * Lane channels lie at or above the channels a call supplies (nIn, or nInStreams * channels_per_stream): a call that supplies a bound
 * channel answers 6 and renders nothing. The engine's input count for a call is max(supplied, highest lane + 1); a channel in between
 * that has no lane reads zeros, as a missing input does. Code 6, and nothing changes, for a lane that is unsorted, holds a non-finite
 * value or a curve other than 0 or 1, has more than 2^20 points or a linear segment longer than 2^52 frames, and for a channel
 * above 31 (dry handles validate and keep lanes too). With no lane set: no launch, no buffer, not one byte differs.
 * elemhip_process and the device-resident elemhip_process_blocks are not covered: they read the inputs they are given.
 *   elemhip_automation_set     binds a lane to `channel`, replacing the one it had; count 0 clears it
 *   elemhip_automation_read    info: lanes = bit mask of the bound channels, inputs = highest bound channel + 1 (0: none), count = the
 *                              points of `channel`'s lane; points (NULL, or `capacity` points, code 6 when too few) receives them
 *   elemhip_automation_reset   clears every lane
 *   elemhip_automation_host    the scalar twin, no handle: out[k] = the lane's value at t0 + k, k < n (code 6 for a lane that is refused)
 *   elemhip_automation_segment_at  the search a thread of the kernel does for its first frame: the index of the last point whose
 *                              frame is <= t, -1 before the first
 *   elemhip_automation_launches  automation kernels this process has launched so far */
typedef struct elemhip_automation_point { int64_t frame; float value; uint32_t curve; } elemhip_automation_point;
typedef struct elemhip_automation_info { uint32_t lanes, inputs; uint64_t count; } elemhip_automation_info;
int elemhip_automation_set(elemhip_t*, uint32_t channel, const elemhip_automation_point* points, size_t count);
int elemhip_automation_read(elemhip_t*, uint32_t channel, elemhip_automation_info* info, elemhip_automation_point* points, size_t capacity);
int elemhip_automation_reset(elemhip_t*);
int elemhip_automation_host(const elemhip_automation_point* points, size_t count, int64_t t0, size_t n, float* out);
int64_t elemhip_automation_segment_at(const elemhip_automation_point* points, size_t count, int64_t t);
uint64_t elemhip_automation_launches(void);

/* EXTENSION (no counterpart in the reference): the inspector — technical QC of what elemhip_process_blocks_host / _pcm / _pcm_io / _flac
 * deliver, on the GPU (elementary_amd/csrc/qc.hip; the definitions: qc.h) — behind the delivery-rate converter and the limiter, on the
 * floats the loudness meter reads, before any quantisation. It only reads. The programme is the frames those calls delivered since the
 * spec was set or elemhip_qc_reset, less the first `skip`, cut after `limit` frames (0: unbounded); a call of another channel count, and
 * a call that fails, start a new one. A non-finite sample is counted and then inspected as 0.0. A frame is quiet iff |x| <= silence_level
 * (>= 0; 0: exact digital silence) and clipped iff |x| >= clip_level (> 0). A clip event is a maximal run of at least clip_run (1 ..
 * 65535) clipped frames, the run at frame 0 and the open run at the end included; a dropout is a maximal run of at least dropout_frames
 * (1 .. 2^31 - 1) quiet frames with a non-quiet frame before AND after it. Of equally long runs the earliest is the longest; "none" is
 * UINT64_MAX. bucket (0: off; 16 .. 1048576): a min / max overview per `bucket` programme frames. pairs: up to 128 (a, b), a != b, whose
 * sum of x_a x_b is kept; a call that delivers fewer channels than a pair names is refused with code 6. The float64 sums are added in an
 * order that depends on programme frame indices alone (leaves of 64 frames in frame order, the leaves in leaf order): the same bits
 * however the render is cut into calls and launch sets; everything else is exact. Code 6, and nothing changes, for a spec out of these
 * ranges (dry handles validate too); a NULL spec, the default, turns the inspector off: no launch, no buffer, not one byte differs.
 *   elemhip_qc_read      info: channels, pairs, bucket, programme frames, frames delivered, and `queued` complete buckets waiting from
 *                        index first_bucket on. channels (NULL, or channelCapacity records): the cumulative results per channel, the
 *                        open bucket's partial min, max and frame count with them. pairSums (NULL, or pairCapacity doubles). The
 *                        programme is not disturbed.
 *   elemhip_qc_overview  drains the queued buckets: out [channel][queued][2] (min, max), `capacity` floats (code 6 when too few)
 *   elemhip_qc_reset     a new programme; buckets nobody read are dropped
 *   elemhip_qc_host      the scalar twin on plain arrays, no handle: `planar` [channels] rows `stride` floats apart, `frames` frames
 *                        behind programme frame p0; state: elemhip_qc_state_bytes(channels, num_pairs) bytes in-out (initialised here
 *                        where p0 = 0); reports [channels], pairSums [num_pairs] (either may be NULL); overview [channels][k][2] for the
 *                        k = (p0 + frames) / bucket - p0 / bucket buckets the frames complete. skip and limit are the caller's there.
 *   elemhip_qc_launches  inspector kernels this process has launched so far */
typedef struct elemhip_qc_spec { float silence_level, clip_level; uint32_t clip_run, dropout_frames, bucket, num_pairs; const uint32_t* pairs;
                                 uint64_t skip, limit; } elemhip_qc_spec;
typedef struct elemhip_qc_info { uint32_t channels, pairs, bucket, reserved; uint64_t frames, delivered, first_bucket, queued; } elemhip_qc_info;
typedef struct elemhip_qc_runs { uint64_t count, longest, longest_at, first_at; } elemhip_qc_runs;
typedef struct elemhip_qc_channel { uint64_t frames, nonfinite, quiet_frames, clipped_frames, peak_at, head_silence, tail_silence;
                                    elemhip_qc_runs dropouts, clip_events; double sum, sum_sq;
                                    float min, max, bucket_min, bucket_max; uint32_t bucket_frames, reserved; } elemhip_qc_channel;
int elemhip_qc_set(elemhip_t*, const elemhip_qc_spec* spec);
int elemhip_qc_read(elemhip_t*, elemhip_qc_info* info, elemhip_qc_channel* channels, size_t channelCapacity, double* pairSums, size_t pairCapacity);
int elemhip_qc_overview(elemhip_t*, float* out, size_t capacity);
int elemhip_qc_reset(elemhip_t*);
size_t elemhip_qc_state_bytes(uint32_t channels, uint32_t num_pairs);
int elemhip_qc_host(const elemhip_qc_spec* spec, const float* planar, uint32_t channels, size_t stride, size_t frames, uint64_t p0, uint8_t* state,
                    elemhip_qc_channel* reports, double* pairSums, float* overview);
uint64_t elemhip_qc_launches(void);

/* EXTENSION (no counterpart in the reference): the same render delivered as FLAC, encoded on the GPU in the pack kernel's place
 * (elementary_amd/csrc/flac_encode.hip; the arithmetic and the decision rules: flac_encode.h) — behind the delivery-rate converter and
 * the limiter, next to the meter. RFC 9639 "subset" streams of a fixed block size (option "flac_frame": 256, 512, 1024, 2048 or 4096,
 * the default) with 16 or 24 bits (spec.bits, or option "flac_bits" where that is 0) and 1 .. 8 channels per stream; nOutStreams *
 * channels_per_stream = the output channels, laid out as for elemhip_process_blocks_pcm. The sample values are exactly the s16 / s24
 * codes elemhip_process_blocks_pcm delivers for the same render, dither and seed: decoding the stream gives them back, sample for sample.
 * Subframes are CONSTANT, VERBATIM or FIXED of order 0 .. 4 with partitioned Rice residuals (escape partitions allowed), two-channel
 * streams choose per frame among independent, left/side, side/right and mid/side; every choice is made on exact bit counts, so no
 * subframe is longer than its VERBATIM form, and the bytes are the same on the GPU and in elemhip_flac_encode.
 * Option "flac_lpc_order" = P (integral, 0 .. 12; 0, the default: off, and then not one byte differs) adds LPC subframes: per subframe
 * the orders P and ceil(P / 2) (those below the block's samples) are priced to the bit next to the FIXED ones, from a Welch-windowed
 * integer autocorrelation and a Levinson-Durbin recursion whose arithmetic the kernel and elemhip_flac_encode_lpc share
 * (elementary_amd/csrc/flac_lpc.h); ties go to the simpler kind, LPC last. Like "flac_frame" the programme keeps the order it started
 * with: another value is refused (code 6) until elemhip_flac_reset; values that are not integral or outside 0 .. 12 are refused too.
 * The programme is the frames these calls delivered since creation or elemhip_flac_reset, in call order; FLAC frame j holds programme
 * frames [j F, (j + 1) F). A call returns the bytes of the FLAC frames it completed (bytesOut[s], possibly 0) and leaves the open
 * frame's codes on the device, so the bytes of a render do not depend on how it is cut into calls, relay windows or launch sets.
 * The inputs are those of elemhip_process_blocks_pcm_io (planar floats: format 3 with channels_per_stream 1). Every capacities[s] must
 * be at least elemhip_flac_bound(frames delivered, channels_per_stream, bits), else code 103. Codes: 8 for channels_per_stream 0 or
 * above 8, bits other than 16 / 24 or NULL buffers; 6 after elemhip_flac_flush, or where the call's shape (streams, channels, bits,
 * delivery rate) is not the open programme's; 101 on a dry handle. A call that fails starts a new programme.
 * spec.drop / spec.take: of the frames the call delivers, the first `drop` stay out of the programme and at most `take` enter it —
 * how a file leaves the converters' and the limiter's latency out, since frames cannot be cut on the host. The dither stays keyed on
 * the absolute frame, the statistics cover the frames that entered.
 *   elemhip_flac_flush   the open remainder as one final short frame per stream (none where nothing is open); the programme is closed:
 *                        further FLAC calls answer 6 until elemhip_flac_reset
 *   elemhip_flac_read    the programme: info, and per stream (capacity entries) the frames emitted, the samples they hold and the
 *                        smallest / largest frame in bytes — the STREAMINFO fields; frameBytes (NULL, or [stream][frameCap]): every
 *                        frame's byte length, what a SEEKTABLE would be built from (code 6 when frameCap is too small)
 *   elemhip_flac_reset   a new programme: nothing open, frame number 0
 *   elemhip_flac_encode  pure host arithmetic, no handle: planar int32 codes of one stream -> its frames, the scalar twin of the
 *                        kernels (whole frames; with `flush` the remainder as a short frame). Code 103 when `capacity` is too small,
 *                        6 for a code outside the sample size or a frame number above 2^31 - 1.
 *   elemhip_flac_encode_lpc  the same with an LPC order (0 .. 12, else code 6): the twin of a programme with option "flac_lpc_order"
 *   elemhip_flac_lpc_order   the open programme's LPC order, or the option's where none is open
 * A stream needs "fLaC" and a STREAMINFO block in front (elementary_amd/flac.py writes them). Its MD5 is left zero — "not computed":
 * the unencoded samples never reach the host — unless option "flac_md5" = 1 (integral, 0 or 1; 0, the default: no launch, no buffer,
 * not one byte differs): then every stream of a programme carries a running MD5 on the GPU (elementary_amd/csrc/flac_md5.hip, one wave
 * per stream behind the stage kernel of every launch set; the arithmetic: flac_md5.h) over exactly the bytes
 * elemhip_process_blocks_pcm would deliver for it in s16 / s24, and elemhip_flac_flush finalises it there: 16 bytes per stream come back,
 * no sample does. MD5 chains its 64-byte blocks, so one stream hashes at the speed of one wave, about 76 MB/s, on the render's own stream (profiles/r07/flac_md5.txt:
 * +14 ms on a 44 ms set of 128 mono streams, +7 ms on a 1.15 ms set of one stereo stream, where it is several times the render). Like "flac_frame" the programme keeps the value it
 * started with (code 6 until elemhip_flac_reset); a call that fails starts a new digest with the new programme.
 *   elemhip_flac_md5   state 0: the option is off in the programme, or there is none; 1: running, the digests all zero; 2: final, after
 *                      elemhip_flac_flush (a programme none of whose frames entered has the empty message's digest). digests (NULL, or
 *                      [streams][16] with room for `capacity` streams; code 6 when that is too small): what STREAMINFO's last 16 bytes hold
 *   elemhip_flac_md5_init / _update / _final / _record_bytes   pure host arithmetic, no handle: the digest of planar int32 codes of one
 *                      stream as the GPU computes it — for frame f, then channel, the low bits / 8 bytes of the code, little-endian. `record`:
 *                      elemhip_flac_md5_record_bytes() bytes of the caller's; _final leaves it as it is, so the updates may go on. */
typedef struct elemhip_flac_spec { uint32_t bits /* 16, 24; 0: option "flac_bits" */, channels_per_stream, dither /*0 none, 1 TPDF*/, seed;
                                   uint64_t drop, take; /* 0, UINT64_MAX: every delivered frame */ } elemhip_flac_spec;
typedef struct elemhip_flac_info { uint32_t flac_frame, bits, channels_per_stream, streams, sample_rate, flushed; uint64_t frames; } elemhip_flac_info;
typedef struct elemhip_flac_stream_info { uint64_t frames, total_samples; uint32_t min_frame_bytes, max_frame_bytes; } elemhip_flac_stream_info;
int elemhip_process_blocks_flac(elemhip_t*, const void* const* inStreams, size_t nInStreams, const elemhip_pcm_in_spec* inSpec,
                                void* const* outStreams, const size_t* capacities, size_t* bytesOut, size_t nOutStreams, const elemhip_flac_spec*,
                                size_t numFrames, int64_t sampleTime, elemhip_pcm_channel_stats* stats);
size_t elemhip_flac_bound(size_t frames, uint32_t channelsPerStream, uint32_t bits);
int elemhip_flac_flush(elemhip_t*, void* const* outStreams, const size_t* capacities, size_t* bytesOut, size_t nOutStreams);
int elemhip_flac_read(elemhip_t*, elemhip_flac_info* info, elemhip_flac_stream_info* perStream, size_t capacity, uint32_t* frameBytes, size_t frameCap);
int elemhip_flac_reset(elemhip_t*);
int elemhip_flac_encode(const int32_t* const* planar, uint32_t channels, size_t frames, uint32_t flacFrame, uint32_t bits, uint32_t sampleRate,
                        uint32_t firstFrameNumber, int flush, uint8_t* out, size_t capacity, size_t* bytesOut, uint32_t* frameBytes, size_t frameCap,
                        size_t* framesOut);
int elemhip_flac_encode_lpc(const int32_t* const* planar, uint32_t channels, size_t frames, uint32_t flacFrame, uint32_t bits, uint32_t sampleRate,
                            uint32_t firstFrameNumber, int flush, uint8_t* out, size_t capacity, size_t* bytesOut, uint32_t* frameBytes, size_t frameCap,
                            size_t* framesOut, uint32_t lpcOrder);
int elemhip_flac_lpc_order(elemhip_t*, uint32_t* order);
int elemhip_flac_md5(elemhip_t*, uint8_t* digests /*[streams][16]*/, size_t capacity, uint32_t* state);
size_t elemhip_flac_md5_record_bytes(void);
int elemhip_flac_md5_init(uint8_t* record);
int elemhip_flac_md5_update(uint8_t* record, const int32_t* const* planar, uint32_t channels, size_t frames, uint32_t bits /* 16, 24 */);
int elemhip_flac_md5_final(const uint8_t* record, uint8_t digest[16]);

/* EXTENSION (no counterpart in the reference): the same render FED with FLAC, decoded on the GPU in front of the unpack kernel (or
 * the input-rate converter) of every launch set (elementary_amd/csrc/flac_decode.hip; the arithmetic: flac_decode.h). Input format
 *   format  4: inStreams[s] points at an elemhip_flac_in — the stream's frames (the bytes behind its metadata blocks), the table
 *           elemhip_flac_index makes of them (frames + 1 entries: byte offset and first sample of every frame, one closing entry) and
 *           `position`, the stream sample at the call's first input frame. channels_per_stream has to be the streams' channel count,
 *           and all streams of a call have one sample size.
 * of elemhip_process_blocks_pcm_io and elemhip_process_blocks_flac. Only the frames that cover a launch set's input frames cross the
 * host link. A sample of `bits` <= 16 bits is worth code * 2^-(bits - 1), as the s16 sample code << (16 - bits) is; above 16 bits as
 * the s24 sample code << (24 - bits): the floats a graph sees are bit for bit those of the PCM input of the same samples, however the
 * render is cut into calls (a frame that straddles two launch sets or calls is decoded in both). Input frames past the table's
 * closing entry are silence; total_samples (the whole stream's length, where the table is a slice of it) is carried for the caller's
 * book-keeping and read by the engine for one thing only: with option "flac_in_md5" it is where the stream's digest ends (0: at the table's closing entry). With "input_rate" on a call pulls elemhip_input_resample_frames(numFrames) input frames from `position`.
 * What is read: fixed-block-size streams of 8 / 12 / 16 / 20 / 24 bits, 1 .. 8 channels, blocks of 16 .. 16384 samples (a shorter last
 * one), CONSTANT / VERBATIM / FIXED / LPC subframes, wasted bits, both residual coding methods with escapes, all channel assignments;
 * every frame's CRC-16 is verified on the GPU. Not read: variable block size, 32-bit samples, blocks above 16384.
 * STREAMINFO's MD5 — what catches a stream cut at a frame boundary, spliced, or re-encoded by a broken tool, which no CRC-16 does — is
 * computed on the GPU with option "flac_in_md5" = 1 (integral, 0 or 1; 0, the default: no launch, no buffer, not one byte differs; with
 * it on every rendered sample is still bit for bit what it is without: the stage only reads). Input stream s of a call is slot s. Behind
 * the decode kernels of every launch set one wave per stream (elementary_amd/csrc/flac_in_md5.hip; the arithmetic: flac_in_md5.h) takes
 * the samples the decoder restored — for stream sample t, then channel, the low (bits + 7) / 8 bytes of the code, little-endian, as
 * libFLAC hashes them — into the slot's running digest, every stream sample once: a set that decodes samples [c0, c1) hashes those from
 * the slot's `hashed` on, so the frame two sets decode enters once and feeding a completed stream again changes nothing. The launch that
 * hashes the stream's last sample (total_samples, or the table's closing entry where that is 0) finishes the digest; silence past the end is never hashed. A slot's state:
 * 0 off or never fed, 1 running, 2 complete, 3 broken until the reset — a gap (a render that starts behind sample 0, a seek forward), a
 * frame that answered 106, another total, sample size or channel count under a running slot. No decoded sample reaches the host, and the
 * set loop gains no synchronisation. Comparing the 16 bytes with what the file announces is the caller's (sixteen zeros there: "not computed").
 *   elemhip_flac_in_md5        waits for what is in flight; *slots: the slots fed since the reset; digests [slots][16] (zero unless
 *                              state 2), states and hashed (stream samples in the digest) [slots], each NULL or with room for `capacity`
 *                              slots (code 6 when that is too small)
 *   elemhip_flac_in_md5_reset  every slot back to state 0; so does another value of the option
 *   elemhip_flac_in_md5_update the handle-less twin, pure host arithmetic: planar int32 codes of 8 / 12 / 16 / 20 / 24 bits, 1 .. 8
 *                              channels into a record of elemhip_flac_md5_init / _final / _record_bytes (code 8 otherwise)
 * Codes: 8 for a NULL field, a sample size or channel count outside the above, or channels_per_stream unequal to a stream's channels;
 * 106 where a frame does not decode — elemhip_flac_in_error then names the first such (stream, frame index in the stream's table) and
 * the reason: 1 bad CRC, 2 reserved value, 3 bits missing, 4 non-zero padding, 5 sample out of range, 6 unsupported. A call that
 * answers 106 has delivered the launch sets in front of the failing one and renders nothing further; the engine stays usable.
 *   elemhip_flac_index   pure host arithmetic, no handle: a stream's frame bytes -> the table. *entries receives the entries the
 *                        stream needs (frames + 1); the tables are filled up to `capacity` entries — call again with more where it was
 *                        too small. blockSize 0: the first frame's. Code 106 where the bytes hold no frame this decoder reads.
 *   elemhip_flac_decode  pure host arithmetic, no handle: the scalar twin of the kernels — stream samples [position, position + count)
 *                        as planar int32 codes (zeros past the end). Code 106 with *badFrame / *reason on a frame that fails. */
typedef struct elemhip_flac_in { const uint8_t* data; uint64_t bytes; const uint64_t* frame_offsets; const uint64_t* frame_first_samples;
                                 uint64_t frames; uint32_t channels, bits; uint64_t total_samples, position; } elemhip_flac_in;
int elemhip_flac_index(const uint8_t* data, size_t bytes, uint32_t channels, uint32_t bits, uint32_t blockSize, uint64_t* frameOffsets,
                       uint64_t* frameFirstSamples, size_t capacity, size_t* entries);
int elemhip_flac_decode(const elemhip_flac_in* in, size_t count, int32_t* const* planar, size_t* badFrame, uint32_t* reason);
int elemhip_flac_in_error(elemhip_t*, uint32_t* stream, uint64_t* frame, uint32_t* reason);   /* of the last call that answered 106 (code 6: none) */
int elemhip_flac_in_md5(elemhip_t*, uint8_t* digests /*[slots][16]*/, uint32_t* states, uint64_t* hashed, size_t capacity, size_t* slots);
int elemhip_flac_in_md5_reset(elemhip_t*);
int elemhip_flac_in_md5_update(uint8_t* record, const int32_t* const* planar, uint32_t channels, size_t frames, uint32_t bits /* 8, 12, 16, 20, 24 */);

/* bool addSharedResource(name, unique_ptr<SharedResource>)       Runtime.h:83,461-465 (insert-only) */
int    elemhip_add_shared_resource(elemhip_t*, const char* name, const float* const* channels, size_t nCh, size_t nSamples);
/* EXTENSION (no counterpart in the reference): a shared resource from a file's own bytes, decoded — and, where the file's rate is not
 * the engine's, converted — on the GPU into the resource's device rows (elementary_amd/csrc/resource_load.hip; the arithmetic:
 * resource_load.h). The source is ONE interleaved stream of `channels` channels (1 .. 32) and `frames` frames:
 *   format 1 s16 / 2 packed s24 / 3 f32   `data` holds frames * channels samples (`bytes` of them at least), little-endian
 *   format 4 FLAC                         `flac` points at an elemhip_flac_in (what FLAC input reads, see above; 1 .. 8 channels): stream
 *                                         samples [position, position + frames), cut at the table's closing entry
 * sample_rate 0 or the engine's: channel g, frame f of the resource is the decoded sample (f, g) — the bits elemhip_add_shared_resource
 * leaves for the same floats. Another (integral) rate: the resource holds ceil(frames * L / M) frames (L / M = engine rate / file rate
 * in lowest terms) of the delivery converter's Kaiser-windowed sinc, CENTRED: frame 0 of the file lies at frame 0 of the resource, no
 * latency to take out; in front of and behind the file is silence. The bits do not depend on option "resource_load_frames" (the piece
 * of the file, in frames, that is staged at a time; 64 .. 2^24, default 2^20). The call does not hold process() up: the render lock
 * is taken only to insert the finished resource. Such a resource has no floats on the host until something needs them (convolve).
 * Returns 0 with *inserted = 1, or = 0 where the name is taken (insert-only, the old resource untouched), else
 *   8   a format outside 1 .. 4, 0 or more than 32 channels, a NULL field, fewer `bytes` than frames * channels samples, a malformed
 *       FLAC table
 *   6   a rate pair without a plan (L <= 1024, 2 * ceil(32 * max(1, M / L)) <= 1024 taps, L <= 8 M, both rates integral) or a
 *       resource of more than 2^31 - 1 frames
 *   106 a FLAC frame that does not decode (elemhip_flac_in_error names it, stream 0); nothing is inserted
 * With option "flac_in_md5" = 1 (see FLAC input above) a FLAC source is hashed by the same kernel under the same rule, on the loader's
 * stream behind the decode of every piece, with a record of the load's own: a load that decodes the stream from sample 0 to its end
 * leaves the digest of the FILE's samples with the resource (also where the resource is rate-converted), anything less leaves
 * "incomplete". The resource's floats do not depend on the option. Not done: resources added as floats are never converted.
 *   elemhip_shared_resource_md5    *state 0: not hashed (the option was off, or no FLAC source); 1: incomplete; 2: digest[16] is the
 *                                  STREAMINFO MD5 of the source's samples. Comparing it is the caller's; 6: no such name
 *   elemhip_shared_resource_info   channels and frames (of channel 0) of any resource; 6: no such name
 *   elemhip_shared_resource_read   frames [first, first + count) of `channel` as the nodes see them; a resource shorter than the engine's
 *                                  block can be read up to the block size (the device row's zero padding); 6: no such name, channel or range */
typedef struct elemhip_resource_src { uint32_t format, channels; double sample_rate; uint64_t frames; const void* data; uint64_t bytes;
                                      const elemhip_flac_in* flac; } elemhip_resource_src;
int    elemhip_add_shared_resource_pcm(elemhip_t*, const char* name, const elemhip_resource_src* src, int* inserted);
int    elemhip_shared_resource_info(elemhip_t*, const char* name, uint32_t* channels, uint64_t* frames);
int    elemhip_shared_resource_read(elemhip_t*, const char* name, uint32_t channel, uint64_t first, uint64_t count, float* out);
int    elemhip_shared_resource_md5(elemhip_t*, const char* name, uint8_t digest[16], uint32_t* state);
/* void pruneSharedResources()                                    Runtime.h:89,467-471 */
void   elemhip_prune_shared_resources(elemhip_t*);
/* std::set<NodeId> gc()                                          Runtime.h:76,220-272
 * Prunes every unreferenced node and returns how many; the first min(count, cap) ids (ascending) land in prunedOut.
 * When count > cap the full set of THAT pass can still be read with elemhip_last_gc (same ordering). */
size_t elemhip_gc(elemhip_t*, int32_t* prunedOut, size_t cap);
size_t elemhip_last_gc(elemhip_t*, int32_t* prunedOut, size_t cap);
/* void reset()                                                   Runtime.h:70,448-458 */
void   elemhip_reset(elemhip_t*);

/* int registerNodeType(std::string const& type, NodeFactoryFn&&)  Runtime.h:105-106,480-487 (code 4 when the name is taken)
 * A custom node type whose instances run ON THE CPU (the reference's GraphNode plug-in interface, GraphNode.h:19-96): the
 * engine renders everything upstream on the GPU, drains the stream, hands the node its input blocks on the host, calls
 * process() and uploads the output block — a call-out per node and block, slow by construction, kept so that hosts with
 * their own C++ nodes (wasm/Main.cpp:47-61 registers three this way) keep working. Plans containing such nodes render
 * block by block (no multi-block launches, no hipGraph replay).
 *   create       NodeFactoryFn(NodeId, sampleRate, blockSize)                          GraphNode.h:27
 *   set_property GraphNode::setProperty(key, js::Value) with the value as JSON text    GraphNode.h:49; return a ReturnCode
 *   process      GraphNode::process(BlockContext): planar inputs, ONE output channel   GraphNode.h:72, Types.h:91-101
 *                (`sample_time` is what the reference's hosts pass as userData, `active` = BlockContext::active)
 *   reset        GraphNode::reset                                                      GraphNode.h:86 (may be NULL) */
typedef struct elemhip_node_type {
    void* (*create)(int32_t node_id, double sample_rate, int block_size, void* user);
    void  (*destroy)(void* node, void* user);
    int   (*set_property)(void* node, const char* key, const char* json_value, void* user);
    void  (*process)(void* node, const float* const* in, size_t n_in, float* out, size_t num_samples, int64_t sample_time, int active, void* user);
    void  (*reset)(void* node, void* user);
    void* user;
} elemhip_node_type;
int elemhip_register_node_type(elemhip_t*, const char* type, const elemhip_node_type* vt);

/* js::Object snapshot()                                          Runtime.h:110,489-498
 * {"<8-digit hex node id>": {property: value, ...}, ...} as JSON text; returns the bytes needed (including the NUL). */
size_t elemhip_snapshot_json(elemhip_t*, char* buf, size_t cap);
/* SharedResourceMap::KeyViewType getSharedResourceMapKeys()      Runtime.h:94 — a JSON array of names */
size_t elemhip_shared_resource_keys_json(elemhip_t*, char* buf, size_t cap);

/* ReturnCode::describe                                           Types.h:62-85 */
const char* elemhip_describe(int code);
int  elemhip_get_stats(elemhip_t*, elemhip_stats* out);
/* Measurement hook: render `numBlocks` blocks (no host inputs) with a HIP event pair around every
 * kernel launch on the engine's stream. msOut[l] = mean ms of launch level l, msOut[levels] = the
 * epilogue kernel. Returns the number of entries written (levels + 1) or a negated error code. */
int  elemhip_time_launches(elemhip_t*, size_t nOut, size_t numBlocks, float* msOut, size_t cap);
/* Measurement hook for timed regions: after elemhip_set_option("profile_launches", 1) every multi-block launch that
 * elemhip_process_blocks issues is bracketed by a HIP event pair on the engine's stream. msOut[l] = summed ms of launch
 * level l, msOut[levels] = the epilogue kernel; *launchSets / *blocks = launch sets and blocks covered. Returns the number
 * of entries available (levels + 1). Setting the option to 1 again clears the sums. */
int  elemhip_get_launch_profile(elemhip_t*, double* msOut, size_t cap, uint64_t* launchSets, uint64_t* blocks);
/* Tracing hook: render one block while workgroup 0 of launch level `level` logs shader-clock
 * timestamps per task. out[wave*192 + 0..3] = {tasks, kernel start, prologue end, kernel end};
 * out[wave*192 + 3*(k+2) + 0..2] = {opcode | stage<<16 | flags<<24, start, end} for the wave's k-th task. */
/* void processQueuedEvents(std::function<void(std::string const&, js::Value)>&&)   runtime/elem/Runtime.h:64, 437-446
 * Non-render thread. Relays the newest readout of every `meter` / `snapshot` node (builtins/Analyzers.h) of the current
 * render sequence whose root is active: cb(type, JSON payload, user), e.g. ("meter", {"min":..,"max":..,"source":name|null}). */
typedef void (*elemhip_event_cb)(const char* type, const char* json_payload, void* user);
int  elemhip_process_queued_events(elemhip_t*, elemhip_event_cb cb, void* user);
/* The relay of a caller that renders many blocks per call and still wants what the reference's offline renderer delivers by
 * calling processQueuedEvents after EVERY block (js/packages/offline-renderer/index.ts:112-120): every block's events since the
 * last relay, in block order, nodes in render order inside a block — reconstructed from per-block readout logs the kernels keep
 * (builtins/Analyzers.h:23-62, 83-131: `meter` queues one readout per block, `snapshot` one per latch; a per-block relay hands on the
 * newest of each block). Exact while no more than elemhip_event_window_blocks() blocks pass between two relays (1024 for meter /
 * snapshot; less with a `scope` or an `fft` — their 8192-frame rings must not overrun inside a window: floor((8191 - size) / block)
 * blocks for a scope, floor((8192 - size) / block) for an fft, 1 when `size` is below the block — and 1 with a `capture` node, whose
 * take belongs to the block in which the gate fell). An `fft` node's frames are transformed on the GPU, all frames of a relay in one
 * launch on the relay's stream, and arrive as ("fft", {"source":name|null,"data":{"real":[size/2+1],"imag":[size/2+1]}}). Neither relay holds up a render thread: the readouts are snapshotted in stream order
 * and fetched on a stream of their own (runtime/elem/Runtime.h:437-446 drains lock-free queues). */
int  elemhip_process_queued_events_blockwise(elemhip_t*, elemhip_event_cb cb, void* user);
uint32_t elemhip_event_window_blocks(elemhip_t*);
/* elemhip_set_option(h, "event_history_blocks", W), W = 0 ... 1024 (clamped; 0 = off, the default): `scope` and `fft` nodes created
 * AFTERWARDS keep a device ring of bitceil(W * blockSize + 8192) frames per channel instead of 8192 (4 MB per channel at W = 1024 and
 * 512 frames), and the blockwise relay replays the reference ring's per-block reads and overrun nudges on the host: for such nodes
 * elemhip_event_window_blocks() is min(W, 1024 / slices per block) whatever their `size` — overruns included, the events are the
 * per-block relay's. Nodes that already exist keep their 8192-frame ring and the rule above; `capture` stays at 1.
 * elemhip_set_option(h, "capture_history_blocks", W), same range and default: `capture` and `mc.capture` nodes created AFTERWARDS keep
 * a device ring of bitceil(W * blockSize + bitceil(sampleRate)) frames per capture channel (4 MB at W = 1024, 512 frames and 48 kHz)
 * and a per-block log of the frames handed to the ring and of falling gate edges; the blockwise relay replays from it what a relay
 * after every block would have drained and emitted, and elemhip_event_window_blocks() is min(W, 1024 / slices per block) for them.
 * Nodes that already exist keep their ring of bitceil(sampleRate) frames and a window of 1. */

int  elemhip_trace_level(elemhip_t*, size_t nOut, uint32_t level, unsigned long long* out, size_t cap);
/* Debug/test hook: JSON description of the current render plan (islands, launch levels, LDS).
 * deviceOrdinal == -1 at create time gives a "dry" handle that runs all host logic (instruction
 * decode, graph mutation, plan build, gc) without a GPU; it cannot render (process returns 101). */
size_t elemhip_describe_plan(elemhip_t*, char* buf, size_t cap);
/* Debug/test hook: program text, compiler log and state (0 compiling, 1 ready, -1 failed) of the k-th specialised
 * island shape of the newest plan; returns the number of shapes or -1. */
int  elemhip_spec_info(elemhip_t*, size_t k, char* src, size_t srcCap, char* log, size_t logCap, int* state, uint32_t* islands);
/* Run the launches on a caller-owned hipStream_t (e.g. torch's current stream). */
int  elemhip_set_stream(elemhip_t*, void* hipStream);
/* Multi-GPU hosts: the path shards over independent units (voices, render jobs: SURVEY 8(e)) and its one exchange step is the sum
 * of the ranks' output buses. The reference has no counterpart (one thread, one bus: GraphRenderSequence.h:286-290 zeroes it,
 * every root adds into it). Once the ranks' buses sit on one device (hipMemcpyPeer, or ncclSend / ncclRecv — INTEGRATION.md
 * section 6) this adds them in the order given: dst = ((partials[0] + partials[1]) + partials[2]) + ... — the same bits on every
 * run, unlike a ring all-reduce. Device pointers, `nFloats` each; at most 64 partials; asynchronous on `hipStream` (NULL: the
 * null stream); no engine handle needed. */
int  elemhip_sum_buses(int deviceOrdinal, void* hipStream, float* dst, const float* const* partials, size_t nPartials, size_t nFloats);
/* Tunables (the full table with defaults: INTEGRATION.md section 5): "batch_blocks" (blocks per multi-block launch, 1 ... 1024),
 * "specialize" (0 interpreter kernels only, 1 per-island-shape kernels compiled in the background and used once ready, 2 commit
 * waits for them), "spec_blocks" / "host_out_direct" (elemhip_process through the specialised kernels / output written straight
 * into pinned host memory), "use_graph" / "graph_blocks" (per-block launch path replayed from a hipGraph), "stateless_rows",
 * "mixer_split", "pipeline_copies", "merge_phases", "pack_islands" / "pack_max" / "cu_count" (lane-packing of isomorphic
 * islands), "event_history_blocks" / "capture_history_blocks" (above, at elemhip_event_window_blocks), "loudness_meter" (above, at
 * elemhip_loudness_read), "resample_rate" (above, at elemhip_resample_frames), "input_rate" (above, at elemhip_input_resample_frames), "limiter" /
 * "limiter_*" (above, at elemhip_limiter_read), "profile_launches", "time_batch". Unknown keys return code 6. */
int  elemhip_set_option(elemhip_t*, const char* key, double value);

#ifdef __cplusplus
}
#endif
#endif /* ELEMHIP_H */
