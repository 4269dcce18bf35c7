// launch.h — host-callable launchers for the kernels in kernels.hip.
#pragma once
#include <hip/hip_runtime_api.h>
#include "device.h"
#include "pcm_pack.h"
#include "loudness.h"
#include "resample.h"
#include "limiter.h"
#include "flac_decode.h"
#include "flac_md5.h"
#include "flac_in_md5.h"
#include "noise_shape.h"
#include "spectrum.h"
#include "qc.h"
#include "automation.h"

namespace elemhip {

// Output bus channels per process call (the epilogue kernels' thread-per-channel tables; device.h's kMaxOut = 256 was the r01-r03
// limit and is still what the JIT-compiled island kernels see — they never look at it)
constexpr uint32_t kMaxOutBus = 1024;
constexpr uint32_t kEventLogEntries = 1024;   // per-block readout log of a meter / snapshot node (device.h EVT_LOG), a power of two

// ---- the resident form of the single-block path (resident.hip) ----
constexpr uint32_t kResidentQuit = 0xFFFFFFFFu;   // block number that asks the kernel to leave
constexpr uint32_t kResidentMaxLevels = 32;
constexpr uint32_t kResidentMaxRoots = 64;
struct ResidentCtl {              // mapped, coherent host memory; one cache line per direction
    uint32_t seq;                 // host -> device: number of the block to render next (1, 2, ...; kResidentQuit: leave)
    uint32_t pad0[15];
    uint32_t done;                // device -> host: number of the block whose output is in the host's output block
    uint32_t exited;              // device -> host: 0 running, 1 left (asked to, or idle), 2 a device-wide barrier timed out (block lost)
    uint32_t ticksBody, ticksEpilogue;   // of the last block: block number seen -> levels rendered -> output block written (10 ns units)
    uint32_t pad1[12];
};
struct ResidentLevels { uint32_t count; uint32_t offset[kResidentMaxLevels + 1]; };   // entries of PlanView::levelIslands per launch level
hipError_t configure_resident(uint32_t maxLdsBytes);
hipError_t launch_resident(hipStream_t s, const PlanView& pv, uint32_t* recs, float* hbm, Globals* g, const uint32_t* lcg,
                           const ResidentLevels& lv, uint32_t groups, uint32_t ldsBytes, ResidentCtl* ctlDev, const float* inHostDev,
                           float* outHostDev, unsigned long long* sync, uint64_t idleTicks, uint64_t hangTicks);

hipError_t configure_kernels(uint32_t maxLdsBytes);
void launch_level(hipStream_t s, const PlanView& pv, uint32_t* recs, float* hbm, const Globals* g, const uint32_t* lcg,
                  uint32_t levelBegin, uint32_t numIslands, uint32_t ldsBytes, uint32_t batch = 1, uint32_t arenaFloats = 0,
                  uint32_t statelessRows = 8);
// (`doneFlag`: a word in mapped host memory the epilogue of a ONE-block set publishes `doneValue` to behind its output, or null)
void launch_epilogue_batch(hipStream_t s, const PlanView& pv, uint32_t* recs, const float* hbm, Globals* g, float* outRing,
                           uint32_t batch, uint32_t arenaFloats, uint32_t* doneFlag = nullptr, uint32_t doneValue = 0u);
void launch_epilogue(hipStream_t s, const PlanView& pv, uint32_t* recs, const float* hbm, Globals* g, float* outRing,
                     uint32_t* doneFlag = nullptr, uint32_t doneValue = 0u);
hipError_t configure_kernels_rt(uint32_t maxLdsBytes);
void launch_level_rt(hipStream_t s, const PlanView& pv, uint32_t* recs, float* hbm, const Globals* g, const uint32_t* lcg,
                     uint32_t levelBegin, uint32_t numIslands, uint32_t ldsBytes);
void launch_convolve(hipStream_t s, const PlanView& pv, uint32_t* recs, float* hbm, const Globals* g,
                     uint32_t workBegin, uint32_t numWorkgroups);
size_t convolve_batch_scratch_floats(uint32_t maxBatch, uint32_t longHistRows);   // per convolve node (longHistRows: 0 = no long-partition area)
void launch_convolve_batch(hipStream_t s, const PlanView& pv, uint32_t* recs, float* hbm, const Globals* g, uint32_t workBegin,
                           uint32_t numNodes, uint32_t batch, uint32_t arenaFloats, float* scratch, uint32_t maxBatch, uint32_t macMode,
                           bool anyShortIr, bool anyLongIr, uint32_t longHistRows, bool anyShortPath, uint32_t longStateBlocks,
                           const float* inDirect, uint32_t numInCh, float* outDirect, uint32_t numOutCh);
void launch_convolve_fix_overlap(hipStream_t s, const PlanView& pv, uint32_t* recs, float* hbm, const Globals* g, uint32_t workBegin,
                                 uint32_t numWork, float* scratch, uint32_t maxBatch, uint32_t longHistRows, uint32_t maxPartitions);
uint32_t convolve_mfma_max_partitions();   // IRs of up to this many 512-tap partitions take the matrix-core MAC
uint32_t convolve_long_tap_group();        // long-partition IR spectra are allocated in multiples of this many rows
uint32_t convolve_long_row_floats();       // floats per long-partition spectrum row (4097 bins, padded)
hipError_t upload_convolve_tables(const float* twiddleReIm, const float* twiddle8192ReIm);
void launch_patches(hipStream_t s, const Patch* patches, uint32_t count, uint32_t* recs, uint32_t* globals);
// ---- the `fft` node's relay kernel (fft_frames.hip): one workgroup per frame ----
struct FftFrame {
    const float*  ring;        // the node's ring: mask + 1 floats
    const double* window;      // Blackman-Harris table of `size` doubles
    const double* twiddles;    // exp(-2 pi i q / size), q < size, as (re, im) pairs
    float*        out;         // receives real[size/2 + 1] | imag[size/2 + 1]
    uint32_t      read;        // ring position of the frame's first sample
    uint32_t      size;        // 256, 512, 1024, 2048 or 4096
    uint32_t      mask;        // ring frames - 1 (8191, or the history ring of "event_history_blocks")
    uint32_t      pad_;
};
// `maxSize`: the largest `size` among the frames — the launch's LDS is sized by it
hipError_t launch_fft_frames(hipStream_t s, const FftFrame* framesDev, uint32_t count, uint32_t maxSize);
// ---- PCM delivery (pcm_pack.hip): one workgroup per tile of (block, stream), pcm_pack.h ----
struct PcmPackArgs {
    const float*    src;            // the set's output, [block][numChannels][blockSize]
    unsigned char*  dst;            // [stream] at `streamStride` bytes (a multiple of 16; the base 16-byte aligned): validFrames * G samples each
    pcm_pack::ChannelStats* stats;  // [numStreams * G], added into
    const uint16_t* rowBase;        // pcm_pack_row_table(G) on the device
    int64_t         time0;          // sample time of the set's first frame (the dither's key)
    uint64_t        streamStride;
    uint32_t        blockSize, numChannels, G, numStreams, validFrames, tilesPerBlock, rowDwords, dither, seed;
    const int32_t*  shaped;         // null, or the set's codes where its floats lie in `src` (noise_shape.hip): taken in place of quantising
};
uint32_t pcm_pack_row_table(uint32_t G, uint16_t* out);      // out[G]; returns PcmPackArgs::rowDwords
hipError_t launch_pcm_pack(hipStream_t s, const PcmPackArgs& a, uint32_t format);
// ---- PCM input (pcm_unpack.hip): the inverse, one workgroup per tile of (block, stream), pcm_unpack.h ----
struct PcmUnpackArgs {
    const unsigned char* src;       // [stream] at `streamStride` bytes (a multiple of 16; the base 16-byte aligned): validFrames * G samples each
    float*          dst;            // the set's input, [numBlocks][numChannels][blockSize]: rows s * G + g of every block are written whole
    const uint16_t* rowBase;        // pcm_pack_row_table(G) on the device
    uint64_t        streamStride;
    uint32_t        blockSize, numChannels, G, numStreams, validFrames, numBlocks, tilesPerBlock, rowDwords;   // frames behind validFrames: zero
};
hipError_t launch_pcm_unpack(hipStream_t s, const PcmUnpackArgs& a, uint32_t format);
// ---- breakpoint automation (automation.hip): in front of a launch set's first level, next to the unpack kernel, automation.h ----
struct AutomationArgs {
    float*          dst;            // the set's input, [block][numChannels][blockSize]: rows of channels [firstChannel, numChannels) are written
    const automation::Point* points;        // every lane's points behind one another (device)
    uint64_t        numPoints;
    int64_t         time0;          // the absolute engine frame of the set's first frame
    uint64_t        validFrames;    // frames of the set inside the call: zeros behind them
    uint32_t        blockSize, numChannels, firstChannel, numBlocks;
    uint32_t        offset[automation::kMaxChannels], count[automation::kMaxChannels];      // per channel: its lane's points (count 0: no lane, zeros)
};
hipError_t launch_automation(hipStream_t s, const AutomationArgs& a);
uint64_t automation_launches();     // kernels launched by this process so far
// ---- loudness meter (loudness.hip): behind a launch set's last level, loudness.h ----
struct LoudnessArgs {
    const float*    src;            // the set's output, [block][numChannels][blockSize]
    loudness::ChannelState* state;  // [numChannels], carried from set to set
    double*         segState;       // [numChannels][segCap][4]: pass one's end states, then the scan's start states
    double*         segEnergy;      // [numChannels][segCap][2]: pass two's sums
    double*         out;            // [numChannels][outStride]: the sums of the sub-blocks this set completed
    uint32_t        blockSize, numChannels, validFrames, numSegs, segCap, outStride;
    uint32_t        q0;             // the programme's frame count at the set's start, mod hop
    loudness::Plan  plan;
};
hipError_t launch_loudness(hipStream_t s, const LoudnessArgs& a);
// ---- spectrum analyser (spectrum.hip): behind a launch set's last level, next to the meter, spectrum.h ----
struct SpectrumArgs {
    const float*    src;            // the set's output, [block][numChannels][blockSize] (not read where validFrames = 0: a flush)
    const float*    tailIn;         // [numChannels][size - 1]: the programme's frames in front of the set, oldest first
    float*          tailOut;        // the other copy: receives the frames in front of the NEXT set (updateTail)
    float*          out;            // [numChannels][numFrames][cols]: the frames this set completes
    double*         sums;           // [numChannels][cols]: the running sums, added into in frame order
    uint64_t        n0, j0;         // the programme's delivered frames and emitted frames at the set's start
    uint32_t        numFrames, validFrames, blockSize, numChannels, updateTail;
    spectrum::Plan  plan;           // (device pointers)
};
hipError_t launch_spectrum(hipStream_t s, const SpectrumArgs& a);
uint64_t spectrum_launches();       // kernels launched by this process so far
// ---- inspector (qc.hip): behind a launch set's last level, next to the meter and the analyser, qc.h ----
struct QcArgs {
    const float*    src;            // the set's output, [block][numChannels][blockSize]; frames [q0, q0 + count) enter the programme
    qc::ChannelState* state;        // [numChannels]: the programme so far, carried on the device
    qc::PairState*  pairState;      // [numPairs]
    const uint32_t* pairs;          // [numPairs][2]: the channels of every pair
    qc::Stretch<uint32_t>* tileStretch;     // scratch [numChannels][tileCap]: the tiles' summaries
    double*         leafSums;       // scratch [2 numChannels + numPairs][leafCap]: the leaves' sums of x and x^2 per channel, x_a x_b per pair
    float*          tileEdge;       // scratch [numChannels][tileCap][4]: min, max of a tile's lead and trail piece of the overview
    float*          out;            // [numChannels][outCount][2]: the buckets this set completes
    uint64_t        p0;             // programme frames in front of the set
    uint32_t        q0, count, blockSize, numChannels, numPairs, numTiles, tileCap, leafCap, outCount;
    qc::Spec        spec;
};
hipError_t launch_qc(hipStream_t s, const QcArgs& a);
uint64_t qc_launches();             // kernels launched by this process so far
// ---- delivery-rate conversion (resample.hip): behind a launch set's last level, in front of the pack kernel and the meter, resample.h ----
struct ResampleArgs {
    const float*    src;            // the set's output, [block][numChannels][blockSize]: validIn frames at the engine's rate
    float*          dst;            // [outBlocks][numChannels][blockSize]: validOut frames at the delivery rate, zeros up to the last block's end
    const float*    histIn;         // [numChannels][plan.H]: the programme's frames in front of the set, oldest first
    float*          histOut;        // the other copy: receives the frames in front of the NEXT set
    const float*    table;          // resample::make_tables: [plan.T][plan.L]
    const int32_t*  rowBase;        // [plan.L]
    uint64_t        t0, n0;         // the programme's input / output frame index at the set's start
    uint32_t        blockSize, numChannels, validIn, validOut, outBlocks, outBlocksCap;
    resample::Plan  plan;
};
hipError_t launch_resample(hipStream_t s, const ResampleArgs& a);
// ---- input-rate conversion (resample_in.hip): in front of a launch set's first level, in the unpack kernel's place, resample.h ----
struct ResampleInArgs {
    const unsigned char* src;       // [stream] at `streamStride` bytes (a multiple of 16; the base 16-byte aligned): validIn * G samples each,
                                    // the programme's input frames [t0, t0 + validIn)
    float*          dst;            // the set's input, [numBlocks][numChannels][blockSize]: rows s * G + g of every block are written whole —
                                    // validOut frames at the engine's rate, zeros up to the last block's end
    const float*    histIn;         // [numStreams * G][plan.H]: the decoded input frames in front of t0, oldest first
    float*          histOut;        // the other copy: receives the frames in front of the NEXT set's stretch
    const float*    table;          // resample::make_tables: [plan.T][plan.L]
    const int32_t*  rowBase;        // [plan.L]
    uint64_t        t0, n0;         // the programme's input / engine frame index at the set's start: t0 = inputs_before(n0)
    uint64_t        streamStride;
    uint32_t        blockSize, numChannels, G, numStreams, validIn, validOut, numBlocks, pad;
    resample::Plan  plan;           // fin = the input's rate, fout = the engine's
};
hipError_t launch_resample_in(hipStream_t s, const ResampleInArgs& a, uint32_t format);
// ---- true-peak limiter (limiter.hip): behind the converter, in front of the pack kernel and the meter, limiter.h ----
struct LimiterArgs {
    const float*    src;            // the set's delivered frames, [block][numChannels][blockSize]: validFrames of them
    float*          dst;            // [outBlocks][numChannels][blockSize]: the limited frames, zeros up to the last block's end
    const unsigned char* stateIn;   // limiter::state_bytes: M | d | frames in front of the set
    unsigned char*  stateOut;       // the other copy: receives the state in front of the NEXT set
    limiter::GroupStats* stats;     // [groups], accumulated over the programme
    double*         frames;         // [groups][frameCap] scratch: dm, then d
    double*         tiles;          // [groups][tileCap] scratch: the tiles' maxima, then M in front of each tile
    uint64_t        n0;             // the programme's frame index at the set's start
    uint32_t        blockSize, numChannels, validFrames, outBlocks, outBlocksCap, frameCap, tileCap, pad;
    limiter::Plan   plan;
    loudness::Plan  meter;          // the delivery rate's: its interpolator is the detector
};
hipError_t launch_limiter(hipStream_t s, const LimiterArgs& a);
// ---- FLAC delivery (flac_encode.hip): behind the converter and the limiter, in the pack kernel's place, flac_encode.h ----
struct FlacStageArgs {
    const float*    src;            // the set's delivered frames, [block][numChannels][blockSize]: validFrames of them from srcOffset on
    const int32_t*  carry;          // [numChannels][flacFrame]: the open frame's codes, `open` of them
    int32_t*        codes;          // [numChannels][cap]: receives the carried codes, then the set's
    pcm_pack::ChannelStats* stats;  // [numChannels], added into
    int64_t         time0;          // sample time of frame 0 of `src` (the dither's key)
    uint32_t        blockSize, numChannels, validFrames, open, cap, bits, dither, seed;
    uint32_t        srcOffset;      // frames of `src` in front of the validFrames that stay out of the programme
    const int32_t*  shaped;         // null, or the set's codes where its floats lie in `src` (noise_shape.hip): taken in place of quantising
};
hipError_t launch_flac_stage(hipStream_t s, const FlacStageArgs& a);
// the codes behind the last whole frame become the next set's carry
hipError_t launch_flac_carry(hipStream_t s, const int32_t* codes, int32_t* carry, uint32_t numChannels, uint32_t cap, uint32_t flacFrame, uint32_t from, uint32_t count);
struct FlacEncodeArgs {
    const int32_t*  codes;          // [numStreams * G][cap]
    uint32_t*       slots;          // [numStreams][numFrames][candidates][slotWords]: the candidates' subframes, bit 0 = the top of word 0
    uint32_t*       subBits;        // [numStreams][numFrames][candidates]
    unsigned char*  dst;            // [stream] at `streamStride` bytes (a multiple of 16; the base 16-byte aligned): the frames back to back
    uint32_t*       frameBytes;     // [numStreams][numFrames]
    uint64_t        streamStride;
    uint32_t        cap, G, numStreams, bits, flacFrame, n /* samples of every frame: flacFrame, or the flushed remainder */, numFrames, slotWords, rate, firstNumber;
    uint32_t        lpcOrder;       // flac_lpc.h: 0 (no LPC candidates) .. 12
};
hipError_t launch_flac_encode(hipStream_t s, const FlacEncodeArgs& a);      // the encode kernel, then the assemble kernel
// ---- the STREAMINFO MD5 of FLAC delivery (flac_md5.hip): behind the stage kernel, flac_md5.h ----
struct FlacMd5Args {
    const int32_t*  codes;          // [numStreams * G][cap]: frames [first, first + count) of every channel enter their stream's digest
    flac_md5::Record* records;      // [numStreams], carried from launch to launch
    uint8_t*        digests;        // [numStreams][16], 4-byte aligned: written with `finish`
    uint32_t        cap, G, numStreams, bits, first, count, finish /* pad, append the bit length, write the digests */, pad;
};
hipError_t launch_flac_md5(hipStream_t s, const FlacMd5Args& a);
// ---- noise-shaped requantisation (noise_shape.hip): behind the limiter, in front of the pack kernel or the FLAC stage kernel, noise_shape.h ----
struct NoiseShapeArgs {
    const float*    src;            // the set's delivered frames, [block][numChannels][blockSize]: validFrames of them
    int32_t*        dst;            // the same shape: the code of a sample lies where its float lies
    noise_shape::ChannelState* state;   // [numChannels], carried from set to set, updated in place
    int64_t         time0;          // sample time of frame 0 of `src` (the dither's key)
    uint32_t        blockSize, numChannels, validFrames, bits, dither, seed, taps, pad;
    int32_t         cq[noise_shape::kMaxTaps];
};
hipError_t launch_noise_shape(hipStream_t s, const NoiseShapeArgs& a);
// ---- FLAC input (flac_decode.hip): in front of the unpack kernel or the input-rate converter, flac_decode.h ----
using FlacInFrame = flac_decode::FrameRec;
using FlacInStream = flac_decode::StreamRec;
using FlacInError = flac_decode::ErrorRec;
struct FlacDecodeArgs {
    const unsigned char* staged;    // the covering frames' bytes
    const FlacInFrame*  frames;
    const FlacInStream* streams;
    void*           subs;           // [numFrames][G] flac_decode::Sub
    uint32_t*       state;          // [numFrames]: reason | channel assignment << 8
    int32_t*        scratch;
    FlacInError*    error;          // zeroed in front of the launch
    unsigned char*  dst;            // [stream] at `streamStride` bytes (a multiple of 16; the base 16-byte aligned): valid * G samples each
    uint64_t        streamStride;
    uint32_t        numFrames, numStreams, G, bits, valid, pad;
};
// (the host's copies of the two tables are checked against the buffers' sizes before anything is launched)
hipError_t launch_flac_decode(hipStream_t s, const FlacDecodeArgs& a, const FlacInFrame* hostFrames, const FlacInStream* hostStreams,
                              size_t stagedBytes, size_t scratchInts);
// ---- the STREAMINFO MD5 of FLAC inputs and resources (flac_in_md5.hip): behind the decode kernels, flac_in_md5.h ----
struct FlacInMd5Args {
    const int32_t*  scratch;        // the decoder's: the restored samples of the set's covered frames
    flac_md5::Record* records;      // [numStreams], carried from launch to launch
    uint8_t*        digests;        // [numStreams][16], 4-byte aligned: a stream's written with its job's `finish`
    const flac_in_md5::Job* jobs;   // [numStreams], 16-byte aligned, staged with the set
    uint32_t        numStreams, G, bits, pad;
};
hipError_t launch_flac_in_md5(hipStream_t s, const FlacInMd5Args& a, const flac_in_md5::Job* hostJobs, size_t scratchInts);
// ---- resource loader (resource_load.hip): a staged piece of a source file into the resource's planar rows, resource_load.h ----
struct ResourceLoadArgs {
    const unsigned char* src;       // the staged piece, 16-byte aligned, `srcBytes` (whole 16-byte lines): sample (f, g) of its frame f lies at
                                    // head + (f * G + g) * sample bytes — source frames [in0, in0 + validIn) of the file's totalIn
    float*          rows[32];       // the resource's channel rows, `rowFloats` floats each, zeroed before the first piece
    const uint16_t* rowTable;       // pcm_pack_row_table(G) on the device (copy)
    const float*    table;          // resample::make_tables: [plan.T][plan.L] (convert)
    const int32_t*  rowBase;        // [plan.L] (convert)
    uint64_t        in0, out0;      // the piece's first staged source frame / first written resource frame
    uint64_t        totalIn, srcBytes, rowFloats;
    uint32_t        G, head, validIn, validOut, rowDwords, pad;
    resample::Plan  plan;           // fin = the file's rate, fout = the engine's (convert)
};
hipError_t launch_resource_copy(hipStream_t s, const ResourceLoadArgs& a, uint32_t format);         // the file's rate is the engine's
hipError_t launch_resource_convert(hipStream_t s, const ResourceLoadArgs& a, uint32_t format);
hipError_t launch_bus_sum(hipStream_t s, float* dst, const float* const* partials, uint32_t count, size_t n);   // dst = ((p0 + p1) + p2) + ... (rank order)

} // namespace elemhip
