// engine.h — host side of the HIP block-render engine.
//
// `Engine` re-creates the behaviour of `elem::Runtime<float>` (runtime/elem/Runtime.h:39-153) on
// top of device-resident node records and compiled render plans:
//   applyInstructions  -> Engine::apply        (Runtime.h:170-218)
//   process            -> Engine::process      (Runtime.h:274-290)
//   gc / reset / shared resources              (Runtime.h:220-272, 448-477)
// The render sequence the reference builds as a list of closures (Runtime.h:520-577,
// GraphRenderSequence.h:107-187) becomes a `Plan`: islands of nodes rendered by one workgroup
// each, grouped into launch levels (plan.cpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <deque>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "device.h"
#include "json.h"
#include "jit.h"
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

// Return codes 0..8 are the reference's (runtime/elem/Types.h:51-86); >= 100 are ours.
enum ReturnCode : int {
    kOk = 0, kUnknownNodeType = 1, kNodeNotFound = 2, kNodeAlreadyExists = 3, kNodeTypeAlreadyExists = 4,
    kInvalidPropertyType = 5, kInvalidPropertyValue = 6, kInvariantViolation = 7, kInvalidInstructionFormat = 8,
    kHipError = 100, kNoDevice = 101, kBlockTooLarge = 102, kTooManyChannels = 103, kUnsupportedGraph = 104,
    kJsonParseError = 105, kFlacInput = 106,
};
const char* describe(int code);
using FlacInFrame = flac_decode::FrameRec;
using FlacInStream = flac_decode::StreamRec;
using FlacInError = flac_decode::ErrorRec;

// Host call-out node types (Runtime::registerNodeType, runtime/elem/Runtime.h:105-106; GraphNode.h:19-96): a node whose
// process() runs on the CPU between two launch levels. OP_HOST never reaches a kernel, so it is not a device opcode.
constexpr uint16_t OP_HOST = 0x7F00;
struct HostVTable {
    void* (*create)(int32_t nodeId, double sampleRate, int blockSize, void* user) = nullptr;
    void  (*destroy)(void* node, void* user) = nullptr;
    int   (*setProperty)(void* node, const char* key, const char* jsonValue, void* user) = nullptr;
    void  (*process)(void* node, const float* const* in, size_t nIn, float* out, size_t numSamples, int64_t sampleTime, int active, void* user) = nullptr;
    void  (*reset)(void* node, void* user) = nullptr;
    void* user = nullptr;
};

struct DevBuf {
    void* ptr = nullptr;
    size_t bytes = 0;
};

// Shared resource = immutable float channel arrays (SharedResource.h:15-24, AudioBufferResource.h),
// mirrored into device memory on first use.
struct Resource {
    std::vector<std::vector<float>> channels;
    DevBuf dev;                 // channel 0, uploaded lazily
    std::vector<DevBuf> devCh;  // channels >= 1 (multi-output nodes), uploaded lazily; devCh[0] unused
    bool isTap = false;         // created by getTapResource (mutable feedback buffer)
    // made on the device from a file's bytes (Engine::addSharedResourcePcm, resource_load.h): every channel's row is in `dev` / `devCh`
    // already, and `channels` stays empty until something needs the floats on the host (Engine::resourceHost fetches them once)
    bool onDevice = false;
    uint32_t deviceChannels = 0;
    uint64_t deviceFrames = 0;
    // a FLAC source loaded under option "flac_in_md5": 0 — not hashed; 1 — the load did not cover the stream from sample 0 to its end;
    // 2 — `md5` holds the digest of the file's samples
    uint32_t md5State = 0;
    uint8_t md5[16] = {};
    size_t numChannels() const { return onDevice ? deviceChannels : channels.size(); }
    size_t frames(size_t ch) const { return onDevice ? (ch < deviceChannels ? (size_t)deviceFrames : 0) : (ch < channels.size() ? channels[ch].size() : 0); }
};
using ResourcePtr = std::shared_ptr<Resource>;

struct Node;
// (`src` / `srcEpoch`: the planner's memo of nodes.find(source) — valid while Engine::nodesEpoch, which every erase from the node
//  table bumps, equals srcEpoch; node addresses are stable under insertion)
struct Inlet  { int32_t source; uint32_t channel; mutable Node* src = nullptr; mutable uint32_t srcEpoch = 0; };
struct Outlet { int32_t dest; uint32_t channel; };

struct Node {
    int32_t id = 0;
    uint32_t planVisited = 0, planOnStack = 0;   // plan-build scratch (PlanBuilder::traverse, plan.cpp): epoch marks instead of hash sets
    int32_t planIdx = -1;                        // ... planner entry of output channel 0 in the build whose epoch is planVisited
    uint32_t planChans = 0;                      // ... and how many channel entries follow it
    uint16_t op = OP_INVALID;
    uint32_t rec = kNone;
    std::vector<Inlet> inlets;
    std::vector<Outlet> outlets;
    std::map<std::string, Value> props;
    // RootNode / GainFade host mirror (helpers/GainFade.h): the device advances the same floats
    float gain = 0.0f, target = 1.0f, step = 0.0f, inStep = 0.0f, outStep = 0.0f;
    int channel = -1;
    // device-side resources owned by the node
    DevBuf ring;                // delay / sdelay ring, tapOut private buffer, seq data
    ResourcePtr res;            // tap buffer / sample data held by the node
    uint32_t eventCount = 0;    // meter / snapshot: readouts already relayed by processQueuedEvents
    uint32_t logRelayed = 0;    // snapshot: entries of the per-block readout log already relayed
    // scope / fft: the reference's ring positions as the last relay left them (event_replay.h: frames written, read position) — a
    // blockwise relay replays the window's per-block reads from here; frames of the device ring per channel; the relay window
    // (host blocks) the ring was sized for by option "event_history_blocks" when the node was made (0: the plain 8192-frame ring)
    uint64_t ringWritten = 0;
    uint32_t ringRead = 0, ringFrames = 8192, historyBlocks = 0;
    // capture / mc.capture: the relay window (host blocks) the ring was sized for by option "capture_history_blocks" when the node was
    // made (0: the reference's bitceil(sr) frames, no per-block log; then ringFrames is that ring) and the absolute count of recorded
    // frames the relay has drained so far (capture_replay.h; the device counts them in CAP_ABS). logRelayed: blocks of the log relayed.
    uint32_t captureHistoryBlocks = 0;
    uint64_t capRelayed = 0;
    uint32_t convSlices = 1;    // convolve: helper slices its current impulse response wants (conv.hip)
    uint32_t convQp = 0, convHistBlocks = 0, convP = 0;   // convolve: long-partition tap rows (0: none), blocks of its input ring, 512-partitions (conv_long.inc)
    bool mc = false;            // multi-output node (mc.*): one record per output channel, planned as one entry per channel
    std::vector<uint32_t> chanRecs;   // records of output channels 1, 2, ... (allocated when a plan first needs them)
    std::vector<std::vector<float>> relayCh;   // mc.capture: one relay per capture channel (pendingEventData, mc/Capture.h:152)
    std::vector<float> relay;   // OP_CAPTURE: samples drained from the device ring, waiting for the gate's falling edge (Capture.h:102)
    void* hostInst = nullptr;   // OP_HOST: the instance its type's create() returned
    const HostVTable* hostVt = nullptr;
};

struct Plan;   // plan.cpp

// Generated text of one island-program signature (codegen.cpp) and, once computed, its kernel cache key (jit.cpp). Shared by
// Engine::specTextCache and the plans being built; the key is written under the control lock.
struct SpecText {
    std::string text;
    std::string key;          // empty until buildPlan first needs it
    uint32_t keyLdsWords = 0; // the LDS footprint the key was computed for
};

// One island's scheduled program as the planner left it (plan_island.cpp "island program cache"): an island whose nodes, edges,
// arena positions and options are unchanged at the next build takes these instead of being scheduled again.
// Table buffers of retired plans, kept for the next plan (a live graph re-plans dozens of times a second; hipMalloc / hipFree
// cost more than the upload, and hipFree synchronises the device). A buffer comes back when its plan dies, which is after the
// synchronize that follows the plan's last launch (Engine::freeDeferred) or before any launch (a pending plan replaced).
struct TablePool {
    std::mutex m;
    std::vector<DevBuf> free;
    DevBuf take(size_t bytes);           // a pooled buffer of at least `bytes` (not more than 4x), or a fresh allocation; ptr null = out of memory
    void give(DevBuf b);
    ~TablePool();
};

// Device home of the island programs. Blobs are appended and never rewritten, so a re-plan uploads only the programs of the
// islands it had to schedule (the replaced voice) while kernels of the current plan keep reading their own blobs; unchanged
// islands are referenced where they already sit. Replaced islands leave garbage behind: when the heap runs out the engine
// starts a fresh one and forgets the cache (plans keep the heap they point into alive).
struct ProgHeap {
    uint32_t* dev = nullptr;             // null on a dry engine (offsets are still handed out)
    size_t capDwords = 0, usedDwords = 0;
    ~ProgHeap();
};

struct IslandProgram {
    Island I;                            // progBegin / rootRec are re-made per plan
    std::vector<uint32_t> blob;          // host copy of the program (16-byte padded): describePlan, plan_cache = 2
    std::vector<uint32_t> members;       // (node id, opcode, record, arena buffer) of every member in render order: checked on a cache hit (the key is a hash)
    // relocation (plan_island.cpp, "same structure, other nodes"): the records and arena buffers the program names, in the order a canonical
    // walk of the island meets them, and the first stream buffer it was given — an island of the same STRUCTURE (another voice of
    // the patch) takes this program with the i-th record / buffer replaced by its own i-th
    std::vector<uint32_t> canonRecs, canonHbms;
    uint32_t streamStart = 0;
    uint32_t specHbmTab = 0;             // entries of the specialised variant's arena table (behind the record table; its operand table follows)
    uint64_t shapeKey = 0;
    std::shared_ptr<ProgHeap> heap;      // where the device copy lives ...
    uint32_t heapBegin = 0;              // ... as a dword offset (= Island::progBegin of every plan that uses it)
    std::shared_ptr<SpecText> spec;      // specialised-kernel text of its shape (null: none)
    uint32_t numMembers = 0, numOperands = 0, streamDelta = 0;
};

struct Stats {
    uint64_t blocksRendered = 0;
    uint64_t plansBuilt = 0;
    double   lastPlanBuildMs = 0.0;
    uint32_t numIslands = 0, numLevels = 0, numTasks = 0, numNodesInPlan = 0, maxLdsBytes = 0, numHbmBuffers = 0;
    uint64_t graphReplays = 0, graphCaptures = 0, batchLaunches = 0;
    uint64_t specFadeBlocks = 0;         // blocks rendered by the specialised kernels while root fades were running (per-block epilogue)
    uint64_t idleLaunchesSkipped = 0;    // launches left out because no root of their islands ran
    uint64_t progHeaps = 0;              // program heaps started (1 = the first still serves)
    uint64_t planIslandsReused = 0, planIslandsScheduled = 0, planCacheMismatches = 0;   // island program cache (plan.cpp)
    uint64_t planIslandsRelocated = 0, planRelocationMismatches = 0;                      // ... programs taken from a structural twin
    uint64_t specLaunches = 0;             // launches of run-time specialised island kernels
    uint32_t specShapes = 0, specIslands = 0;
    double   lastJitWaitMs = 0.0;
    double   lastGraphCaptureMs = 0.0;     // capture + instantiate of the per-block hipGraph of the current plan
    uint64_t residentLaunches = 0, residentBlocks = 0;   // option "resident": launches of the resident kernel / blocks it rendered
};

struct ResidentCtl;     // launch.h
struct RenderGuard;     // engine_impl.h
struct RelayCtx;        // engine_relay.cpp

class Engine {
    friend struct RenderGuard;
public:
    Engine(double sampleRate, int blockSize, int device);
    ~Engine();
    int initError() const { return initErr; }

    int apply(const Value& batch);
    int createNode(int32_t id, const std::string& type);
    int appendChild(int32_t parent, int32_t child, int32_t channel);
    int setProperty(int32_t id, const std::string& key, const Value& v);
    int activateRoots(const std::vector<int32_t>& ids, bool malformedTail = false);
    int commit(std::unique_lock<std::mutex>& renderLock);

    // one block, host buffers (Runtime::process)
    int process(const float* const* in, size_t nIn, float* const* out, size_t nOut, size_t n, int64_t sampleTime);
    int processSlice(const float* const* in, size_t nIn, float* const* out, size_t nOut, size_t n, int64_t sampleTime);
    int processSliceLocked(const float* const* in, size_t nIn, float* const* out, size_t nOut, size_t n, int64_t sampleTime, bool adopt);   // n <= blockSize
    // numBlocks consecutive full blocks, device-resident output `outDev[block][nOut][blockSize]`
    // (may be null: render only) and optional device-resident input `inDev[block][nIn][blockSize]`
    int processBlocks(const float* inDev, size_t nIn, float* outDev, size_t nOut, size_t numBlocks, int64_t sampleTime);
    // the same for HOST buffers, planar like Runtime::process (Runtime.h:51-57) over `numFrames` = any number of frames: the
    // offline caller's block loop (offline-renderer/index.ts:87-133) in one call. Renders ceil(numFrames / blockSize) full
    // blocks (a short tail of the inputs is zero-padded, the outputs receive numFrames frames). Launch sets are staged
    // through pinned double buffers: the D2H of set k and the H2D of set k + 1 run on a copy stream while set k + 1 renders.
    int processBlocksHost(const float* const* in, size_t nIn, float* const* out, size_t nOut, size_t numFrames, int64_t sampleTime);
    // The same render delivered as PCM (pcm_pack.h): `nStreams` streams of `spec.channelsPerStream` interleaved channels each — stream s,
    // sample (frame, g) = output channel s * G + g — as int16, packed 24-bit or float32, numFrames * G samples per stream. Behind the
    // last render level of every launch set a pack kernel (pcm_pack.hip) converts the set's output block where it lies in HBM; one
    // D2H per set brings the packed streams and the per-channel statistics to a pinned half, one contiguous memcpy per stream puts
    // them into the caller's buffers while the next set renders. `planar` (may be null): nStreams * G planar float arrays that receive
    // the very samples that were packed — the float copy and scatter of processBlocksHost run only then. `stats` (may be null): one
    // per channel, over the delivered frames of this call. Where processBlocksHost renders host block by host block through process()
    // (taps under a sliced host block, ragged slices) the floats are on the host already and are packed there by the header's scalar
    // loop: the same functions, the same bits.
    struct PcmSpec { uint32_t format, channelsPerStream, dither, seed; };
    struct PcmChannelStats { float peak; uint32_t reserved; uint64_t over, nonfinite; };
    int processBlocksPcm(const float* const* in, size_t nIn, void* const* streams, size_t nStreams, float* const* planar,
                         size_t numFrames, int64_t sampleTime, const PcmSpec& spec, PcmChannelStats* stats);
    // Both deliveries fed with PCM (pcm_unpack.h): the nIn = src.nStreams * src.channelsPerStream input channels arrive as interleaved
    // streams of numFrames * G samples — stream s, sample (frame, g) = input channel s * G + g — int16, packed 24-bit or float32. Per
    // launch set one contiguous memcpy per stream fills a pinned packed half, one H2D brings it over and an unpack kernel
    // (pcm_unpack.hip) converts and de-interleaves it into the set's input block where the render kernels read it; a short tail is
    // zero there as it is for planar input. `outSpec` null: the `nPlanar` output channels as planar floats (processBlocksHost);
    // else processBlocksPcm's delivery, `planar` (may be null) nOutStreams * G arrays. Where the block-by-block path renders, the
    // header's scalar loop unpacks on the host: the same floats.
    struct PcmSource { uint32_t format, channelsPerStream; const void* const* streams; size_t nStreams; };
    int processBlocksPcmIo(const PcmSource& src, void* const* outStreams, size_t nOutStreams, const PcmSpec* outSpec, float* const* planar,
                           size_t nPlanar, size_t numFrames, int64_t sampleTime, PcmChannelStats* stats);
    // The FLAC form of a PcmSource (format flac_decode::kFormat = 4): streams[s] points at a FlacIn — the stream's frames, the table
    // flac_decode::index_host makes of them, and `position`, the stream sample at the call's first input frame. Decoded on the GPU
    // into the packed input half (flac_decode.hip); where the block-by-block path renders, decode_host decodes on the host.
    // A frame that does not decode ends the call with kFlacInput; flacInError names it.
    struct FlacIn { const uint8_t* data; uint64_t bytes; const uint64_t* frameOffsets; const uint64_t* frameFirstSamples; uint64_t frames;
                    uint32_t channels, bits; uint64_t totalSamples, position; };
    int flacInError(uint32_t* stream, uint64_t* frame, uint32_t* reason);
    // Option "flac_in_md5" (flac_in_md5.h; 0, the default: off — no launch, no buffer, not one byte differs; 1): input stream s of a call is
    // slot s, and the samples the decoder restores enter the slot's running MD5 on the device (flac_in_md5.hip) behind the decode kernels
    // of every set — each stream sample once, also where two sets decode the same FLAC frame. A slot's state: 0 off or never fed, 1 running,
    // 2 complete (the digest of the whole stream, finished by the launch that hashed its last sample), 3 broken (a gap, a frame that did not
    // decode, another stream under a running slot) until the reset. The stage only reads: no rendered sample depends on it.
    // flacInMd5Read waits for what is in flight; digests [slots][16] (zero unless state 2), states and hashed [slots]; capacity in slots.
    int flacInMd5Read(uint8_t* digests, uint32_t* states, uint64_t* hashed, size_t capacity, size_t* slots);
    int flacInMd5Reset();
    // the digest a FLAC resource's load left (option "flac_in_md5" at the time): state as Resource::md5State
    int sharedResourceMd5(const std::string& name, uint8_t digest[16], uint32_t* state);
    // Option "loudness_meter" (loudness.h): every launch set of processBlocksHost / processBlocksPcm / processBlocksPcmIo is metered
    // where its output lies in HBM (loudness.hip), float or PCM delivery alike; where those calls render host block by host block the
    // header's scalar loop meters the floats on the host. process() and the device-resident processBlocks() are NOT metered. The
    // programme is the frames those calls delivered, in call order, since the last reset; its channel count is that of the first
    // metered call (a call with another count starts a new programme).
    struct LoudnessInfo { uint32_t channels, hop; uint64_t subBlocks, frames; };
    // meanSquares: [channel][subBlocks] (capacity in doubles; too small: the info is filled and kInvalidPropertyValue returned);
    // truePeak (zero-padded tail included, the carried state is not disturbed) / samplePeak: one per channel; any pointer may be null
    int loudnessRead(LoudnessInfo* info, double* meanSquares, size_t capacity, double* truePeak, float* samplePeak);
    int loudnessReset();
    // Option "resample_rate" (resample.h; 0 or the engine's own rate: off): the frames processBlocksHost / processBlocksPcm /
    // processBlocksPcmIo deliver — planar floats, packed streams, what the meter meters — are the render converted to that rate behind
    // every launch set's last level (resample.hip); where those calls render host block by host block the header's scalar loop converts
    // the floats on the host. `numFrames` stays the RENDERED count; the arrays and streams receive resampleFrames(numFrames) frames.
    // process() and the device-resident processBlocks() are NOT resampled. The programme is the frames those calls rendered, in call
    // order, since the option was set or the last reset; its clock lives on the host, the last H input frames of every channel on
    // the device. Its channel count is that of the first call: a call with another count is refused (reset first). A call that
    // fails starts a new programme.
    struct ResampleInfo { uint32_t up, down, taps, latencyFrames; uint64_t framesIn, framesOut; };
    int resampleFrames(size_t numFrames, size_t* out);       // frames the next host-buffer call of numFrames delivers (off: numFrames)
    int resampleRead(ResampleInfo* info);
    int resampleReset();
    // Option "input_rate" (resample.h, the input side; 0 or the engine's own rate: off): the inputs of processBlocksHost /
    // processBlocksPcm / processBlocksPcmIo arrive at that rate — planar floats or interleaved PCM — and a kernel in front of every
    // launch set's first level (resample_in.hip) decodes and converts them to the engine's rate where the H2D left them; where those
    // calls render host block by host block the header's scalar loop converts on the host, the same bits. `numFrames` stays in ENGINE
    // frames; the input arrays and streams hold inputResampleFrames(numFrames) frames. The programme is the engine frames those calls
    // rendered with inputs, in call order, since the option was set or the last reset; its clock lives on the host, the last H decoded
    // input frames of every channel on the device. Its channel count is that of the first call: a call with another count is refused
    // (reset first). A call that fails starts a new programme. Independent of "resample_rate", "limiter" and "loudness_meter".
    int inputResampleFrames(size_t numFrames, size_t* out);  // input frames the next host-buffer call of numFrames consumes (off: numFrames)
    int inputResampleRead(ResampleInfo* info);               // (latencyFrames in engine frames, framesOut = engine frames)
    int inputResampleReset();
    // Options "limiter" and "limiter_*" (limiter.h; off by default): a static gain and a look-ahead true-peak limiter on what the
    // host-buffer render calls deliver, behind the converter and in front of the pack kernel and the meter (limiter.hip; the header's
    // scalar loop where those calls render host block by host block). Frames in = frames out, delayed by latencyFrames. The programme
    // is the frames those calls delivered since the option was turned on, a parameter changed or the last reset; its channel count is
    // that of the first call (a multiple of `link`): a call with another count is refused. A call that fails starts a new programme.
    struct LimiterInfo { uint32_t lookaheadFrames, latencyFrames, releaseFrames, link, groups; uint64_t frames; };
    // maxReduction[group] (the largest d behind a delivered gain, 0 .. 1) / limitedFrames[group] (frames with g < 1): `capacity` entries each
    int limiterRead(LimiterInfo* info, double* maxReduction, uint64_t* limitedFrames, size_t capacity);
    int limiterReset();
    // Noise-shaped requantisation (noise_shape.h; off by default: no launch, no buffer, not one byte differs): with `count` = 1 .. 12
    // coefficients set, the s16 / s24 codes of processBlocksPcm / PcmIo / Flac come from an error-feedback quantiser with the noise
    // transfer function 1 - sum c_k z^-k, behind the limiter and in front of the pack kernel or the FLAC stage kernel (noise_shape.hip;
    // the header's scalar loop where those calls render host block by host block). Float delivery launches nothing. The programme is
    // the frames those calls quantised since the coefficients were set or the last reset; a call of another channel count, and a call
    // that fails, start a new one. A set that is refused (noise_shape::quantise_coeffs) changes nothing; count 0 turns it off.
    struct NoiseShapeInfo { uint32_t taps, channels; uint64_t frames; };
    int noiseShapeSet(const float* coeffs, uint32_t count);
    // cq: the quantised coefficients, saturated[channel]: the error clamps so far; `capacity` entries each (either may be null)
    int noiseShapeRead(NoiseShapeInfo* info, int32_t* cq, uint64_t* saturated, size_t capacity);
    int noiseShapeReset();
    int noiseShapeAfter(int rc);      // behind a packed delivery call: a call that failed, wherever it did, starts a new programme; returns rc
    // Spectrum analyser (spectrum.h; off by default: no launch, no buffer, not one byte differs): with a spec set, what processBlocksHost /
    // Pcm / PcmIo / Flac deliver — behind the converter and the limiter, the floats the meter reads, before any quantisation — is framed
    // per channel (frame j = programme frames [j hop - P, j hop - P + size), P = size / 2 when centred, zeros outside the programme),
    // windowed and transformed behind every launch set's last level (spectrum.hip; the header's scalar twin where those calls render
    // host block by host block) into power spectra (size / 2 + 1 columns) or band sums (`bands` rows of first bin, count and `count`
    // float weights, the weights of all rows behind one another). Frames leave when their last sample was delivered and queue up on the
    // host until spectrumRead drains them; spectrumFlush pads with zeros and ends the programme: the next analysed call starts a new
    // one, as do spectrumReset, a call with another channel count and a call that fails — and a new programme drops what was not read.
    // A null spec turns the analyser off. A spec that is refused (spectrum::spec_ok) changes nothing.
    struct SpectrumSpec { uint32_t size, hop, center, bands; const double* window; const uint32_t* bandFirst; const uint32_t* bandCount; const float* weights; };
    struct SpectrumInfo { uint32_t channels, columns, size, hop, center, bands, flushed, reserved; uint64_t firstFrame, queued, frames, delivered; };
    int spectrumSet(const SpectrumSpec* spec);
    // info.queued frames from info.firstFrame on wait in the queue. `out` (null: nothing is drained), `capacity` floats: receives
    // [channel][queued][columns] and the queue is emptied (too small: kInvalidPropertyValue, nothing drained). `sums` (null, or
    // `sumCapacity` doubles): [channel][columns], the running sums over every frame emitted so far. The programme is not disturbed.
    int spectrumRead(SpectrumInfo* info, float* out, size_t capacity, double* sums, size_t sumCapacity);
    int spectrumFlush();
    int spectrumReset();
    // Inspector (qc.h; off by default: no launch, no buffer, not one byte differs): with a spec set, what processBlocksHost / Pcm / PcmIo /
    // Flac deliver — behind the converter and the limiter, the floats the meter reads, before any quantisation — is inspected per
    // channel behind every launch set's last level (qc.hip; the header's scalar twin where those calls render host block by host
    // block): quiet and clipped frames and their runs (head and tail silence, dropouts, clip events), non-finite samples, min, max and
    // the first peak, the float64 sums of x and x^2 and of x_a x_b for up to 128 channel pairs, and with `bucket` a min / max overview.
    // The programme is the delivered frames since the spec was set or qcReset, less the first `skip`, cut after `limit` (0: unbounded);
    // a call of another channel count, and a call that fails, start a new one. It only reads. A null spec turns it off. A spec that is
    // refused (qc::spec_ok; a pair of one channel twice) changes nothing; a call that delivers fewer channels than a pair names is
    // refused with kInvalidPropertyValue.
    struct QcSpec { float silenceLevel, clipLevel; uint32_t clipRun, dropoutFrames, bucket, numPairs; const uint32_t* pairs; uint64_t skip, limit; };
    struct QcInfo { uint32_t channels, pairs, bucket, reserved; uint64_t frames, delivered, firstBucket, queued; };
    int qcSet(const QcSpec* spec);
    // `channels` (null, or room for channelCap reports) and `pairSums` (null, or pairCap doubles): the cumulative results; the open
    // bucket's partial comes with the channel. The programme is not disturbed. info.queued complete buckets from info.firstBucket on wait.
    int qcRead(QcInfo* info, qc::ChannelReport* channels, size_t channelCap, double* pairSums, size_t pairCap);
    int qcOverview(float* out, size_t capacity);      // drains the queue: [channel][queued][2] (min, max); too small: kInvalidPropertyValue
    int qcReset();
    // Breakpoint automation (automation.h; no lane set: no launch, no buffer, not one byte differs): a lane — a sorted list of
    // {frame, value, hold | linear} points — bound to engine input channel `channel` (0 .. 31) feeds that channel of processBlocksHost /
    // Pcm / PcmIo / Flac with the lane's value at the ABSOLUTE engine frame sampleTime + f for frame f of the call, zeros behind the call's
    // last frame like every input. The points cross the host link once, when the lane is set; a kernel in front of every launch set's
    // first level (automation.hip, next to the unpack kernel) writes the channel's rows of the set's input, and where those calls
    // render host block by host block the header's scalar twin fills them: the same floats. Lane channels lie at or above the channels
    // a call supplies — a call that supplies a bound channel is refused (kInvalidPropertyValue, nothing rendered); the engine's input
    // count for a call is max(supplied, highest lane + 1), and a channel in between that has no lane reads zeros. With option
    // "input_rate" on, lanes are not inputs at that rate: they bypass the converter and frame f of a call of numFrames ENGINE frames is
    // still evaluated at sampleTime + f, sampleTime counting engine frames. A lane that is refused (automation::lane_ok: unsorted, a
    // non-finite value, an unknown curve, more than 2^20 points, a linear segment longer than 2^52 frames) changes nothing. process()
    // and the device-resident processBlocks() do not know lanes. Works on a dry handle too (the tables stay on the host).
    struct AutomationInfo { uint32_t lanes, inputs; uint64_t count; };      // mask of bound channels, highest bound channel + 1, this lane's points
    int automationSet(uint32_t channel, const automation::Point* points, size_t count);      // count 0 clears the lane
    int automationRead(uint32_t channel, AutomationInfo* info, automation::Point* points, size_t capacity);
    int automationReset();
    // FLAC delivery (flac_encode.h; options "flac_frame" 256 .. 4096, default 4096, "flac_bits" 16 / 24, "flac_lpc_order" 0 .. 12 and "flac_md5" 0 / 1): the host-buffer render
    // delivered as RFC 9639 frames of a fixed block size, encoded on the GPU in the pack kernel's place (flac_encode.hip) — behind the
    // converter and the limiter, next to the meter. The sample values are processBlocksPcm's codes for the same render. The programme is
    // the frames FLAC calls delivered since creation or flacReset; FLAC frame j holds its frames [j F, (j + 1) F). A call returns the
    // bytes of the frames it completed (bytesOut[s]; maybe none) and leaves the open frame's codes on the device; flacFlush encodes
    // them as one short final frame, after which calls answer kInvalidPropertyValue until flacReset. spec.bits 0: the option's.
    // spec.drop / spec.take: of the frames the call delivers, the first `drop` stay out of the programme and at most `take` enter it.
    struct FlacSpec { uint32_t bits, channelsPerStream, dither, seed; uint64_t drop, take; };
    struct FlacInfo { uint32_t flacFrame, bits, channelsPerStream, streams, sampleRate, flushed; uint64_t frames; };
    struct FlacStreamInfo { uint64_t frames, totalSamples; uint32_t minFrameBytes, maxFrameBytes; };
    int processBlocksFlac(const PcmSource& src, void* const* outStreams, const size_t* capacities, size_t* bytesOut, size_t nOutStreams,
                          const FlacSpec& spec, size_t numFrames, int64_t sampleTime, PcmChannelStats* stats);
    int flacFlush(void* const* outStreams, const size_t* capacities, size_t* bytesOut, size_t nOutStreams);
    // perStream: `capacity` entries; frameBytes (may be null): [stream][frameCap], the byte length of every frame emitted so far
    int flacRead(FlacInfo* info, FlacStreamInfo* perStream, size_t capacity, uint32_t* frameBytes, size_t frameCap);
    int flacReset();
    // option "flac_lpc_order" (flac_lpc.h; 0 .. 12, default 0: none): the open programme's, else the option's
    uint32_t flacLpcOrder();
    // option "flac_md5" (flac_md5.h; 0, the default: off — no launch, no buffer, not one byte differs; 1): every stream of a programme carries
    // a running MD5 of its s16 / s24 bytes on the device (flac_md5.hip), which flacFlush finalises. state 0: the option is off in the
    // programme, or there is none; 1: running, the digests zero; 2: final. digests: [streams][16], `capacity` streams of room (null: the state only).
    int flacMd5Read(uint8_t* digests, size_t capacity, uint32_t* state);
    // render `numBlocks` blocks with a HIP event pair around every kernel launch; msOut[l] = mean
    // duration of launch level l (l < numLevels), msOut[numLevels] = epilogue. Returns levels + 1.
    int timeLaunches(size_t nOut, size_t numBlocks, float* msOut, size_t cap);
    // debug: render one block of launch level `level` tracing workgroup 0; out = 4 waves x 192 u64
    int traceLevel(size_t nOut, uint32_t level, unsigned long long* out, size_t cap);

    bool addSharedResource(const std::string& name, const float* const* ch, size_t nCh, size_t nSamples);
    void pruneSharedResources();
    // A shared resource from a file's own bytes (resource_load.h; option "resource_load_frames"): one interleaved stream of `channels`
    // channels and `frames` frames of format 1 s16 / 2 packed s24 / 3 f32 in `data`, or 4 FLAC in `flac` (position .. position + frames,
    // cut at the stream's end), at `sampleRate` Hz (0: the engine's). Decoded — and, at another rate, converted with the centred filter —
    // on the GPU into the resource's device rows, piece by piece on a stream of its own; the render lock is taken only to insert the
    // finished resource, so process() is not held up. A handle without a device runs load_host(). *inserted false: the name is taken.
    struct ResourceSrc { uint32_t format, channels; double sampleRate; uint64_t frames; const void* data; uint64_t bytes; const FlacIn* flac; };
    int addSharedResourcePcm(const std::string& name, const ResourceSrc& src, bool* inserted);
    int sharedResourceInfo(const std::string& name, uint32_t* channels, uint64_t* frames);
    // the floats the nodes see: frames [first, first + count) of `channel` (kInvalidPropertyValue: no such name, channel or range)
    int sharedResourceRead(const std::string& name, uint32_t channel, uint64_t first, uint64_t count, float* out);
    size_t gc(int32_t* out, size_t cap);
    size_t lastGc(int32_t* out, size_t cap);          // the ids the most recent gc() pruned (ascending)
    bool hasNode(int32_t id);
    void reset();
    // Runtime::processQueuedEvents (Runtime.h:64, 437-446): relays the newest meter / snapshot readout of every such node
    // of the current render sequence whose root is active. cb(type, json payload, user).
    // `blockwise`: every block's events since the last relay in block order, as a host that relayed after each block would have
    // got them (offline-renderer/index.ts:112-120), from the kernels' per-block readout logs
    int processQueuedEvents(void (*cb)(const char*, const char*, void*), void* user, bool blockwise = false);
    uint32_t eventWindowBlocks();          // blocks a blockwise relay window may span and still be exact for the newest plan's event nodes
    void setStream(hipStream_t s);
    const Stats& stats() const { return st; }
    uint64_t fftLaunchCount() const { return fftLaunches; }     // launches of the fft relay kernel / frames they transformed
    uint64_t fftFrameCount() const { return fftFrames; }
    // dry-engine introspection for host-logic tests: adopt the pending plan and describe it as JSON
    std::string describePlan();
    int setOption(const std::string& key, double value);
    uint32_t lastTimedBatch() const { return lastTimeBatch; }
    // option "profile_launches": HIP event pairs around every multi-block launch of processBlocks (same stream, inside
    // whatever region the caller times). msOut[l] = summed ms of level l, msOut[levels] = epilogue; launchSets = sets timed.
    int registerNodeType(const std::string& type, const HostVTable& vt);   // Runtime.h:480-487
    std::string snapshotJson();                        // Runtime::snapshot (Runtime.h:110, 489-498)
    std::string sharedResourceKeysJson();              // Runtime::getSharedResourceMapKeys (Runtime.h:94)
    int specInfo(size_t k, std::string* source, std::string* log, int* state, uint32_t* islands);
    int launchProfile(double* msOut, size_t cap, uint64_t* launchSets, uint64_t* blocks);

private:
    friend struct PlanBuilder;
    friend struct IslandSchedule;
    int initErr = 0;
    bool dry = false;                      // device == -1: host logic only, cannot render
    double sampleRate;
    int blockSize;                         // the engine's block: <= kMaxBlock frames (one LDS slot per buffer)
    std::vector<int32_t> tapNodeIds;       // every tapIn / tapOut node alive (setTapSlice)
    size_t tapSliceOff = 0;                // frames: where in the shared tap buffers the tap records point right now
    void setTapSlice(size_t off);
    int hostBlockSize = 0;                 // what the host created the runtime with: blockSize, or a multiple of kMaxBlock rendered in slices
    int device;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    // Two locks. `ctl` serialises the control plane (applyInstructions, gc, resources, options, snapshots ...) and owns
    // the node table's structure; `mu` guards what the render calls touch (current / pending plan, patch list, record
    // shadow, device buffers, stream). Order: ctl, then mu. process* take `mu` only; a commit drops `mu` while it plans.
    std::mutex ctl;
    std::mutex mu;
    Stats st;

    std::unordered_map<int32_t, Node> nodes;
    uint32_t nodesEpoch = 1;               // bumped whenever a node leaves `nodes` (Inlet::src memos of the planner)
    std::shared_ptr<TablePool> tablePool = std::make_shared<TablePool>();
    std::shared_ptr<ProgHeap> progHeap;    // island programs on the device (plan.cpp); owned by the mutator side (`ctl`)
    std::unordered_map<uint64_t, std::shared_ptr<IslandProgram>> islandShapeCache;   // structure -> a program of that structure (relocated for its peers)
    bool relocatePrograms = true;          // option "plan_relocate"
    size_t lastPlanProgDwords = 0, progHeapCap = 0;
    std::set<int32_t> currentRoots;
    std::unordered_map<std::string, ResourcePtr> resources;
    std::unordered_map<std::string, std::unique_ptr<HostVTable>> hostTypes;
    std::vector<float> hostIn, hostOut;    // staging for call-out nodes
    // generated text per island-program signature: 256 voices (and every re-plan of a live graph) format their text once
    // (the kernel cache key of a text lives NEXT TO the text, in the same shared object: nothing is keyed by an address)
    std::unordered_map<uint64_t, std::shared_ptr<SpecText>> specTextCache;
    // per-island programs of earlier builds (plan_island.cpp "island program cache"); same locking as specTextCache
    std::unordered_map<uint64_t, std::shared_ptr<IslandProgram>> islandCache;
    int planCache = 1;                     // 0 off, 1 reuse unchanged islands' programs, 2 schedule anyway and compare (tests)
    uint32_t planEpoch = 0;                // PlanBuilder::traverse marks
    int64_t curBlockTime = 0;              // sample time of the block being enqueued (call-out nodes get it as userData)
    bool shouldRebuild = false;
    bool rebuildOwed = false;              // a commit failed to build its plan: the next commit retries even without ACTIVATE_ROOTS
    std::vector<int32_t> lastPruned;
    bool planStale = false;                // a property changed the launch shape of the plan (convolve IR length)

    // record arena
    uint32_t* dRecs = nullptr;
    uint32_t recCapacity = 0;
    std::vector<uint32_t> shadow;          // host copy of every record as last written by the host
    std::vector<uint32_t> freeRecs;
    uint32_t nextRec = 0;
    std::vector<uint32_t> freshRecs;       // records to upload whole before the next block
    std::vector<std::pair<uint32_t, uint32_t>> recClones;   // (channel-0 record, new channel record): device-side copy of the live state at the next flush
    std::vector<uint8_t> freshFlag;        // freshFlag[rec] != 0 while rec is in freshRecs
    std::vector<Patch> patches;            // param patches to apply before the next block
    Patch* hPatches = nullptr;             // pinned staging
    uint32_t patchCap = 0;
    size_t patchCursor = 0;                // next free staging slot (rewound after a stream sync)

    // device globals, host mirror
    Globals* dGlobals = nullptr;
    Globals hGlobals{};
    uint32_t* dLcg = nullptr;

    // buffers
    float* dHbm = nullptr; size_t hbmBuffers = 0;
    float* dOutRing = nullptr; size_t outRingFloats = 0;
    float* hOut = nullptr; size_t hOutFloats = 0;     // pinned
    float* hOutDev = nullptr;                          // hOut as the device sees it (mapped)
    float* hIn = nullptr; size_t hInFloats = 0;       // pinned
    std::vector<void*> deferredFree;
    // the event relay's snapshot (processQueuedEvents): records copied device-side in stream order, fetched on a stream of its own
    hipStream_t relayStream = nullptr; hipEvent_t evRelay = nullptr;
    uint8_t* dRelay = nullptr; uint8_t* hRelay = nullptr; size_t relayBytes = 0;
    // the `fft` node's relay (fft_frames.hip): per size the window + twiddle tables on the device (made at the first setProperty that
    // names the size, never freed before the engine), and the relay's frame descriptors + spectra, device side and pinned host side
    void* dFftTables[13] = {};             // [log2 size]: `size` doubles of window, then `size` (re, im) double pairs
    int  ensureFftTables(uint32_t size);
    uint8_t* dFft = nullptr; uint8_t* hFft = nullptr; size_t fftBytes = 0;
    uint32_t captureHistoryBlocks = 0; // option "capture_history_blocks": relay window (host blocks) of takes the rings of NEW capture / mc.capture nodes keep (0: off)
    uint32_t eventHistoryBlocks = 0;   // option "event_history_blocks": relay window (host blocks) the rings of NEW scope / fft nodes keep (0: off)
    uint64_t fftLaunches = 0, fftFrames = 0;   // relay launches / frames transformed since the handle was made (describe_plan)
    // the relay's readers, one per node kind, over the context of one relay (engine_relay.cpp): they fetch off the render lock and
    // leave events and read-position write-backs in the context
    int  relayFftFrames(RelayCtx& c);                     // every fft node's frames of the window: collect, ONE launch ...
    void relayFft(RelayCtx& c, size_t item);              // ... and the events of one node from its spectra
    int  relayScope(RelayCtx& c, Node& n, const uint32_t* rec, uint32_t order);
    int  relayCapture(RelayCtx& c, Node& n, const uint32_t* rec, uint32_t order);
    int  relayMeter(RelayCtx& c, Node& n, const uint32_t* rec, uint32_t order);
    int  relaySnapshot(RelayCtx& c, Node& n, const uint32_t* rec, uint32_t order);
    uint64_t relayBlocksMark = 0;          // Stats::blocksRendered at the last relay: a blockwise relay's window starts here
    // A host block longer than the engine's is k slices = k engine blocks, and the reference's nodes queue their readouts per HOST block
    // (one meter readout over all its frames, Analyzers.h:38-39): Stats::blocksRendered at the end of every host block rendered since the
    // last relay (kept only while hostBlockSize != blockSize; `mu` held), so that a relay can put the slices back together.
    std::deque<uint64_t> hostBlockEnds;
    void noteHostBlockEnd() { if (hostBlockSize != blockSize) { if (hostBlockEnds.size() >= 65536) hostBlockEnds.pop_front(); hostBlockEnds.push_back(st.blocksRendered); } }
    std::vector<std::shared_ptr<Plan>> retiredPlans;   // replaced plans whose launches may still be in flight; released by freeDeferred()

    // host-buffer launch sets (processBlocksHost): copy stream, pinned + device staging halves, hand-over events
    hipStream_t ioStream = nullptr;
    float* hStageOut[2] = {nullptr, nullptr}; float* hStageIn[2] = {nullptr, nullptr};
    float* dStageOut[2] = {nullptr, nullptr}; float* dStageIn[2] = {nullptr, nullptr};
    size_t stageOutFloats = 0, stageInFloats = 0;
    hipEvent_t evIn[2] = {nullptr, nullptr}, evRendered[2] = {nullptr, nullptr}, evOut[2] = {nullptr, nullptr};
    int ensureHostStaging(size_t outFloats, size_t inFloats);
    // PCM delivery (processBlocksPcm): packed halves behind the float ones (streams, then the set's per-channel statistics), and
    // the pack kernel's row table for the group size in use
    unsigned char* hPcm[2] = {nullptr, nullptr}; unsigned char* dPcm[2] = {nullptr, nullptr};
    size_t pcmBytes = 0;
    uint16_t* dPcmRowBase = nullptr; uint32_t pcmTableGroup = 0, pcmRowDwords = 0;
    int ensurePcmStaging(size_t bytes, uint32_t group);
    // PCM input (processBlocksPcmIo): packed halves in front of the float input halves, the unpack kernel's row table
    unsigned char* hPcmIn[2] = {nullptr, nullptr}; unsigned char* dPcmIn[2] = {nullptr, nullptr};
    size_t pcmInBytes = 0;
    uint16_t* dPcmInRowBase = nullptr; uint32_t pcmInTableGroup = 0, pcmInRowDwords = 0;
    int ensurePcmInStaging(size_t bytes, uint32_t group);
    // loudness meter (option "loudness_meter"): carried state per channel on the device, the segment scratch of a set, and per half the
    // sums of the sub-blocks the set completed (they leave with the set's D2H)
    bool loudnessOn = false;
    loudness::Plan loudPlan{};
    uint32_t loudChannels = 0;             // channels of the programme (0: none yet)
    uint64_t loudFrames = 0;               // programme frames metered so far
    std::vector<std::vector<double>> loudSeries;      // [channel]: mean squares of the completed sub-blocks
    loudness::ChannelState* dLoudState = nullptr; size_t loudStateCap = 0;
    double* dLoudSeg = nullptr; double* dLoudEnergy = nullptr; size_t loudSegCap = 0, loudSegChannels = 0;
    double* dLoudOut[2] = {nullptr, nullptr}; double* hLoudOut[2] = {nullptr, nullptr}; size_t loudOutStride = 0, loudOutChannels = 0;
    uint32_t loudCountOf[2] = {0, 0};      // sub-blocks the set in each half completed
    // spectrum analyser (spectrumSet): the tables on both sides; per channel two copies of the last size - 1 delivered frames and the
    // running sums on the device; per half the frames a set completes (device, pinned); the emitted frames nobody has read yet
    bool spcOn = false, spcFlushed = false;
    spectrum::Plan spcPlan{}, spcPlanDev{};          // host pointers (the vectors below) / device pointers (dSpcTables)
    uint32_t spcCenter = 0;
    std::vector<double> spcWindow, spcTwiddles; std::vector<uint32_t> spcBandIdx; std::vector<float> spcWeights;
    unsigned char* dSpcTables = nullptr;
    uint32_t spcChannels = 0;              // channels of the programme (0: none yet)
    uint64_t spcFrames = 0, spcEmitted = 0;         // programme frames delivered / analyser frames emitted so far
    float* dSpcTail[2] = {nullptr, nullptr}; int spcTailCur = 0; double* dSpcSums = nullptr; size_t spcStateCap = 0;
    float* dSpcOut[2] = {nullptr, nullptr}; float* hSpcOut[2] = {nullptr, nullptr}; size_t spcOutCap = 0, spcOutChannels = 0;   // (cap: frames per channel)
    uint32_t spcCountOf[2] = {0, 0};       // frames the set in each half completed
    std::vector<std::vector<float>> spcQueue; uint64_t spcQueueFirst = 0;      // [channel]: frames x columns; the index of the first one
    static constexpr size_t kSpcHalfBytes = 256u << 20;                       // the most a pinned half may hold
    size_t spectrumSetFrames(size_t deliveredFrames) const { return deliveredFrames / spcPlan.hop + 2; }     // frames a set of that many completes at most
    // inspector (qcSet): per channel and per pair the programme's summary on the device; per set the tiles' summaries, the leaves' sums
    // and the overview's edge pieces (scratch); per half the buckets a set completes (device, pinned); the buckets nobody has read yet
    bool qcOn = false;
    qc::Spec qcSpec{}; std::vector<uint32_t> qcPairs; uint64_t qcSkip = 0, qcLimit = 0;
    uint32_t qcChannels = 0;               // channels of the programme (0: none yet)
    uint64_t qcFrames = 0, qcDelivered = 0;         // programme frames inspected / frames delivered by inspected calls (the window's clock)
    qc::ChannelState* dQcState = nullptr; qc::PairState* dQcPairState = nullptr; uint32_t* dQcPairs = nullptr; size_t qcStateCap = 0;
    qc::Stretch<uint32_t>* dQcTiles = nullptr; double* dQcLeaves = nullptr; float* dQcEdges = nullptr; size_t qcSetCap = 0, qcScratchChannels = 0;
    float* dQcOut[2] = {nullptr, nullptr}; float* hQcOut[2] = {nullptr, nullptr}; size_t qcOutCap = 0, qcOutChannels = 0;      // (cap: buckets per channel)
    uint32_t qcCountOf[2] = {0, 0};        // buckets the set in each half completed
    std::vector<std::vector<float>> qcQueue; uint64_t qcQueueFirst = 0;        // [channel]: buckets x 2; the index of the first one
    int ensureQc(size_t channels, size_t setFrames);            // (`mu` held) a programme of `channels`; scratch for sets of `setFrames` (0: none)
    int qcResetLocked(size_t channels);
    void qcFree();
    int ensureSpectrum(size_t channels, size_t setFrames);      // (`mu` held) a programme of `channels`; halves for sets of `setFrames` (0: none)
    int spectrumResetLocked(size_t channels);
    void spectrumFree(bool tables);
    // breakpoint automation (automationSet): every lane's points behind one another, on the host and — uploaded when a lane is set —
    // on the device. The set is immutable and shared: a render call works on the one it found at its start, whatever is set meanwhile.
    struct AutoLanes {
        std::vector<automation::Point> points;
        uint32_t offset[automation::kMaxChannels] = {}, count[automation::kMaxChannels] = {};
        uint32_t lowest = 0, inputs = 0;       // the lowest bound channel; the highest + 1
        automation::Point* dev = nullptr;
        ~AutoLanes();
    };
    std::shared_ptr<const AutoLanes> autoLanes;      // null: no lane
    int ensureLoudness(size_t channels, size_t setFrames);      // (`mu` held, both streams idle)
    int loudnessResetLocked(size_t channels);
    void loudnessFree();
    // delivery-rate conversion (option "resample_rate"): the tables and two copies of the carried frames on the device (a set's kernel
    // reads one, its history step writes the other), per half the converted set; the programme's clock on the host
    bool resampleOn = false;
    double resampleRate = 0.0;             // the delivery rate (0: off)
    resample::Plan resPlan{};
    std::vector<float> resTable; std::vector<int32_t> resRowBase;                 // host copies: the scalar loop's
    float* dResTable = nullptr; int32_t* dResRowBase = nullptr;
    float* dResHist[2] = {nullptr, nullptr}; size_t resHistChannels = 0; int resHistCur = 0;
    float* dRes[2] = {nullptr, nullptr}; size_t resFloats = 0;
    uint32_t resChannels = 0;              // channels of the programme (0: none yet)
    uint64_t resFramesIn = 0, resFramesOut = 0;
    uint32_t resValidOf[2] = {0, 0}; uint64_t resOffsetOf[2] = {0, 0};            // per half: the set's delivered frames, and where in the call's arrays they go
    double deliveryRate() const { return resampleOn ? resampleRate : sampleRate; }
    int setResampleRate(double hz);                              // (`mu` held)
    int ensureResample(size_t channels, size_t outBlocksCap);   // (`mu` held, both streams idle)
    int resampleResetLocked(size_t channels);
    void resampleFree();
    // input-rate conversion (option "input_rate"): the tables and two copies of the carried decoded frames on the device (a set's kernel
    // reads one, its history step writes the other); the programme's clock on the host
    bool inResOn = false;
    double inResRate = 0.0;                // the inputs' rate (0: off)
    resample::Plan inPlan{};
    std::vector<float> inTable; std::vector<int32_t> inRowBase;                   // host copies: the scalar loop's
    float* dInTable = nullptr; int32_t* dInRowBase = nullptr;
    float* dInHist[2] = {nullptr, nullptr}; size_t inHistChannels = 0; int inHistCur = 0;
    uint32_t inChannels = 0;               // channels of the programme (0: none yet)
    uint64_t inFramesIn = 0, inFramesOut = 0;                                     // inFramesIn = inputs_before(inFramesOut), always
    int setInputRate(double hz);                                 // (`mu` held)
    int ensureInputResample(size_t channels);                    // (`mu` held, both streams idle)
    int inputResampleResetLocked(size_t channels);
    void inputResampleFree();
    // the limiter (options "limiter", "limiter_*"): two copies of the carried state on the device (a set's kernels read one, its history
    // step writes the other), the statistics, the per-set scratch and per half the limited set; the programme's clock on the host
    bool limiterOn = false;
    double limCeilingDb = -1.0, limGainDb = 0.0, limLookaheadMs = 1.5, limReleaseMs = 500.0, limLink = 0.0;
    limiter::Plan limPlan{};
    loudness::Plan limMeter{};             // the delivery rate's interpolator: the detector
    unsigned char* dLimState[2] = {nullptr, nullptr}; size_t limStateCap = 0; int limCur = 0;
    limiter::GroupStats* dLimStats = nullptr; size_t limStatsCap = 0;
    double* dLimFrames = nullptr; double* dLimTiles = nullptr; size_t limFrameCap = 0, limTileCap = 0, limScratchGroups = 0;
    float* dLim[2] = {nullptr, nullptr}; size_t limFloats = 0;
    uint32_t limChannels = 0;              // channels of the programme (0: none yet)
    uint64_t limFrames = 0;
    int setLimiterOption(const std::string& key, double value);      // (`mu` held)
    int limiterReplan(double rate, bool apply);                      // the plan at `rate` from the current parameters (`mu` held)
    int ensureLimiter(size_t channels, size_t outBlocksCap, size_t setFrames);   // (`mu` held, both streams idle)
    int limiterResetLocked(size_t channels);
    void limiterFree();
    // noise-shaped requantisation (noiseShapeSet): the channels' carried states on the device, updated in place by the one stream that
    // touches them, and the set's codes in a buffer shaped like the float halves; the programme's clock on the host
    uint32_t nsTaps = 0;                   // 0: off
    int32_t nsCq[noise_shape::kMaxTaps] = {};
    noise_shape::ChannelState* dNsState = nullptr; size_t nsStateCap = 0;
    int32_t* dNsCodes = nullptr; size_t nsCodesCap = 0;
    uint32_t nsChannels = 0;               // channels of the programme (0: none yet)
    uint64_t nsFrames = 0;
    int ensureNoiseShape(size_t channels, size_t codes);             // (`mu` held) a programme of `channels`, room for `codes` codes
    int noiseShapeResetLocked();
    void noiseShapeFree();
    template <class T> int growHalves(T* (&h)[2], T* (&d)[2], size_t& have, size_t want);      // (engine_render.cpp: float and unsigned char)
    int growPackedHalves(unsigned char* (&h)[2], unsigned char* (&d)[2], size_t& have, size_t want) { return growHalves(h, d, have, want); }
    int ensureRowTable(uint16_t*& dev, uint32_t& haveGroup, uint32_t& dwords, uint32_t group);
    // what a packed delivery counts per channel, summed over the call (peakBits: pcm_pack.h)
    struct ChannelTally {
        std::vector<uint32_t> peakBits; std::vector<uint64_t> over, nonfinite;
        void init(size_t n) { peakBits.assign(n, 0u); over.assign(n, 0u); nonfinite.assign(n, 0u); }
        void writeTo(PcmChannelStats* stats) const {      // (null: nobody asked)
            for (size_t c = 0; stats && c < peakBits.size(); ++c) {
                std::memcpy(&stats[c].peak, &peakBits[c], 4);
                stats[c].reserved = 0u; stats[c].over = over[c]; stats[c].nonfinite = nonfinite[c];
            }
        }
    };
    // what a processBlocksPcm call carries through the render
    struct PcmJob {
        PcmSpec spec;
        void* const* streams; size_t nStreams;
        ChannelTally tally;
        uint32_t validOf[2] = {0, 0};           // delivered frames of the set in each half
    };
    // FLAC delivery: the open frame's codes, the set's codes, the candidates' subframes and their bit counts on the device; the frames
    // and their length table go through the packed halves (hPcm / dPcm), the payload copied on a stream of its own once the table is here
    struct FlacJob {
        FlacSpec spec;
        void* const* streams; const size_t* caps; size_t* bytes; size_t nStreams;
        ChannelTally tally;
        uint32_t framesOf[2] = {0, 0};          // FLAC frames of the set in each half
        uint64_t dropLeft = 0, takeLeft = 0;    // of the call's delivered frames still to come
        size_t statsOff = 0, payloadOff = 0, stride = 0;
    };
    uint32_t flacFrameOpt = 4096, flacBitsOpt = 16, flacLpcOpt = 0;
    uint32_t flacLpc = 0;       // the programme's LPC order (flac_lpc.h), taken with flacFF
    uint32_t flacMd5Opt = 0, flacMd5 = 0;       // option "flac_md5", and the programme's, taken with flacFF
    bool flacMd5Final = false;                  // flacFlush has brought the digests over
    std::vector<uint8_t> flacDigests;           // [flacStreams][16] once final
    unsigned char* dFlacMd5 = nullptr;          // flacMd5Cap records (flac_md5::Record), then as many 16-byte digests
    size_t flacMd5Cap = 0;
    flac_md5::Record* flacMd5Records() const { return reinterpret_cast<flac_md5::Record*>(dFlacMd5); }
    uint8_t* flacMd5Digests() const { return dFlacMd5 + flacMd5Cap * sizeof(flac_md5::Record); }
    int flacMd5Launch(uint32_t first, uint32_t count, bool finish);        // (`mu` held) on `stream`
    int flacMd5Finish();                                                   // (`mu` held) pad, chain, digests -> flacDigests
    uint32_t flacFF = 0, flacBits = 0, flacG = 0, flacStreams = 0, flacRate = 0, flacOpen = 0;      // the programme (flacStreams 0: none yet)
    bool flacFlushed = false;
    uint64_t flacFrames = 0, flacEmitted = 0;   // programme frames delivered; FLAC frames emitted per stream
    std::vector<std::vector<uint32_t>> flacFrameBytes;
    int32_t* dFlacCarry = nullptr; int32_t* dFlacCodes = nullptr; uint32_t* dFlacSlots = nullptr; uint32_t* dFlacSubBits = nullptr;
    size_t flacCarryCh = 0, flacCodesCh = 0, flacCodesCap = 0, flacSlotCount = 0, flacSlotWords = 0;
    hipStream_t flacStream = nullptr;
    int ensureFlac(FlacJob& job, size_t setFrames);     // (`mu` held, both streams idle)
    int flacResetLocked();
    void flacFree();
    int flacDeliver(FlacJob& job, int half);            // the table is in the pinned half: payload -> the caller's buffers
    // FLAC input (flac_decode.h, engine_flac_in.cpp): per launch set the FLAC frames that cover the set's input frames go through
    // staging halves of their own (two record tables in front of the bytes), are decoded into the packed input half (flac_decode.hip)
    // and leave an error record that comes back with the set. The scratch and the descriptors are touched by the render stream's
    // kernels only, in order: one copy serves both halves.
    struct FlacInSet {
        std::vector<FlacInFrame> frames; std::vector<FlacInStream> streams;
        std::vector<uint64_t> from, len;        // per stream: its covering bytes in the caller's buffer
        size_t stagedBytes = 0, scratchInts = 0;
        std::vector<flac_in_md5::Job> jobs;     // option "flac_in_md5": one per stream, staged at jobsOff behind the bytes
        size_t jobsOff = 0; bool md5Work = false, md5Finish = false;
    };
    FlacInSet flacInSets[2];
    unsigned char* hFlacIn[2] = {nullptr, nullptr}; unsigned char* dFlacIn[2] = {nullptr, nullptr};
    size_t flacInBytes = 0;
    FlacInError* hFlacInErr = nullptr; FlacInError* dFlacInErr = nullptr;      // one per half
    void* dFlacInSubs = nullptr; uint32_t* dFlacInState = nullptr; int32_t* dFlacInScratch = nullptr;
    size_t flacInFrameCap = 0, flacInScratchCap = 0;
    bool flacInErrSet = false; uint32_t flacInErrStream = 0, flacInErrReason = 0; uint64_t flacInErrFrame = 0;
    int flacInCheck(const PcmSource& src) const;
    uint32_t flacInBits(const PcmSource& src) const;
    void flacInPlan(const PcmSource& src, uint64_t from, size_t valid, FlacInSet& set, bool md5 = false) const;
    int ensureFlacIn(size_t stagedBytes, size_t frames, size_t scratchInts, uint32_t G);      // (`mu` held)
    void flacInStage(const PcmSource& src, const FlacInSet& set, int half);
    int flacInLaunch(const FlacInSet& set, int half, uint32_t G, uint32_t bits, size_t valid, size_t streamStride);      // (`mu` held)
    bool flacInFailed(int half);                // the set's error record has arrived: anything in it -> the last error
    int flacInHostImage(const PcmSource& src, uint64_t from, size_t n, std::vector<std::vector<unsigned char>>& images, flac_md5::Record* md5 = nullptr);
    void flacInFree();
    // option "flac_in_md5": kMaxHostIn records on the device, as many 16-byte digests behind them and a pinned copy of the digests
    uint32_t flacInMd5Opt = 0;
    std::vector<flac_in_md5::Slot> flacInMd5Slots;      // the slots fed since the reset
    unsigned char* dFlacInMd5 = nullptr; uint8_t* hFlacInMd5 = nullptr;
    flac_md5::Record* flacInMd5Records() const { return reinterpret_cast<flac_md5::Record*>(dFlacInMd5); }
    uint8_t* flacInMd5Digests() const { return dFlacInMd5 + (size_t)kMaxHostIn * sizeof(flac_md5::Record); }
    int ensureFlacInMd5();                                                  // (`mu` held)
    static flac_in_md5::Job flacInMd5Job(const FlacIn& f, const FlacInSet& set, size_t s, flac_in_md5::Slot& slot);      // one stream's
    void flacInMd5Jobs(const PcmSource& src, FlacInSet& set, int half);     // (`mu` held) the rule per stream -> the set's staged jobs
    int flacInMd5Launch(const FlacInSet& set, int half, uint32_t G, uint32_t bits);      // (`mu` held) on `stream`, behind the decode
    int flacInMd5ResetLocked();
    // The resource loader (engine_resource_load.cpp): everything below is touched under `ctl` only and by the loader's own stream —
    // never by a render. Two staging halves (pinned: the piece as it lies in the file; device: the FLAC bytes, and the PCM image the
    // load kernels read), an event per half, the FLAC decoder's scratch, the last rate pair's tables and the last group's row table.
    uint32_t resourceLoadFramesOpt = 1u << 20;      // option "resource_load_frames"
    hipStream_t loadStream = nullptr;
    hipEvent_t loadDone[2] = {nullptr, nullptr};
    unsigned char* hLoad[2] = {nullptr, nullptr}; unsigned char* dLoadFlac[2] = {nullptr, nullptr}; unsigned char* dLoadImage[2] = {nullptr, nullptr};
    size_t hLoadBytes = 0, dLoadFlacBytes = 0, dLoadImageBytes = 0;
    FlacInError* hLoadErr = nullptr; FlacInError* dLoadErr = nullptr;      // one per half
    void* dLoadSubs = nullptr; uint32_t* dLoadState = nullptr; int32_t* dLoadScratch = nullptr;
    size_t loadFrameCap = 0, loadScratchCap = 0;
    unsigned char* dLoadMd5 = nullptr;              // option "flac_in_md5": the current load's record and, behind it, its digest
    resample::Plan loadPlan{};                      // L == 0: no tables yet
    std::vector<float> loadTable; std::vector<int32_t> loadRowBase;
    float* dLoadTable = nullptr; int32_t* dLoadRowBase = nullptr;
    uint16_t* dLoadRowTable = nullptr; uint32_t loadRowGroup = 0, loadRowDwords = 0;
    int resourceLoadTables(const resample::Plan& p);
    int resourceLoadGrow(size_t pinned, size_t flacBytes, size_t imageBytes, size_t frames, size_t scratchInts, uint32_t G);
    int resourceLoadDevice(const ResourceSrc& src, uint32_t fmt, uint64_t N, const resample::Plan* plan, Resource& r);
    int resourceLoadHost(const ResourceSrc& src, uint32_t fmt, uint64_t N, const resample::Plan* plan, Resource& r);
    void resourceLoadFree();
    // the host floats of a resource: `channels`, fetched from the device rows first where the resource was made there (`mu` held)
    const std::vector<std::vector<float>>& resourceHost(const ResourcePtr& r);
    // A host-buffer render call: its arguments (`pcm` null: planar floats only; `out` may be null with `pcm` or `flac`: nobody asked for
    // the floats; with `src` the nIn input channels come from its streams and `in` is null) and what both renderers derive from them and
    // from the options, computed once by hostCall().
    struct HostCall {
        const float* const* in; size_t nIn; float* const* out; size_t nOut; size_t numFrames; int64_t sampleTime;
        PcmJob* pcm; const PcmSource* src; FlacJob* flac;
        size_t bs, hb;                                  // the engine's block, the host's
        bool flacSrc; uint32_t flacInB;                 // a FLAC source, its bits
        bool inMd5;                                     // ... hashed under option "flac_in_md5"
        uint32_t srcG, srcFmt; size_t srcB;             // the source's group, format (a FLAC source: its image's) and sample bytes
        bool wantFloat;
        uint32_t pcmG, pcmFmt; size_t pcmB;
        bool packed;                                    // PCM or FLAC delivery
        bool meter, resamp, limit, inres;               // options "loudness_meter", "resample_rate", "limiter", "input_rate" apply to this call
        resample::Plan rp, inp; limiter::Plan lmp;
        bool shape; uint32_t shapeBits, shapeDither, shapeSeed;      // noiseShapeSet applies to this call: s16 / s24 / FLAC delivery
        bool spectrum;                                  // spectrumSet applies to this call
        bool qc;                                        // qcSet applies to this call
        uint32_t inG, inFmt; size_t inStreams, inB;     // the inputs as streams: planar floats count as nIn one-channel float streams
        std::shared_ptr<const AutoLanes> lanes;         // automationSet applies to this call (null: no lane)
        size_t nEng;                                    // the engine's input channels: nIn, or with lanes max(nIn, highest lane + 1)
        const unsigned char* inStream(size_t s) const { return src ? static_cast<const unsigned char*>(src->streams[s]) : reinterpret_cast<const unsigned char*>(in[s]); }
    };
    HostCall hostCall(const float* const* in, size_t nIn, float* const* out, size_t nOut, size_t numFrames, int64_t sampleTime, PcmJob* pcm,
                      const PcmSource* src, FlacJob* flac) const;
    // processBlocksHost / Pcm / PcmIo / Flac: decides between the two renderers — taps under a host block longer than the engine's and
    // ragged slices go host block by host block through process() (renderHostBlocks, engine_host_blocks.cpp); everything else through
    // the launch-set loop, which is the rest of this function (engine_render.cpp)
    int renderHostSets(const float* const* in, size_t nIn, float* const* out, size_t nOut, size_t numFrames, int64_t sampleTime, PcmJob* pcm,
                       const PcmSource* src = nullptr, FlacJob* flac = nullptr);
    struct HostCarry;                                   // (engine_host_blocks.cpp: the stages' carried state on the host for a call)
    int renderHostBlocks(const HostCall& c);
    // enqueue `numBlocks` blocks on `stream` (no synchronise at the end): the body of processBlocks
    int enqueueBlocks(const float* inDev, size_t nIn, float* outDev, size_t nOut, size_t numBlocks, int64_t sampleTime);

    std::shared_ptr<Plan> current, pending;
    uint32_t maxLdsConfigured = 0;
    // ---- elemhip_process ends by spinning on a word the block's epilogue kernel publishes to mapped host memory behind the output block,
    // not by synchronising the stream (option "sync_poll", default 1; island.inc publish_done) ----
    bool syncPoll = true;
    uint32_t* hDone = nullptr; uint32_t* dDone = nullptr;     // the word: host / device address
    uint32_t doneSeq = 0;
    uint32_t* armFlag = nullptr; uint32_t armValue = 0;        // what the epilogue launch of the call being enqueued publishes (null: nothing)
    bool flagArmed = false;                                    // ... and whether an epilogue kernel took it
    uint32_t unsyncedCalls = 0;                                // calls since the stream was last synchronised for real
    uint64_t syncPolls = 0, syncPollFallbacks = 0;
    // ---- option "resident": elemhip_process through a kernel that stays on the GPU between calls (resident.hip) ----
    bool residentOpt = false;
    uint32_t residentIdleUs = 2000;        // option "resident_idle_us": the kernel leaves by itself after this long without a block
    uint32_t residentAfter = 3;            // ... and is launched once this many plain blocks in a row went through the launch path
    bool residentLive = false;             // the kernel is (or may still be) on `stream`
    uint32_t residentSeq = 0, residentStreak = 0;
    const Plan* residentPlan = nullptr; size_t residentNIn = 0, residentNOut = 0;
    ResidentCtl* hResident = nullptr; ResidentCtl* dResidentCtl = nullptr;   // mapped host memory, host / device address
    float* hResIn = nullptr; float* hResOut = nullptr; const float* dResIn = nullptr; float* dResOut = nullptr; size_t resInFloats = 0, resOutFloats = 0;
    unsigned long long* dResidentSync = nullptr;
    uint32_t residentLdsConfigured = 0;
    uint64_t residentTicksBody = 0, residentTicksEpilogue = 0;   // ELEMHIP_RESIDENT_TRACE: device-side phase times of this residency
    bool residentEligible(const Plan& p, size_t nIn, size_t nOut) const;
    int residentStart(const Plan& p, size_t nIn, size_t nOut);
    void residentStop();                   // (`mu` held) ask the kernel to leave and wait until it has; a no-op when it is not there
    // renders one block through the live kernel: kOk, an error, or kResidentGone — it left (idle) before it saw the block: launch path
    int residentBlock(const float* const* in, size_t nIn, float* const* out, size_t nOut, size_t n);
    static constexpr int kResidentGone = -1000;
    bool useGraph = true;
    int  graphBlocks = 8;
    bool hostOutDirect = true;             // process(): the epilogue kernel writes into the mapped pinned output block
    uint32_t convMinP = 0xFFFFFFFFu, convMaxP = 0;   // fewest / most partitions of any impulse response set so far
    bool convLong = true;                  // option "conv_long": launch sets of a multiple of 8 blocks render IRs of >= 32 partitions with 4096-sample partitions (conv_long.inc)
    bool deviceClockBehind = false;        // direct-I/O convolver sets moved hGlobals.sampleTime on without patching the device's copy (flushPending catches it up)
    bool nextSetDirect = false;            // ... unless the launch being prepared is another such set
    uint32_t convUid = 0;                  // conv::H_UID of the newest convolver state
    uint64_t convScratchKey = ~0ull;       // (batch_blocks, long history rows) the scratch headers were zeroed for
    std::set<int32_t> convStaleNodes;      // convolve nodes last rendered by a long-partition set: their `overlap` is made on demand (fixConvOverlaps), per node
    void fixConvOverlaps(const Plan& p);   // ... before the next 512-partition evaluation (block-at-a-time launches, sets that are no multiple of 8 blocks)
    bool convDirectIo = true;              // option "conv_direct_io": a plan of long-partition convolvers only reads the caller's input / writes the caller's output in place
    // the launch set being enqueued (enqueueBlocks -> enqueueBatch -> launchConvolveBatch): where its convolvers read / write directly
    const float* setInDirect = nullptr; float* setOutDirect = nullptr; uint32_t setNumIn = 0, setNumOut = 0;
    uint64_t convDirectSets = 0;
    void chooseConvDirectIo(const Plan& p, size_t nIn, size_t nOut, uint32_t batch, bool haveIn, bool& dIn, bool& dOut);
    uint64_t convLongSets = 0;             // launch sets in which some node took the long-partition kernels (describe_plan)
    uint32_t convMaxQp = 0;                // most long-partition tap rows of any impulse response set so far (sizes the scratch)
    int convMfma = 1;                      // conv.hip elemhip_convolve_batch_mac: 1 v_mfma_f32_4x4x1_16B_f32 Toeplitz tiles, 0 v_pk_fma_f32 (r03)
    bool skipIdleLaunches = true;          // option "skip_idle_launches": launches of a level whose islands all belong to roots that do not run are left out
    bool specBlocks = true;                // process(): whole blocks of a settled, fully compiled sequence use the specialised kernels
    int  batchBlocks = 64;                 // blocks per multi-block launch in processBlocks (1 = per-block launches)
    int  pipelineCopies = 6;               // blocks a stateful island keeps in flight inside a multi-block launch
    bool convAligned = true;               // every process call so far rendered whole 512-frame blocks (conv.hip batch path)
    float* dConvScratch = nullptr; size_t convScratchFloats = 0;
    uint32_t fuseSvfCoef = 2;              // plan.cpp: svf coefficient pre-pass inside the scan: 0 never, 1 always, 2 in lane-packed islands
    uint32_t mixerSplit = 2;               // workgroups a mixer island is cut into (plan.cpp; each renders blockSize / split frames on 8 / split waves)
    int  packIslands = 0;                  // option "pack_islands": same-shape islands merged into one workgroup (0 auto: when a launch level has more
                                           // stateful islands than the device has CUs; 1 never; K: K per island)
    bool packRoots = false;                // option "pack_roots": lane-packing may merge islands of different ACTIVE roots (render jobs with a root each)
    int  packMax = 2, cuCount = 256;       // auto mode: at most packMax per island (measured on C2: 2 per island pays, 3 leaves two buffer sets and loses); CUs of the device
    bool mergePhases = true;               // option "merge_phases": constant-frequency phasors and oscillator phases of a stage share one recurrence task (OP_PHASE)
    uint32_t statelessRows = 64;           // gridDim.y of a multi-block launch: blocks that stateless islands render side by side
    int  timeBatch = 1;
    int  specialize = 1;                   // 0: interpreter kernels only; 1: specialised kernels compiled in the background and used
                                           // once ready; 2: commit() waits for them (deterministic: tests, benchmarks)
    std::vector<hipStream_t> auxStreams;   // side streams for the independent launches of one level (launchLevelBatch)
    std::vector<hipEvent_t> auxDone;
    hipEvent_t forkEvent = nullptr;
    uint32_t profileEvery = 1, profSetCounter = 0;   // option "profile_launches" = N: events around every N-th launch set
    bool profileLaunches = false;
    std::vector<double> profMs;            // per level + epilogue, summed over the launch sets profiled so far
    uint64_t profSets = 0, profBlocks = 0;
    std::vector<hipEvent_t> profEvents;    // event pool of the current processBlocks call
    size_t profUsed = 0;
    std::vector<uint32_t> profSlots;       // per used pair: which profMs slot it feeds
    hipEvent_t profEvent();
    void profCollect();
    uint32_t lastTimeBatch = 1;            // blocks per launch the last timeLaunches actually used                    // timeLaunches: blocks per timed launch

    uint32_t allocRec();
    uint32_t channelRec(Node& n, uint32_t ch);           // record of output channel `ch` of a (multi-output) node
    void writeRec(uint32_t rec, uint32_t dword, uint32_t value);
    void writeTableChannel(Node& n, uint32_t ch, uint32_t rec);
    void writeChannelBuffer(Node& n, uint32_t ch, uint32_t rec);
    int  ensureResourceChannelOnDevice(const ResourcePtr& r, uint32_t ch, const void** ptr, uint32_t* len);
    void writeParam(Node& n, uint32_t dword, uint32_t value);
    void writeParamF(Node& n, uint32_t dword, float value) { uint32_t u; memcpy(&u, &value, 4); writeParam(n, dword, u); }
    void writeParamI64(Node& n, uint32_t dword, int64_t value) { writeParam(n, dword, (uint32_t)((uint64_t)value & 0xFFFFFFFFu)); writeParam(n, dword + 1, (uint32_t)((uint64_t)value >> 32)); }   // two dwords, low first
    void writeParamF64(Node& n, uint32_t dword, double value) { int64_t i; memcpy(&i, &value, 8); writeParamI64(n, dword, i); }
    void writeParamPtr(Node& n, uint32_t dword, const void* p) { writeParamI64(n, dword, (int64_t)reinterpret_cast<uintptr_t>(p)); }
    void writeChannelBuffers(Node& n) { for (size_t c = 0; c < n.chanRecs.size(); ++c) writeChannelBuffer(n, (uint32_t)c + 1u, n.chanRecs[c]); }   // mc.*: channels >= 1
    int  findResource(const Value& v, ResourcePtr& out);  // engine_nodes.cpp: a `path` property -> the shared resource it names
    int  bindResource(Node& n, const Value& v);            // ... held by the node, channel 0 on the device
    int  uploadRing(Node& n, const void* words, size_t count);
    void freeRec(uint32_t rec);                            // gc: the record back to the free list, queued writes to it dropped
    int  allocRing(Node& n, size_t floats);
    size_t captureLogFloats(const Node& n) const;
    void writeCaptureRing(Node& n, size_t cap);
    int  ensureResourceOnDevice(const ResourcePtr& r);
    int  setConvolverIr(Node& n, const ResourcePtr& res);
    ResourcePtr tapResource(const std::string& name);
    void rootUpdateStep(Node& n);
    int  flushPending();                   // fresh records + patches -> device (stream-ordered)
    void freeDeferred();
    void dropGraphs();                     // the current plan's captured graphs (a pointer or launch geometry baked into them changed)
    int  ensureHbm(size_t buffers);
    size_t arenaBuffers(const Plan& p, size_t blocks) const;
    size_t maxSetBlocks(const Plan& p) const;
    int  ensureOutRing(size_t floats);
    int  swapInPending();
    void enqueueBlock(const Plan& p, float* outRing = nullptr);
    int  renderHostNodes(const Plan& p, size_t level);   // call-out nodes of one launch level (synchronises the stream)
    void enqueueBatch(const Plan& p, uint32_t batch, float* outRing = nullptr);
    // one block of a fully compiled plan whose root fades are still running: the specialised level launches of a set of one, then
    // the PER-BLOCK epilogue (fades advance, taps promoted) — the two blocks after every commit of a live graph
    void enqueueSpecBlock(const Plan& p, float* outRing = nullptr);
    bool specBlockOk(const Plan& p) const;
    void launchConvolveBatch(const Plan& p, size_t l, uint32_t batch, uint32_t arenaFloats);
    // specialised kernels when ready, else the interpreter
    void launchLevelBatch(const Plan& p, size_t level, uint32_t batch, uint32_t arenaFloats);
    bool batchEligible(const Plan& p, size_t nOut, bool oneBlock = false) const;
    bool specReady(const Plan& p) const;
    // background mode: the one-off shapes of the current plan are queued for compilation (behind everything else) once the plan
    // has rendered `lonelyBlocks` blocks and has been current for `lonelyMs` — a plan a live graph replaces 30 ms later never
    // gets there, a static patch does within its first second (plan.cpp "deferred")
    void promoteDeferredShapes();
    int lonelyBlocks = 64, lonelyMs = 30;  // options "spec_lonely_blocks", "spec_lonely_ms"
    int maxShapeLaunches = 6;              // option "max_shape_launches": specialised launches per level (the shapes with the most islands); the rest -> one interpreter launch
    uint64_t islandBlocksSpec = 0, islandBlocksInterp = 0;   // island x block units rendered by specialised / interpreter kernels (describe_plan)
    bool anyRootRuns(const std::vector<int32_t>& rootIds, size_t nOut) const;   // host mirror of spec_root_running (Core.h:28-31, GraphRenderSequence.h:214-219)
    void mirrorRootFades(const Plan& p, uint32_t n, uint32_t nOut, uint32_t nIn);
    int  setGlobalsFor(size_t nIn, size_t nOut, size_t n, int64_t sampleTime);
    void setInRing(const float* ring, uint32_t blocks);
    std::shared_ptr<Plan> buildPlan(std::unique_lock<std::mutex>& renderLock);
    int debugBuildDelayMs = 0;
};

// The specialised-kernel variant of one island's program (plan_island.cpp builds it, codegen.cpp turns it into text).
struct SpecProgram {
    std::vector<Member> members;           // same indexing as the interpreter's tables
    std::vector<uint32_t> operands;
    std::vector<uint8_t> gdirect;          // per task: a recurrence that streams its block straight to the arena
    std::vector<uint32_t> phaseOp;         // per member: waveform tasks of streamed oscillators read the phase from here
    std::vector<uint32_t> hbmTab;          // absolute arena indices named by the variant (appended to the island's blob)
};

// plan.cpp
struct Plan {
    std::vector<Island> islands;
    std::vector<uint32_t> levelIslands;
    std::vector<uint32_t> levelOffsets;    // numLevels + 1
    std::vector<uint32_t> levelLdsBytes;
    std::vector<uint32_t> prog;            // program blobs of the islands THIS build scheduled (staging for the heap upload)
    std::shared_ptr<ProgHeap> progHeap;    // Island::progBegin is an offset into it
    std::vector<std::shared_ptr<IslandProgram>> islandProg;   // per island (null: convolve / call-out islands)
    size_t progDwordsTotal = 0;            // all islands' programs (sizes the next heap)
    size_t heapOverflowDwords = 0;         // build failed: the heap lacked room for this many dwords
    uint32_t numTasks = 0, numMembers = 0, numOperands = 0;
    std::vector<RootEntry> roots;
    std::vector<TapEntry> taps;
    int packedRootChannels = 0;                              // > 0: islands of different roots share workgroups; a call must ask for at least this many outputs
    bool tapsInSets = true;                                  // every tapIn / tapOut pair sits in one island: launch sets may render this plan (plan.cpp)
    std::vector<std::pair<int32_t, int32_t>> tapPairs;       // (tapIn node id, id of the in-island tapOut whose private buffer it reads inside a launch set, or 0)
    std::vector<std::pair<int32_t, int32_t>> eventNodes;   // (node id, owning root id) of meter / snapshot nodes, render order
    std::vector<ConvDesc> convs;           // convolve nodes (conv.hip)
    std::vector<int32_t> convNodeIds;      // ... and their node ids (same order)
    std::vector<uint32_t> convWork;        // conv workgroups, level-major
    std::vector<uint32_t> convLevelOffsets; // numLevels + 1
    std::vector<int32_t> rootIds;          // same order as `roots`
    std::vector<uint32_t> islandLevel;     // launch level of each island
    std::vector<int32_t> islandRoot;       // node id of the root whose sequence owns the island (packed islands: of the head island)
    std::vector<std::vector<int32_t>> restRoots;   // per level: the roots that own the islands of the interpreter launch (launchLevelBatch skips idle launches)
    mutable std::vector<int32_t> nodeIds;  // every node the render sequence references (gc); sorted by the first holdsNode (gc is rare, a build is not)
    mutable bool nodeIdsSorted = false;
    bool holdsNode(int32_t id) const {
        if (!nodeIdsSorted) { std::sort(nodeIds.begin(), nodeIds.end()); nodeIdsSorted = true; }
        return std::binary_search(nodeIds.begin(), nodeIds.end(), id);
    }
    std::vector<int32_t> mcCaptureIds;     // mc.capture nodes of the sequence (their rings are re-made when it is pushed: Engine::commit)
    double buildUs[6] = {0, 0, 0, 0, 0, 0}; // where the build went: render order, islands, island programs, levels + roots, shapes + tables, upload
    uint32_t numHbmBuffers = kMaxHostIn;       // per block of a launch set: host inputs + exports
    uint32_t numStreamBuffers = 0;             // per slice of the stream ring (specialised kernels; device.h kOpStream)
    uint32_t maxCopies = 1;                    // most buffer sets an island of the plan keeps in flight = slices of the stream ring
    uint32_t packK = 1;                        // islands merged per workgroup by the lane-packing step (1 = none were)
    uint32_t maxLdsBytes = 0;
    // device copies
    DevBuf dev;                            // one allocation holding all tables (from / back to `pool`)
    std::shared_ptr<TablePool> pool;
    PlanView view{};
    // host call-out nodes (OP_HOST): rendered on the CPU after the kernels of their launch level
    struct HostDesc {
        int32_t nodeId; int32_t rootId;
        struct In { int kind; uint32_t idx; float value; };   // 0 zero, 1 HBM arena buffer, 2 constant, 3 host input channel idx
        std::vector<In> inputs;
        bool leaf = false;         // no inlets: the node reads the host input channels (GraphRenderSequence.h:107-141)
        uint32_t outHbm; uint32_t level; bool active;
    };
    std::vector<HostDesc> hosts;
    // specialised kernels (jit.cpp): islands of one launch level with the same generated program text share a kernel
    struct SpecShape {
        std::shared_ptr<SpecEntry> entry;
        uint32_t level = 0;
        uint32_t listBegin = 0, count = 0;     // its workgroups: specLists[listBegin, listBegin + count) (island | split part << 24)
        bool stateless = false;                // no block pipeline: the launch spreads the blocks of a set over gridDim.y
        bool optional = false;                 // a one-island shape of a background-mode plan: while it compiles its island renders through
                                               // the interpreter kernel and the plan still counts as ready (Engine::specReady)
        bool deferred = false;                 // ... and its compile has not even been queued: Engine::promoteDeferredShapes does that once
                                               // the plan has rendered for a while
        std::vector<int32_t> roots;            // the roots that own its islands: when none of them runs the launch is skipped
    };
    std::vector<SpecShape> shapes;
    uint32_t deferredShapes = 0;               // shapes whose compile waits for this plan to prove that it stays (0 again once promoted)
    uint64_t blocksAtAdoption = 0;             // Engine stats' blocksRendered when this plan became the current one
    std::chrono::steady_clock::time_point adopted{};   // when it became the current plan
    std::vector<uint32_t> specLists;           // island indices, shape-major
    std::vector<uint32_t> restIslands;         // per level: the levelIslands entries no shape covers (interpreter launch)
    std::vector<uint32_t> restOffsets;         // numLevels + 1
    std::vector<std::shared_ptr<SpecText>> specText;   // per island: generated text (null = interpreter only), consumed by buildPlan
    const uint32_t* dSpecLists = nullptr;      // device copies (inside `dev`)
    const uint32_t* dRestIslands = nullptr;
    // captured launch sequence for multi-block offline rendering
    hipGraphExec_t graphExec = nullptr;
    int graphBlocks = 0;
    uint32_t blockChunks = 0;               // block-at-a-time chunks rendered before the capture
    ~Plan();
};

// The record writers both the render path (setTapSlice) and the control plane call: inline, so that neither pays a call across units.
inline void Engine::writeRec(uint32_t rec, uint32_t dword, uint32_t value) {
    const uint32_t idx = rec * kRecDwords + dword;
    shadow[idx] = value;
    if (!freshFlag[rec]) patches.push_back(Patch{0u, idx, value, 0u});
}

inline void Engine::writeParam(Node& n, uint32_t dword, uint32_t value) {
    const uint32_t idx = n.rec * kRecDwords + dword;
    shadow[idx] = value;
    // a record that has not been uploaded yet travels whole; otherwise patch the one dword
    if (!freshFlag[n.rec])
        patches.push_back(Patch{0u, idx, value, 0u});
    // a multi-output node: every channel's record — except the buffer slots (P0..P2: pointer, length), which differ per
    // channel and are written by writeChannelBuffer only (two patches for one dword in one flush have no order)
    if (dword > rec::P2) for (uint32_t cr : n.chanRecs) writeRec(cr, dword, value);
}

} // namespace elemhip
