// elemhip/Runtime.hpp — header-only C++ façade over the C-ABI (include/elemhip.h) with the public
// surface of `elem::Runtime<float>` (runtime/elem/Runtime.h:39-153), so a host written like
// cli/Benchmark.cpp switches engines by changing the class it instantiates:
//
//     #include <elem/Runtime.h>        ->   #include <elemhip/Runtime.hpp>
//     elem::Runtime<float> rt(sr, bs); ->   elemhip::Runtime<float> rt(sr, bs);
//
// When the reference's own headers are on the include path (<elem/Value.h>, <elem/JSON.h>, <elem/GraphNode.h>) the
// façade also offers the members that speak `elem::js::Value`: applyInstructions(js::Array const&), snapshot(),
// processQueuedEvents with a js::Value payload, and registerNodeType with an unmodified `elem::GraphNode<float>`
// subclass (rendered as a CPU call-out node, see elemhip_register_node_type). Define ELEMHIP_NO_ELEM_HEADERS to
// opt out. Without them the JSON-text members below are the whole surface.
#pragma once
#include <cstdint>
#include <cstdio>
#include <functional>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../elemhip.h"

#if !defined(ELEMHIP_NO_ELEM_HEADERS) && defined(__has_include)
#if __has_include(<elem/Value.h>) && __has_include(<elem/JSON.h>) && __has_include(<elem/GraphNode.h>)
#include <array>
#include <atomic>
#include <cmath>
#include <list>
#include <map>
#include <numeric>
#include <elem/Value.h>
#include <elem/JSON.h>
#include <elem/GraphNode.h>
#define ELEMHIP_HAVE_ELEM_HEADERS 1
#endif
#endif

namespace elemhip {

#ifdef ELEMHIP_HAVE_ELEM_HEADERS
namespace detail {
// elem::js::Value -> JSON text (Value::toString is a debug print, not JSON)
inline void toJSON(elem::js::Value const& v, std::string& out) {
    if (v.isBool()) out += ((elem::js::Boolean)v) ? "true" : "false";
    else if (v.isNumber()) { char b[40]; std::snprintf(b, sizeof b, "%.17g", (double)(elem::js::Number)v); out += b; }
    else if (v.isString()) {
        out += '"';
        for (unsigned char ch : (elem::js::String)v) {
            if (ch == '"' || ch == '\\') { out += '\\'; out += (char)ch; }
            else if (ch < 0x20) { char b[8]; std::snprintf(b, sizeof b, "\\u%04x", ch); out += b; }
            else out += (char)ch;
        }
        out += '"';
    } else if (v.isArray()) {
        out += '[';
        auto const& a = v.getArray();
        for (size_t i = 0; i < a.size(); ++i) { if (i) out += ','; toJSON(a[i], out); }
        out += ']';
    } else if (v.isFloat32Array()) {
        out += '[';
        auto const& a = v.getFloat32Array();
        for (size_t i = 0; i < a.size(); ++i) { char b[40]; std::snprintf(b, sizeof b, "%s%.9g", i ? "," : "", (double)a[i]); out += b; }
        out += ']';
    } else if (v.isObject()) {
        out += '{';
        bool first = true;
        for (auto const& kv : v.getObject()) {
            if (!first) out += ',';
            first = false;
            toJSON(elem::js::Value(kv.first), out); out += ':'; toJSON(kv.second, out);
        }
        out += '}';
    } else out += "null";
}
} // namespace detail
#endif

template <typename FloatType>
class Runtime;

template <>
class Runtime<float> {
public:
    // Runtime(double sampleRate, int blockSize)                       Runtime.h:44
    Runtime(double sampleRate, int blockSize, int deviceOrdinal = 0)
        : h(elemhip_create(sampleRate, blockSize, deviceOrdinal)) {
        if (!h) throw std::runtime_error(std::string("elemhip_create: ") + elemhip_describe(elemhip_last_create_error()));
    }
    ~Runtime() { elemhip_destroy(h); }
    Runtime(Runtime const&) = delete;
    Runtime& operator=(Runtime const&) = delete;

    // int applyInstructions(js::Array const& batch)                   Runtime.h:48 — as the JSON text the
    // hosts already hold (cli/Benchmark.cpp:40-43 parses it only to hand it over)
    int applyInstructionsJSON(std::string const& batch) { return elemhip_apply_instructions_json(h, batch.data(), batch.size()); }

    // void process(const F** in, size_t nIn, F** out, size_t nOut, size_t n, void* userData)   Runtime.h:51-57
    // userData is what the reference's hosts pass: a pointer to the int64_t sample time (wasm/Main.cpp:212) or null.
    void process(const float** in, size_t nIn, float** out, size_t nOut, size_t numSamples, void* userData = nullptr) {
        const int64_t t = userData ? *static_cast<int64_t*>(userData) : implicitTime;
        (void)elemhip_process(h, in, nIn, out, nOut, numSamples, t);
        if (!userData) implicitTime += (int64_t)numSamples;
    }

    // The offline caller's block loop (js/packages/offline-renderer/index.ts:87-133) in one call: planar HOST arrays of
    // numFrames frames per channel, ceil(numFrames / blockSize) full blocks, outputs overwritten. Same userData rule as
    // process(): a pointer to the int64_t sample time of the first frame, or null for the implicit running clock.
    int processBlocks(const float** in, size_t nIn, float** out, size_t nOut, size_t numFrames, void* userData = nullptr) {
        const int64_t t = userData ? *static_cast<int64_t*>(userData) : implicitTime;
        const int rc = elemhip_process_blocks_host(h, in, nIn, out, nOut, numFrames, t);
        if (!userData) implicitTime += (int64_t)numFrames;
        return rc;
    }

    // EXTENSION (no counterpart in elem::Runtime): the same block loop delivered as interleaved PCM, packed on the GPU
    // (elemhip_process_blocks_pcm): nStreams buffers of numFrames * spec.channels_per_stream samples, stream s / sample (frame, g) =
    // output channel s * G + g; `planar` (or null) receives the floats that were packed, `stats` (or null) one entry per channel.
    int processBlocksPcm(const float** in, size_t nIn, void* const* streams, size_t nStreams, float** planar, size_t numFrames,
                         elemhip_pcm_spec const& spec, elemhip_pcm_channel_stats* stats = nullptr, void* userData = nullptr) {
        const int64_t t = userData ? *static_cast<int64_t*>(userData) : implicitTime;
        const int rc = elemhip_process_blocks_pcm(h, in, nIn, streams, nStreams, planar, numFrames, t, &spec, stats);
        if (!userData) implicitTime += (int64_t)numFrames;
        return rc;
    }

    // EXTENSION: the block loop fed with interleaved PCM, unpacked on the GPU (elemhip_process_blocks_pcm_io): nInStreams streams of
    // numFrames * inSpec.channels_per_stream samples. `outSpec` null: `planar` = nPlanar planar float arrays (processBlocksHost's
    // output); else processBlocksPcm's delivery into `outStreams`, `planar` null or the floats that were packed.
    int processBlocksPcmIo(const void* const* inStreams, size_t nInStreams, elemhip_pcm_in_spec const& inSpec, void* const* outStreams,
                           size_t nOutStreams, const elemhip_pcm_spec* outSpec, float** planar, size_t nPlanar, size_t numFrames,
                           elemhip_pcm_channel_stats* stats = nullptr, void* userData = nullptr) {
        const int64_t t = userData ? *static_cast<int64_t*>(userData) : implicitTime;
        const int rc = elemhip_process_blocks_pcm_io(h, inStreams, nInStreams, &inSpec, outStreams, nOutStreams, outSpec, planar, nPlanar,
                                                     numFrames, t, stats);
        if (!userData) implicitTime += (int64_t)numFrames;
        return rc;
    }

    // EXTENSION: the loudness meter (elemhip_loudness_read / _reset / _gate; setOption("loudness_meter", 1) turns it on): BS.1770
    // sub-block mean squares [channel][sub_blocks] and true peaks of everything processBlocksHost / processBlocksPcm /
    // processBlocksPcmIo delivered since the last reset. process() and processBlocks() are not metered.
    int loudnessRead(elemhip_loudness_info* info, double* meanSquares, size_t capacity, double* truePeak = nullptr, float* samplePeak = nullptr) {
        return elemhip_loudness_read(h, info, meanSquares, capacity, truePeak, samplePeak);
    }
    int loudnessReset() { return elemhip_loudness_reset(h); }
    // EXTENSION: delivery at another sample rate (setOption("resample_rate", hz)): the host-buffer render calls then fill
    // resampleFrames(numFrames) frames
    int resampleFrames(size_t numFrames, size_t* out) { return elemhip_resample_frames(h, numFrames, out); }
    int resampleRead(elemhip_resample_info* info) { return elemhip_resample_read(h, info); }
    int resampleReset() { return elemhip_resample_reset(h); }
    // EXTENSION: inputs at another sample rate (setOption("input_rate", hz)): numFrames of the host-buffer render calls stays in
    // engine frames, their input arrays and streams hold inputResampleFrames(numFrames) frames
    int inputResampleFrames(size_t numFrames, size_t* out) { return elemhip_input_resample_frames(h, numFrames, out); }
    int inputResampleRead(elemhip_resample_info* info) { return elemhip_input_resample_read(h, info); }
    int inputResampleReset() { return elemhip_input_resample_reset(h); }
    // EXTENSION: gain and true-peak limiter on what the host-buffer render calls deliver (setOption("limiter", 1), "limiter_*")
    int limiterRead(elemhip_limiter_info* info, double* maxReduction, uint64_t* limitedFrames, size_t capacity) {
        return elemhip_limiter_read(h, info, maxReduction, limitedFrames, capacity);
    }
    int limiterReset() { return elemhip_limiter_reset(h); }
    // EXTENSION: noise-shaped requantisation of s16 / s24 / FLAC delivery (count 0: off)
    int noiseShapeSet(const float* coeffs, uint32_t count) { return elemhip_noise_shape_set(h, coeffs, count); }
    int noiseShapeRead(elemhip_noise_shape_info* info, int32_t* cq, uint64_t* saturated, size_t capacity) {
        return elemhip_noise_shape_read(h, info, cq, saturated, capacity);
    }
    int noiseShapeReset() { return elemhip_noise_shape_reset(h); }
    // EXTENSION: STFT power or band spectra of what the host-buffer render calls deliver (null spec: off)
    int spectrumSet(const elemhip_spectrum_spec* spec) { return elemhip_spectrum_set(h, spec); }
    int spectrumRead(elemhip_spectrum_info* info, float* out, size_t capacity, double* sums, size_t sumCapacity) {
        return elemhip_spectrum_read(h, info, out, capacity, sums, sumCapacity);
    }
    int spectrumFlush() { return elemhip_spectrum_flush(h); }
    int spectrumReset() { return elemhip_spectrum_reset(h); }
    // EXTENSION: the inspector — silence, dropouts, clip events, DC, energy, pair sums and a min / max overview of what the host-buffer
    // render calls deliver (null spec: off)
    int qcSet(const elemhip_qc_spec* spec) { return elemhip_qc_set(h, spec); }
    int qcRead(elemhip_qc_info* info, elemhip_qc_channel* channels, size_t channelCapacity, double* pairSums, size_t pairCapacity) {
        return elemhip_qc_read(h, info, channels, channelCapacity, pairSums, pairCapacity);
    }
    int qcOverview(float* out, size_t capacity) { return elemhip_qc_overview(h, out, capacity); }
    int qcReset() { return elemhip_qc_reset(h); }
    // EXTENSION: breakpoint automation lanes on engine input channels of the host-buffer render calls, expanded on the GPU (count 0: cleared)
    int automationSet(uint32_t channel, const elemhip_automation_point* points, size_t count) { return elemhip_automation_set(h, channel, points, count); }
    int automationRead(uint32_t channel, elemhip_automation_info* info, elemhip_automation_point* points, size_t capacity) {
        return elemhip_automation_read(h, channel, info, points, capacity);
    }
    int automationReset() { return elemhip_automation_reset(h); }
    // EXTENSION: the block loop delivered as FLAC frames encoded on the GPU (elemhip_process_blocks_flac; setOption("flac_frame" /
    // "flac_bits")): inputs as processBlocksPcmIo takes them, per output stream a buffer of at least flacBound(frames delivered,
    // channels_per_stream, bits) bytes; bytesOut[s] = the bytes of the FLAC frames the call completed. flacFlush closes the programme
    // with the open remainder as a short frame, flacReset starts a new one.
    int processBlocksFlac(const void* const* inStreams, size_t nInStreams, elemhip_pcm_in_spec const& inSpec, void* const* outStreams,
                          const size_t* capacities, size_t* bytesOut, size_t nOutStreams, elemhip_flac_spec const& spec, size_t numFrames,
                          elemhip_pcm_channel_stats* stats = nullptr, void* userData = nullptr) {
        const int64_t t = userData ? *static_cast<int64_t*>(userData) : implicitTime;
        const int rc = elemhip_process_blocks_flac(h, inStreams, nInStreams, &inSpec, outStreams, capacities, bytesOut, nOutStreams, &spec, numFrames, t, stats);
        if (!userData) implicitTime += (int64_t)numFrames;
        return rc;
    }
    int flacFlush(void* const* outStreams, const size_t* capacities, size_t* bytesOut, size_t nOutStreams) {
        return elemhip_flac_flush(h, outStreams, capacities, bytesOut, nOutStreams);
    }
    int flacRead(elemhip_flac_info* info, elemhip_flac_stream_info* perStream, size_t capacity, uint32_t* frameBytes = nullptr, size_t frameCap = 0) {
        return elemhip_flac_read(h, info, perStream, capacity, frameBytes, frameCap);
    }
    int flacReset() { return elemhip_flac_reset(h); }
    static size_t flacBound(size_t frames, uint32_t channelsPerStream, uint32_t bits) { return elemhip_flac_bound(frames, channelsPerStream, bits); }
    static int flacEncode(const int32_t* const* planar, uint32_t channels, size_t frames, uint32_t flacFrame, uint32_t bits, uint32_t sampleRate,
                          uint32_t firstFrameNumber, bool flush, uint8_t* out, size_t capacity, size_t* bytesOut, uint32_t* frameBytes = nullptr,
                          size_t frameCap = 0, size_t* framesOut = nullptr) {
        return elemhip_flac_encode(planar, channels, frames, flacFrame, bits, sampleRate, firstFrameNumber, flush ? 1 : 0, out, capacity, bytesOut, frameBytes,
                                   frameCap, framesOut);
    }
    // ... with LPC subframes (setOption("flac_lpc_order", P), 0 .. 12): the twin of such a programme, and the order in force
    static int flacEncodeLpc(const int32_t* const* planar, uint32_t channels, size_t frames, uint32_t flacFrame, uint32_t bits, uint32_t sampleRate,
                             uint32_t firstFrameNumber, bool flush, uint8_t* out, size_t capacity, size_t* bytesOut, uint32_t lpcOrder,
                             uint32_t* frameBytes = nullptr, size_t frameCap = 0, size_t* framesOut = nullptr) {
        return elemhip_flac_encode_lpc(planar, channels, frames, flacFrame, bits, sampleRate, firstFrameNumber, flush ? 1 : 0, out, capacity, bytesOut,
                                       frameBytes, frameCap, framesOut, lpcOrder);
    }
    int flacLpcOrder(uint32_t* order) { return elemhip_flac_lpc_order(h, order); }
    // ... with the STREAMINFO MD5 computed on the GPU (setOption("flac_md5", 1)): state 0 off / no programme, 1 running, 2 final after
    // flacFlush; digests [streams][16]. The host twins digest planar codes of one stream the same way.
    int flacMd5(uint8_t* digests, size_t capacity, uint32_t* state) { return elemhip_flac_md5(h, digests, capacity, state); }
    static size_t flacMd5RecordBytes() { return elemhip_flac_md5_record_bytes(); }
    static int flacMd5Init(uint8_t* record) { return elemhip_flac_md5_init(record); }
    static int flacMd5Update(uint8_t* record, const int32_t* const* planar, uint32_t channels, size_t frames, uint32_t bits) {
        return elemhip_flac_md5_update(record, planar, channels, frames, bits);
    }
    static int flacMd5Final(const uint8_t* record, uint8_t digest[16]) { return elemhip_flac_md5_final(record, digest); }
    static int loudnessGate(const double* meanSquares, size_t channels, size_t subBlocks, const double* weights, elemhip_loudness_result* out) {
        return elemhip_loudness_gate(meanSquares, channels, subBlocks, weights, out);
    }

    // bool addSharedResource(name, unique_ptr<SharedResource>)         Runtime.h:83 — planar float channels
    bool addSharedResource(std::string const& name, const float* const* channels, size_t nCh, size_t nSamples) {
        return elemhip_add_shared_resource(h, name.c_str(), channels, nCh, nSamples) != 0;
    }
    // EXTENSION: the resource from a file's own bytes, decoded (and rate-converted) on the GPU — elemhip_add_shared_resource_pcm.
    // Returns the engine's code; *inserted false where the name is taken.
    int addSharedResourcePcm(std::string const& name, const elemhip_resource_src& src, bool* inserted = nullptr) {
        int done = 0;
        const int rc = elemhip_add_shared_resource_pcm(h, name.c_str(), &src, &done);
        if (inserted) *inserted = done != 0;
        return rc;
    }
    int sharedResourceInfo(std::string const& name, uint32_t* channels, uint64_t* frames) { return elemhip_shared_resource_info(h, name.c_str(), channels, frames); }
    int sharedResourceRead(std::string const& name, uint32_t channel, uint64_t first, uint64_t count, float* out) {
        return elemhip_shared_resource_read(h, name.c_str(), channel, first, count, out);
    }
    void pruneSharedResources() { elemhip_prune_shared_resources(h); }                    // Runtime.h:89
    std::vector<std::string> getSharedResourceMapKeys() {                                 // Runtime.h:94
        std::string j = text([&](char* b, size_t c) { return elemhip_shared_resource_keys_json(h, b, c); });
        std::vector<std::string> keys;   // a flat JSON array of strings
        size_t i = 0;
        while ((i = j.find('"', i)) != std::string::npos) {
            std::string k;
            for (++i; i < j.size() && j[i] != '"'; ++i) { if (j[i] == '\\' && i + 1 < j.size()) ++i; k += j[i]; }
            keys.push_back(k);
            ++i;
        }
        return keys;
    }
    std::string snapshotJSON() { return text([&](char* b, size_t c) { return elemhip_snapshot_json(h, b, c); }); }   // Runtime.h:110
    // processQueuedEvents with the payload as JSON text                                  Runtime.h:64
    void processQueuedEventsJSON(std::function<void(std::string const&, std::string const&)>&& cb) {
        auto tramp = [](const char* type, const char* json, void* user) {
            (*static_cast<std::function<void(std::string const&, std::string const&)>*>(user))(type, json);
        };
        elemhip_process_queued_events(h, tramp, &cb);
    }
#ifndef ELEMHIP_HAVE_ELEM_HEADERS
    void processQueuedEvents(std::function<void(std::string const&, std::string const&)>&& cb) { processQueuedEventsJSON(std::move(cb)); }
#endif
    void reset() { elemhip_reset(h); }                                                    // Runtime.h:70
    std::set<int32_t> gc() {                                                              // Runtime.h:76
        std::vector<int32_t> buf(1 << 12);
        size_t n = elemhip_gc(h, buf.data(), buf.size());
        if (n > buf.size()) { buf.resize(n); n = elemhip_last_gc(h, buf.data(), buf.size()); }
        return std::set<int32_t>(buf.begin(), buf.begin() + (long)n);
    }
    // int registerNodeType(type, NodeFactoryFn&&)                      Runtime.h:105 — C form (include/elemhip.h)
    int registerNodeType(std::string const& type, elemhip_node_type const& vt) { return elemhip_register_node_type(h, type.c_str(), &vt); }

#ifdef ELEMHIP_HAVE_ELEM_HEADERS
    // ---- the members that speak elem::js::Value (reference headers on the include path) ----
    // bool addSharedResource(std::string const& name, std::unique_ptr<SharedResource> resource)   Runtime.h:83,461-465
    // The engine copies the channels (the resource may die when this returns); insert-only like the reference.
    bool addSharedResource(std::string const& name, std::unique_ptr<elem::SharedResource> resource) {
        if (!resource) return false;
        const size_t nCh = resource->numChannels(), n = resource->numSamples();
        std::vector<const float*> chans(nCh ? nCh : 1, nullptr);
        for (size_t c = 0; c < nCh; ++c) chans[c] = resource->getChannelData(c).data();
        return addSharedResource(name, chans.data(), nCh, n);
    }
    int applyInstructions(elem::js::Array const& batch) {                                 // Runtime.h:48,170-218
        std::string j;
        detail::toJSON(elem::js::Value(batch), j);
        return applyInstructionsJSON(j);
    }
    elem::js::Object snapshot() {                                                         // Runtime.h:110
        auto v = elem::js::parseJSON(snapshotJSON());
        return v.isObject() ? v.getObject() : elem::js::Object();
    }
    void processQueuedEvents(std::function<void(std::string const&, elem::js::Value)>&& cb) {   // Runtime.h:64
        processQueuedEventsJSON([&](std::string const& type, std::string const& json) { cb(type, elem::js::parseJSON(json)); });
    }
    // registerNodeType with the reference's own factory type (Runtime.h:100-106): the node is an unmodified
    // elem::GraphNode<float> subclass, rendered as a CPU call-out between two GPU launch levels.
    using NodeFactoryFn = std::function<std::shared_ptr<elem::GraphNode<float>>(elem::NodeId const id, double sampleRate, int const blockSize)>;
    int registerNodeType(std::string const& type, NodeFactoryFn&& fn) {
        auto* holder = new Factory{std::move(fn)};   // lives as long as the engine may create nodes of the type
        factories.emplace_back(holder);
        elemhip_node_type vt{};
        vt.user = holder;
        vt.create = [](int32_t id, double sr, int bs, void* user) -> void* {
            auto node = static_cast<Factory*>(user)->fn(id, sr, bs);
            return node ? new std::shared_ptr<elem::GraphNode<float>>(std::move(node)) : nullptr;
        };
        vt.destroy = [](void* node, void*) { delete static_cast<std::shared_ptr<elem::GraphNode<float>>*>(node); };
        vt.set_property = [](void* node, const char* key, const char* json, void*) -> int {
            if (!node) return 0;
            // (elem::js::parseJSON only accepts an array or object at the top level: wrap the bare value)
            auto wrapped = elem::js::parseJSON("[" + std::string(json) + "]");
            return (*static_cast<std::shared_ptr<elem::GraphNode<float>>*>(node))->setProperty(key, wrapped.getArray().at(0));
        };
        vt.process = [](void* node, const float* const* in, size_t nIn, float* out, size_t n, int64_t sampleTime, int active, void*) {
            if (!node) return;
            int64_t t = sampleTime;
            float* outs[1] = {out};
            elem::BlockContext<float> ctx{const_cast<float const**>(in), nIn, outs, 1, n, &t, active != 0};
            (*static_cast<std::shared_ptr<elem::GraphNode<float>>*>(node))->process(ctx);
        };
        vt.reset = [](void* node, void*) { if (node) (*static_cast<std::shared_ptr<elem::GraphNode<float>>*>(node))->reset(); };
        return elemhip_register_node_type(h, type.c_str(), &vt);
    }
#endif

    elemhip_t* handle() { return h; }

private:
    template <typename F>
    static std::string text(F&& get) {
        const size_t need = get(nullptr, 0);
        std::string s(need ? need : 1, '\0');
        get(&s[0], s.size());
        s.resize(need ? need - 1 : 0);
        return s;
    }
#ifdef ELEMHIP_HAVE_ELEM_HEADERS
    struct Factory { NodeFactoryFn fn; };
    std::vector<std::unique_ptr<Factory>> factories;
#endif
    elemhip_t* h;
    int64_t implicitTime = 0;
};

} // namespace elemhip
