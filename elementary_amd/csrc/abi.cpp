// abi.cpp — the extern "C" surface declared in include/elemhip.h.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/elemhip.h"
#include "engine.h"
#include "launch.h"
#include "flac_encode.h"

using elemhip::Engine;
using elemhip::Value;

struct elemhip_s {
    Engine engine;
    // typed path: root ids staged by elemhip_activate_roots until the next elemhip_commit of THIS handle (any thread)
    std::mutex stagedMu;
    std::vector<int32_t> stagedRoots;
    bool haveStaged = false;
    elemhip_s(double sr, int bs, int dev) : engine(sr, bs, dev) {}
};

static std::atomic<int> g_lastCreateError{0};

extern "C" {

elemhip_t* elemhip_create(double sampleRate, int blockSize, int deviceOrdinal) {
    elemhip_s* h = new (std::nothrow) elemhip_s(sampleRate, blockSize, deviceOrdinal);
    if (!h) { g_lastCreateError = elemhip::kHipError; return nullptr; }
    if (h->engine.initError()) { g_lastCreateError = h->engine.initError(); delete h; return nullptr; }
    g_lastCreateError = 0;
    return h;
}

void elemhip_destroy(elemhip_t* h) { delete h; }
int elemhip_last_create_error(void) { return g_lastCreateError.load(); }

int elemhip_apply_instructions_json(elemhip_t* h, const char* json, size_t len) {
    if (!h || !json) return elemhip::kInvalidInstructionFormat;
    Value v;
    elemhip::JsonParser parser(json, len);
    if (!parser.parse(v)) return elemhip::kJsonParseError;
    return h->engine.apply(v);
}

static int applyOne(elemhip_t* h, Value&& instr) {
    Value batch; batch.type = Value::Array;
    batch.arr.push_back(std::move(instr));
    return h->engine.apply(batch);
}

int elemhip_create_node(elemhip_t* h, int32_t id, const char* type) {
    if (!h || !type) return elemhip::kInvalidInstructionFormat;
    Value i; i.type = Value::Array;
    i.arr = {Value::number(0), Value::number(id), Value::string(type)};
    return applyOne(h, std::move(i));
}

int elemhip_append_child(elemhip_t* h, int32_t parent, int32_t child, int32_t ch) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    Value i; i.type = Value::Array;
    i.arr = {Value::number(2), Value::number(parent), Value::number(child), Value::number(ch)};
    return applyOne(h, std::move(i));
}

int elemhip_set_property_json(elemhip_t* h, int32_t id, const char* key, const char* json, size_t len) {
    if (!h || !key || !json) return elemhip::kInvalidInstructionFormat;
    // a bare scalar is valid here, so wrap it to reuse the array parser
    std::string wrapped = "[" + std::string(json, len) + "]";
    Value v;
    elemhip::JsonParser parser(wrapped.data(), wrapped.size());
    if (!parser.parse(v) || v.arr.size() != 1) return elemhip::kJsonParseError;
    Value i; i.type = Value::Array;
    i.arr = {Value::number(3), Value::number(id), Value::string(key), v.arr[0]};
    return applyOne(h, std::move(i));
}

// ACTIVATE_ROOTS and COMMIT_UPDATES only rebuild when they share a batch (Runtime.h:172,199-205),
// so the typed path keeps the pair together: activate validates and stages the ids in the handle,
// commit sends [4,...],[5].
int elemhip_activate_roots(elemhip_t* h, const int32_t* ids, size_t n) {
    if (!h || (!ids && n)) return elemhip::kInvalidInstructionFormat;
    for (size_t i = 0; i < n; ++i) if (!h->engine.hasNode(ids[i])) return elemhip::kNodeNotFound;   // Runtime.h:386-390
    std::lock_guard<std::mutex> lock(h->stagedMu);
    h->stagedRoots.assign(ids, ids + n);
    h->haveStaged = true;
    return elemhip::kOk;
}

int elemhip_commit(elemhip_t* h) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    Value batch; batch.type = Value::Array;
    {
        std::lock_guard<std::mutex> lock(h->stagedMu);
        if (h->haveStaged) {
            Value roots; roots.type = Value::Array;
            for (int32_t id : h->stagedRoots) roots.arr.push_back(Value::number(id));
            Value a; a.type = Value::Array;
            a.arr = {Value::number(4), roots};
            batch.arr.push_back(std::move(a));
            h->haveStaged = false;
        }
    }
    Value c; c.type = Value::Array; c.arr = {Value::number(5)};
    batch.arr.push_back(std::move(c));
    return h->engine.apply(batch);
}

int elemhip_process(elemhip_t* h, const float* const* in, size_t nIn, float* const* out, size_t nOut, size_t n, int64_t st) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    return h->engine.process(in, nIn, out, nOut, n, st);
}

int elemhip_process_blocks(elemhip_t* h, const float* inDev, size_t nIn, float* outDev, size_t nOut, size_t numBlocks, int64_t st) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    return h->engine.processBlocks(inDev, nIn, outDev, nOut, numBlocks, st);
}

int elemhip_process_blocks_host(elemhip_t* h, const float* const* in, size_t nIn, float* const* out, size_t nOut, size_t numFrames, int64_t st) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    return h->engine.processBlocksHost(in, nIn, out, nOut, numFrames, st);
}

int elemhip_process_blocks_pcm(elemhip_t* h, const float* const* in, size_t nIn, void* const* streams, size_t nStreams, float* const* planar,
                               size_t numFrames, int64_t st, const elemhip_pcm_spec* spec, elemhip_pcm_channel_stats* stats) {
    if (!h || !spec) return elemhip::kInvalidInstructionFormat;
    static_assert(sizeof(elemhip_pcm_channel_stats) == sizeof(Engine::PcmChannelStats) && sizeof(elemhip_pcm_spec) == sizeof(Engine::PcmSpec), "same layout");
    const Engine::PcmSpec sp{spec->format, spec->channels_per_stream, spec->dither, spec->seed};
    return h->engine.noiseShapeAfter(h->engine.processBlocksPcm(in, nIn, streams, nStreams, planar, numFrames, st, sp, reinterpret_cast<Engine::PcmChannelStats*>(stats)));
}

int elemhip_process_blocks_pcm_io(elemhip_t* h, const void* const* inStreams, size_t nInStreams, const elemhip_pcm_in_spec* inSpec,
                                  void* const* outStreams, size_t nOutStreams, const elemhip_pcm_spec* outSpec, float* const* planar, size_t nPlanar,
                                  size_t numFrames, int64_t st, elemhip_pcm_channel_stats* stats) {
    if (!h || (nInStreams && (!inSpec || !inStreams))) return elemhip::kInvalidInstructionFormat;
    const Engine::PcmSource src{inSpec ? inSpec->format : 0u, inSpec ? inSpec->channels_per_stream : 0u, inStreams, nInStreams};
    Engine::PcmSpec sp{};
    if (outSpec) sp = Engine::PcmSpec{outSpec->format, outSpec->channels_per_stream, outSpec->dither, outSpec->seed};
    return h->engine.noiseShapeAfter(h->engine.processBlocksPcmIo(src, outStreams, nOutStreams, outSpec ? &sp : nullptr, planar, nPlanar, numFrames, st,
                                                                  reinterpret_cast<Engine::PcmChannelStats*>(stats)));
}

int elemhip_loudness_read(elemhip_t* h, elemhip_loudness_info* info, double* meanSquares, size_t capacity, double* truePeak, float* samplePeak) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    Engine::LoudnessInfo li{};
    const int rc = h->engine.loudnessRead(&li, meanSquares, capacity, truePeak, samplePeak);
    if (info) { info->channels = li.channels; info->hop = li.hop; info->sub_blocks = li.subBlocks; info->frames = li.frames; }
    return rc;
}

int elemhip_loudness_reset(elemhip_t* h) { return h ? h->engine.loudnessReset() : elemhip::kInvalidInstructionFormat; }

int elemhip_resample_frames(elemhip_t* h, size_t numFrames, size_t* out) { return h ? h->engine.resampleFrames(numFrames, out) : elemhip::kInvalidInstructionFormat; }

int elemhip_resample_read(elemhip_t* h, elemhip_resample_info* info) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    Engine::ResampleInfo ri{};
    const int rc = h->engine.resampleRead(&ri);
    if (info && rc == elemhip::kOk) {
        info->up = ri.up; info->down = ri.down; info->taps = ri.taps; info->latency_frames = ri.latencyFrames;
        info->frames_in = ri.framesIn; info->frames_out = ri.framesOut;
    }
    return rc;
}

int elemhip_resample_reset(elemhip_t* h) { return h ? h->engine.resampleReset() : elemhip::kInvalidInstructionFormat; }

int elemhip_input_resample_frames(elemhip_t* h, size_t numFrames, size_t* out) { return h ? h->engine.inputResampleFrames(numFrames, out) : elemhip::kInvalidInstructionFormat; }

int elemhip_input_resample_read(elemhip_t* h, elemhip_resample_info* info) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    Engine::ResampleInfo ri{};
    const int rc = h->engine.inputResampleRead(&ri);
    if (info && rc == elemhip::kOk) {
        info->up = ri.up; info->down = ri.down; info->taps = ri.taps; info->latency_frames = ri.latencyFrames;
        info->frames_in = ri.framesIn; info->frames_out = ri.framesOut;
    }
    return rc;
}

int elemhip_input_resample_reset(elemhip_t* h) { return h ? h->engine.inputResampleReset() : elemhip::kInvalidInstructionFormat; }

int elemhip_limiter_read(elemhip_t* h, elemhip_limiter_info* info, double* maxReduction, uint64_t* limitedFrames, size_t capacity) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    Engine::LimiterInfo li{};
    const int rc = h->engine.limiterRead(&li, maxReduction, limitedFrames, capacity);
    if (info && rc == elemhip::kOk) {
        info->lookahead_frames = li.lookaheadFrames; info->latency_frames = li.latencyFrames; info->release_frames = li.releaseFrames;
        info->link = li.link; info->groups = li.groups; info->reserved = 0u; info->frames = li.frames;
    }
    return rc;
}

int elemhip_limiter_reset(elemhip_t* h) { return h ? h->engine.limiterReset() : elemhip::kInvalidInstructionFormat; }

int elemhip_noise_shape_set(elemhip_t* h, const float* coeffs, uint32_t count) {
    return h ? h->engine.noiseShapeSet(coeffs, count) : elemhip::kInvalidInstructionFormat;
}

int elemhip_noise_shape_read(elemhip_t* h, elemhip_noise_shape_info* info, int32_t* cq, uint64_t* saturated, size_t capacity) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    Engine::NoiseShapeInfo ni{};
    const int rc = h->engine.noiseShapeRead(&ni, cq, saturated, capacity);
    if (info) { info->taps = ni.taps; info->channels = ni.channels; info->frames = ni.frames; }
    return rc;
}

int elemhip_noise_shape_reset(elemhip_t* h) { return h ? h->engine.noiseShapeReset() : elemhip::kInvalidInstructionFormat; }

size_t elemhip_noise_shape_state_bytes(void) { return sizeof(noise_shape::ChannelState); }

int elemhip_noise_shape_host(const float* coeffs, uint32_t count, uint32_t bits, int dither, uint32_t seed, uint32_t channel0, int64_t time0,
                             const float* planar, uint32_t channels, size_t stride, size_t frames, uint8_t* state, int32_t* codes) {
    namespace ns = noise_shape;
    int32_t cq[ns::kMaxTaps] = {};
    if (!ns::quantise_coeffs(coeffs, count, cq)) return elemhip::kInvalidPropertyValue;
    if (!ns::bits_ok(bits) || (channels && frames && (!planar || !codes)) || (frames > stride && channels > 1u)) return elemhip::kInvalidInstructionFormat;
    std::vector<ns::ChannelState> st(channels);
    if (state) {
        std::memcpy(st.data(), state, channels * sizeof(ns::ChannelState));           // (the caller's bytes need not be aligned)
        for (auto& s : st) for (int32_t& e : s.e) e = std::max(-ns::kErrMax, std::min(ns::kErrMax, e));      // what the recurrence itself keeps
    }
    ns::shape_host(cq, count, bits, dither != 0, seed, channel0, time0, planar, channels, stride, frames, st.data(), codes);
    if (state) std::memcpy(state, st.data(), channels * sizeof(ns::ChannelState));
    return elemhip::kOk;
}

int elemhip_spectrum_set(elemhip_t* h, const elemhip_spectrum_spec* spec) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    if (!spec) return h->engine.spectrumSet(nullptr);
    const Engine::SpectrumSpec sp{spec->size, spec->hop, spec->center, spec->bands, spec->window, spec->band_first, spec->band_count, spec->weights};
    return h->engine.spectrumSet(&sp);
}

int elemhip_spectrum_read(elemhip_t* h, elemhip_spectrum_info* info, float* out, size_t capacity, double* sums, size_t sumCapacity) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    static_assert(sizeof(elemhip_spectrum_info) == sizeof(Engine::SpectrumInfo), "same layout");
    Engine::SpectrumInfo si{};
    const int rc = h->engine.spectrumRead(&si, out, capacity, sums, sumCapacity);
    if (info) std::memcpy(info, &si, sizeof si);
    return rc;
}

int elemhip_spectrum_flush(elemhip_t* h) { return h ? h->engine.spectrumFlush() : elemhip::kInvalidInstructionFormat; }

int elemhip_spectrum_reset(elemhip_t* h) { return h ? h->engine.spectrumReset() : elemhip::kInvalidInstructionFormat; }

uint64_t elemhip_spectrum_frames(uint32_t size, uint32_t hop, int center, uint64_t n, int flushed) {
    if (!ffr::size_ok(size) || hop == 0u || hop > size) return 0u;
    const uint32_t P = center ? size / 2u : 0u;
    return flushed ? spectrum::frames_total(n, size, hop, P) : spectrum::frames_complete(n, size, hop, P);
}

int elemhip_spectrum_host(const elemhip_spectrum_spec* spec, const float* planar, uint32_t channels, size_t stride, size_t frames, uint64_t n0,
                          uint64_t j0, uint64_t j1, float* tail, double* sums, float* out) {
    if (!spec || !spec->window || !spectrum::spec_ok(spec->size, spec->hop, spec->bands, spec->band_first, spec->band_count) || (spec->bands && !spec->weights))
        return elemhip::kInvalidPropertyValue;
    if (j1 < j0 || (channels && (!tail || !sums || (frames && !planar) || (j1 > j0 && !out))) || (frames > stride && channels > 1u)) return elemhip::kInvalidInstructionFormat;
    const uint32_t S = spec->size, B = spec->bands, P = spec->center ? S / 2u : 0u;
    // every frame asked for must start within the carried frames and end within what zero padding may complete
    if (j1 > j0 && ((int64_t)(j0 * spec->hop) - (int64_t)P < (int64_t)n0 - (int64_t)(S - 1u))) return elemhip::kInvalidPropertyValue;
    std::vector<double> tw(2u * S);
    ffr::make_twiddles(S, reinterpret_cast<ffr::c2*>(tw.data()));
    std::vector<uint32_t> offset(B);
    uint32_t nw = 0;
    for (uint32_t b = 0; b < B; ++b) { offset[b] = nw; nw += spec->band_count[b]; }
    const spectrum::Plan p{S, spec->hop, P, B ? B : S / 2u + 1u, B, spec->window, tw.data(), spec->band_first, spec->band_count, offset.data(), spec->weights};
    for (uint32_t c = 0; c < channels; ++c)
        spectrum::analyse_host(p, tail + (size_t)c * (S - 1u), planar + (size_t)c * stride, frames, n0, j0, j1, out + (size_t)c * (size_t)(j1 - j0) * p.cols, sums + (size_t)c * p.cols);
    return elemhip::kOk;
}

uint64_t elemhip_spectrum_launches(void) { return elemhip::spectrum_launches(); }

static_assert(sizeof(elemhip_automation_point) == sizeof(automation::Point) && offsetof(elemhip_automation_point, value) == offsetof(automation::Point, value) &&
              offsetof(elemhip_automation_point, curve) == offsetof(automation::Point, curve), "same layout");

int elemhip_automation_set(elemhip_t* h, uint32_t channel, const elemhip_automation_point* points, size_t count) {
    if (!h || (count && !points)) return elemhip::kInvalidInstructionFormat;
    return h->engine.automationSet(channel, reinterpret_cast<const automation::Point*>(points), count);
}

int elemhip_automation_read(elemhip_t* h, uint32_t channel, elemhip_automation_info* info, elemhip_automation_point* points, size_t capacity) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    Engine::AutomationInfo ai{};
    const int rc = h->engine.automationRead(channel, &ai, reinterpret_cast<automation::Point*>(points), capacity);
    if (info) { info->lanes = ai.lanes; info->inputs = ai.inputs; info->count = ai.count; }
    return rc;
}

int elemhip_automation_reset(elemhip_t* h) { return h ? h->engine.automationReset() : elemhip::kInvalidInstructionFormat; }

int elemhip_automation_host(const elemhip_automation_point* points, size_t count, int64_t t0, size_t n, float* out) {
    const automation::Point* p = reinterpret_cast<const automation::Point*>(points);
    if (!automation::lane_ok(p, count)) return elemhip::kInvalidPropertyValue;
    if (n && !out) return elemhip::kInvalidInstructionFormat;
    automation::value_host(p, count, t0, n, out);
    return elemhip::kOk;
}

int64_t elemhip_automation_segment_at(const elemhip_automation_point* points, size_t count, int64_t t) {
    return automation::segment_at(reinterpret_cast<const automation::Point*>(points), points ? count : 0, t);
}

uint64_t elemhip_automation_launches(void) { return elemhip::automation_launches(); }

int elemhip_qc_set(elemhip_t* h, const elemhip_qc_spec* spec) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    if (!spec) return h->engine.qcSet(nullptr);
    const Engine::QcSpec sp{spec->silence_level, spec->clip_level, spec->clip_run, spec->dropout_frames, spec->bucket, spec->num_pairs, spec->pairs, spec->skip, spec->limit};
    return h->engine.qcSet(&sp);
}

int elemhip_qc_read(elemhip_t* h, elemhip_qc_info* info, elemhip_qc_channel* channels, size_t channelCapacity, double* pairSums, size_t pairCapacity) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    static_assert(sizeof(elemhip_qc_info) == sizeof(Engine::QcInfo) && sizeof(elemhip_qc_channel) == sizeof(qc::ChannelReport), "same layout");
    Engine::QcInfo qi{};
    const int rc = h->engine.qcRead(&qi, reinterpret_cast<qc::ChannelReport*>(channels), channelCapacity, pairSums, pairCapacity);
    if (info) std::memcpy(info, &qi, sizeof qi);
    return rc;
}

int elemhip_qc_overview(elemhip_t* h, float* out, size_t capacity) { return h ? h->engine.qcOverview(out, capacity) : elemhip::kInvalidInstructionFormat; }

int elemhip_qc_reset(elemhip_t* h) { return h ? h->engine.qcReset() : elemhip::kInvalidInstructionFormat; }

size_t elemhip_qc_state_bytes(uint32_t channels, uint32_t numPairs) { return (size_t)channels * sizeof(qc::ChannelState) + (size_t)numPairs * sizeof(qc::PairState); }

int elemhip_qc_host(const elemhip_qc_spec* spec, const float* planar, uint32_t channels, size_t stride, size_t frames, uint64_t p0, uint8_t* state,
                    elemhip_qc_channel* reports, double* pairSums, float* overview) {
    if (!spec || !qc::spec_ok(spec->silence_level, spec->clip_level, spec->clip_run, spec->dropout_frames, spec->bucket, spec->num_pairs) || (spec->num_pairs && !spec->pairs))
        return elemhip::kInvalidPropertyValue;
    for (uint32_t k = 0; k < spec->num_pairs; ++k)
        if (spec->pairs[2u * k] == spec->pairs[2u * k + 1u] || spec->pairs[2u * k] >= channels || spec->pairs[2u * k + 1u] >= channels) return elemhip::kInvalidPropertyValue;
    if (!state || (frames && !planar) || (frames > stride && channels > 1u) || frames > 0xFFFFFFFFull) return elemhip::kInvalidInstructionFormat;
    const qc::Spec sp{spec->silence_level, spec->clip_level, spec->clip_run, spec->dropout_frames, spec->bucket, spec->num_pairs};
    const uint32_t buckets = qc::buckets_complete(p0, (uint32_t)frames, sp.bucket);
    if (buckets && !overview) return elemhip::kInvalidInstructionFormat;
    // (the state is bytes to the caller: worked on in aligned copies)
    std::vector<qc::ChannelState> st(channels);
    std::vector<qc::PairState> ps(spec->num_pairs);
    if (channels) std::memcpy(st.data(), state, channels * sizeof(qc::ChannelState));
    if (spec->num_pairs) std::memcpy(ps.data(), state + channels * sizeof(qc::ChannelState), spec->num_pairs * sizeof(qc::PairState));
    if (p0 == 0u) { for (auto& s : st) s = qc::state_empty(); for (auto& p : ps) p = qc::PairState{0.0, 0.0}; }
    for (uint32_t c = 0; c < channels; ++c) qc::channel_host(sp, st[c], planar + (size_t)c * stride, frames, p0, overview ? overview + (size_t)c * buckets * 2u : nullptr);
    for (uint32_t k = 0; k < spec->num_pairs; ++k)
        qc::pair_host(ps[k], planar + (size_t)spec->pairs[2u * k] * stride, planar + (size_t)spec->pairs[2u * k + 1u] * stride, frames, p0, sp);
    if (channels) std::memcpy(state, st.data(), channels * sizeof(qc::ChannelState));
    if (spec->num_pairs) std::memcpy(state + channels * sizeof(qc::ChannelState), ps.data(), spec->num_pairs * sizeof(qc::PairState));
    for (uint32_t c = 0; c < channels && reports; ++c) { const qc::ChannelReport r = qc::report(sp, st[c]); std::memcpy(reports + c, &r, sizeof r); }
    for (uint32_t k = 0; k < spec->num_pairs && pairSums; ++k) pairSums[k] = qc::sums_value(ps[k]);
    return elemhip::kOk;
}

uint64_t elemhip_qc_launches(void) { return elemhip::qc_launches(); }

int elemhip_process_blocks_flac(elemhip_t* h, const void* const* inStreams, size_t nInStreams, const elemhip_pcm_in_spec* inSpec,
                                void* const* outStreams, const size_t* capacities, size_t* bytesOut, size_t nOutStreams, const elemhip_flac_spec* spec,
                                size_t numFrames, int64_t st, elemhip_pcm_channel_stats* stats) {
    if (!h || !spec || (nInStreams && (!inStreams || !inSpec))) return elemhip::kInvalidInstructionFormat;
    static_assert(sizeof(elemhip_flac_spec) == sizeof(Engine::FlacSpec), "same layout");
    const Engine::PcmSource src{nInStreams ? inSpec->format : 0u, nInStreams ? inSpec->channels_per_stream : 0u, inStreams, nInStreams};
    return h->engine.noiseShapeAfter(h->engine.processBlocksFlac(src, outStreams, capacities, bytesOut, nOutStreams, *reinterpret_cast<const Engine::FlacSpec*>(spec),
                                                                 numFrames, st, reinterpret_cast<Engine::PcmChannelStats*>(stats)));
}

size_t elemhip_flac_bound(size_t frames, uint32_t channelsPerStream, uint32_t bits) { return (size_t)flac_encode::stream_bound(frames, channelsPerStream, bits); }

int elemhip_flac_flush(elemhip_t* h, void* const* outStreams, const size_t* capacities, size_t* bytesOut, size_t nOutStreams) {
    return h ? h->engine.flacFlush(outStreams, capacities, bytesOut, nOutStreams) : elemhip::kInvalidInstructionFormat;
}

int elemhip_flac_read(elemhip_t* h, elemhip_flac_info* info, elemhip_flac_stream_info* perStream, size_t capacity, uint32_t* frameBytes, size_t frameCap) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    static_assert(sizeof(elemhip_flac_stream_info) == sizeof(Engine::FlacStreamInfo), "same layout");
    Engine::FlacInfo fi{};
    const int rc = h->engine.flacRead(&fi, reinterpret_cast<Engine::FlacStreamInfo*>(perStream), capacity, frameBytes, frameCap);
    if (info) {
        info->flac_frame = fi.flacFrame; info->bits = fi.bits; info->channels_per_stream = fi.channelsPerStream; info->streams = fi.streams;
        info->sample_rate = fi.sampleRate; info->flushed = fi.flushed; info->frames = fi.frames;
    }
    return rc;
}

int elemhip_flac_reset(elemhip_t* h) { return h ? h->engine.flacReset() : elemhip::kInvalidInstructionFormat; }

int elemhip_flac_lpc_order(elemhip_t* h, uint32_t* order) {
    if (!h || !order) return elemhip::kInvalidInstructionFormat;
    *order = h->engine.flacLpcOrder();
    return elemhip::kOk;
}

int elemhip_flac_md5(elemhip_t* h, uint8_t* digests, size_t capacity, uint32_t* state) {
    return h ? h->engine.flacMd5Read(digests, capacity, state) : elemhip::kInvalidInstructionFormat;
}

size_t elemhip_flac_md5_record_bytes(void) { return sizeof(flac_md5::Record); }

int elemhip_flac_md5_init(uint8_t* record) {
    if (!record) return elemhip::kInvalidInstructionFormat;
    flac_md5::Record r;
    flac_md5::init(r);
    std::memcpy(record, &r, sizeof r);
    return elemhip::kOk;
}

int elemhip_flac_md5_update(uint8_t* record, const int32_t* const* planar, uint32_t channels, size_t frames, uint32_t bits) {
    if (!record || (frames && !planar) || channels == 0u || channels > flac_encode::kMaxChannels || !flac_md5::bits_ok(bits)) return elemhip::kInvalidInstructionFormat;
    for (uint32_t c = 0; c < channels && frames; ++c) if (!planar[c]) return elemhip::kInvalidInstructionFormat;
    flac_md5::Record r;
    std::memcpy(&r, record, sizeof r);           // (the caller's bytes need not be aligned)
    const int32_t* at[flac_encode::kMaxChannels];
    for (size_t f0 = 0; f0 < frames; f0 += (size_t)1 << 30) {       // (an update counts its frames in 32 bits)
        for (uint32_t c = 0; c < channels; ++c) at[c] = planar[c] + f0;
        flac_md5::update_codes(r, at, channels, 0u, std::min<size_t>((size_t)1 << 30, frames - f0), bits);
    }
    std::memcpy(record, &r, sizeof r);
    return elemhip::kOk;
}

int elemhip_flac_in_md5_update(uint8_t* record, const int32_t* const* planar, uint32_t channels, size_t frames, uint32_t bits) {
    namespace fi = flac_in_md5;
    if (!record || (frames && !planar) || channels == 0u || channels > fi::kMaxChannels || !fi::bits_ok(bits)) return elemhip::kInvalidInstructionFormat;
    for (uint32_t c = 0; c < channels && frames; ++c) if (!planar[c]) return elemhip::kInvalidInstructionFormat;
    flac_md5::Record r;
    std::memcpy(&r, record, sizeof r);           // (the caller's bytes need not be aligned)
    const int32_t* at[fi::kMaxChannels];
    for (size_t f0 = 0; f0 < frames; f0 += (size_t)1 << 30) {       // (an update counts its frames in 32 bits)
        for (uint32_t c = 0; c < channels; ++c) at[c] = planar[c] + f0;
        fi::update_codes(r, at, channels, 0u, std::min<size_t>((size_t)1 << 30, frames - f0), bits);
    }
    std::memcpy(record, &r, sizeof r);
    return elemhip::kOk;
}

int elemhip_flac_md5_final(const uint8_t* record, uint8_t digest[16]) {
    if (!record || !digest) return elemhip::kInvalidInstructionFormat;
    flac_md5::Record r;
    std::memcpy(&r, record, sizeof r);
    flac_md5::final(r, digest);
    return elemhip::kOk;
}

int elemhip_flac_encode(const int32_t* const* planar, uint32_t channels, size_t frames, uint32_t flacFrame, uint32_t bits, uint32_t sampleRate,
                        uint32_t firstFrameNumber, int flush, uint8_t* out, size_t capacity, size_t* bytesOut, uint32_t* frameBytes, size_t frameCap,
                        size_t* framesOut) {
    return elemhip_flac_encode_lpc(planar, channels, frames, flacFrame, bits, sampleRate, firstFrameNumber, flush, out, capacity, bytesOut, frameBytes, frameCap,
                                   framesOut, 0u);
}

int elemhip_flac_encode_lpc(const int32_t* const* planar, uint32_t channels, size_t frames, uint32_t flacFrame, uint32_t bits, uint32_t sampleRate,
                            uint32_t firstFrameNumber, int flush, uint8_t* out, size_t capacity, size_t* bytesOut, uint32_t* frameBytes, size_t frameCap,
                            size_t* framesOut, uint32_t lpcOrder) {
    namespace fe = flac_encode;
    if (!fe::lpc_order_ok(lpcOrder)) return elemhip::kInvalidPropertyValue;
    if (!fe::frame_ok(flacFrame) || !fe::bits_ok(bits) || channels == 0u || channels > fe::kMaxChannels || !bytesOut || (frames && !planar) || (capacity && !out))
        return elemhip::kInvalidInstructionFormat;
    const size_t count = frames / flacFrame + (flush && frames % flacFrame ? 1u : 0u);
    if ((uint64_t)firstFrameNumber + count > 0x80000000ull || sampleRate > 1048575u) return elemhip::kInvalidPropertyValue;
    if (frameBytes && frameCap < count) return elemhip::kInvalidPropertyValue;
    const int32_t lim = 1 << (bits - 1u);
    for (uint32_t c = 0; c < channels; ++c) {
        if (frames && !planar[c]) return elemhip::kInvalidInstructionFormat;
        for (size_t i = 0; i < frames; ++i) if (planar[c][i] < -lim || planar[c][i] >= lim) return elemhip::kInvalidPropertyValue;
    }
    size_t done = 0;
    const size_t n = fe::encode_host(planar, channels, frames, flacFrame, bits, sampleRate, firstFrameNumber, flush != 0, out, capacity, frameBytes, &done, lpcOrder);
    if (n == (size_t)-1) return elemhip::kTooManyChannels;
    *bytesOut = n;
    if (framesOut) *framesOut = done;
    return elemhip::kOk;
}

int elemhip_flac_index(const uint8_t* data, size_t bytes, uint32_t channels, uint32_t bits, uint32_t blockSize, uint64_t* frameOffsets,
                       uint64_t* frameFirstSamples, size_t capacity, size_t* entries) {
    if (!entries || (bytes && !data) || (capacity && (!frameOffsets || !frameFirstSamples))) return elemhip::kInvalidInstructionFormat;
    const uint32_t r = flac_decode::index_host(data, bytes, channels, bits, blockSize, frameOffsets, frameFirstSamples, capacity, entries);
    return r == flac_decode::OK ? elemhip::kOk : elemhip::kFlacInput;
}

int elemhip_flac_decode(const elemhip_flac_in* in, size_t count, int32_t* const* planar, size_t* badFrame, uint32_t* reason) {
    namespace fd = flac_decode;
    static_assert(sizeof(elemhip_flac_in) == sizeof(Engine::FlacIn), "same layout");
    if (reason) *reason = fd::OK;
    if (!in || !in->frame_offsets || !in->frame_first_samples || (in->bytes && !in->data) || (count && !planar)) return elemhip::kInvalidInstructionFormat;
    if (!fd::bits_ok(in->bits) || in->channels == 0u || in->channels > fd::kMaxChannels) return elemhip::kInvalidInstructionFormat;
    for (uint32_t c = 0; c < in->channels && count; ++c) if (!planar[c]) return elemhip::kInvalidInstructionFormat;
    for (uint64_t j = 0; j < in->frames; ++j)
        if (in->frame_offsets[j + 1] < in->frame_offsets[j] || in->frame_offsets[j + 1] > in->bytes || in->frame_first_samples[j + 1] <= in->frame_first_samples[j])
            return elemhip::kInvalidInstructionFormat;
    const uint32_t r = fd::decode_host(in->data, in->frame_offsets, in->frame_first_samples, (size_t)in->frames, in->channels, in->bits, in->position, count,
                                       planar, badFrame);
    if (reason) *reason = r;
    return r == fd::OK ? elemhip::kOk : elemhip::kFlacInput;
}

int elemhip_flac_in_error(elemhip_t* h, uint32_t* stream, uint64_t* frame, uint32_t* reason) {
    return h ? h->engine.flacInError(stream, frame, reason) : elemhip::kInvalidInstructionFormat;
}

int elemhip_flac_in_md5(elemhip_t* h, uint8_t* digests, uint32_t* states, uint64_t* hashed, size_t capacity, size_t* slots) {
    return h ? h->engine.flacInMd5Read(digests, states, hashed, capacity, slots) : elemhip::kInvalidInstructionFormat;
}

int elemhip_flac_in_md5_reset(elemhip_t* h) { return h ? h->engine.flacInMd5Reset() : elemhip::kInvalidInstructionFormat; }

int elemhip_loudness_gate(const double* meanSquares, size_t channels, size_t subBlocks, const double* weights, elemhip_loudness_result* out) {
    if (!out || (channels && subBlocks && !meanSquares)) return elemhip::kInvalidInstructionFormat;
    const loudness::Gated g = loudness::gate(meanSquares, channels, subBlocks, weights);
    out->integrated = g.integrated; out->momentary_max = g.momentaryMax; out->short_term_max = g.shortTermMax;
    out->blocks = g.blocks; out->gated_blocks = g.gatedBlocks;
    return elemhip::kOk;
}

int elemhip_add_shared_resource(elemhip_t* h, const char* name, const float* const* ch, size_t nCh, size_t nSamples) {
    if (!h || !name) return 0;
    return h->engine.addSharedResource(name, ch, nCh, nSamples) ? 1 : 0;
}

int elemhip_add_shared_resource_pcm(elemhip_t* h, const char* name, const elemhip_resource_src* src, int* inserted) {
    if (inserted) *inserted = 0;
    if (!h || !name || !src) return elemhip::kInvalidInstructionFormat;
    const Engine::ResourceSrc rs{src->format, src->channels, src->sample_rate, src->frames, src->data, src->bytes,
                                 reinterpret_cast<const Engine::FlacIn*>(src->flac)};
    bool done = false;
    const int rc = h->engine.addSharedResourcePcm(name, rs, &done);
    if (inserted) *inserted = done ? 1 : 0;
    return rc;
}

int elemhip_shared_resource_info(elemhip_t* h, const char* name, uint32_t* channels, uint64_t* frames) {
    return h && name ? h->engine.sharedResourceInfo(name, channels, frames) : elemhip::kInvalidInstructionFormat;
}

int elemhip_shared_resource_read(elemhip_t* h, const char* name, uint32_t channel, uint64_t first, uint64_t count, float* out) {
    return h && name ? h->engine.sharedResourceRead(name, channel, first, count, out) : elemhip::kInvalidInstructionFormat;
}

int elemhip_shared_resource_md5(elemhip_t* h, const char* name, uint8_t digest[16], uint32_t* state) {
    return h && name ? h->engine.sharedResourceMd5(name, digest, state) : elemhip::kInvalidInstructionFormat;
}

void elemhip_prune_shared_resources(elemhip_t* h) { if (h) h->engine.pruneSharedResources(); }
size_t elemhip_gc(elemhip_t* h, int32_t* out, size_t cap) { return h ? h->engine.gc(out, cap) : 0; }
size_t elemhip_last_gc(elemhip_t* h, int32_t* out, size_t cap) { return h ? h->engine.lastGc(out, cap) : 0; }
void elemhip_reset(elemhip_t* h) { if (h) h->engine.reset(); }
const char* elemhip_describe(int code) { return elemhip::describe(code); }

int elemhip_register_node_type(elemhip_t* h, const char* type, const elemhip_node_type* vt) {
    if (!h || !type || !vt) return elemhip::kInvalidInstructionFormat;
    elemhip::HostVTable t;
    t.create = vt->create; t.destroy = vt->destroy; t.setProperty = vt->set_property; t.process = vt->process; t.reset = vt->reset; t.user = vt->user;
    return h->engine.registerNodeType(type, t);
}

static size_t copyOut(const std::string& s, char* buf, size_t cap) {
    if (buf && cap) { const size_t n = s.size() < cap - 1 ? s.size() : cap - 1; std::memcpy(buf, s.data(), n); buf[n] = 0; }
    return s.size() + 1;
}
size_t elemhip_snapshot_json(elemhip_t* h, char* buf, size_t cap) { return h ? copyOut(h->engine.snapshotJson(), buf, cap) : 0; }
size_t elemhip_shared_resource_keys_json(elemhip_t* h, char* buf, size_t cap) { return h ? copyOut(h->engine.sharedResourceKeysJson(), buf, cap) : 0; }

int elemhip_process_queued_events(elemhip_t* h, elemhip_event_cb cb, void* user) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    return h->engine.processQueuedEvents(cb, user);
}

int elemhip_process_queued_events_blockwise(elemhip_t* h, elemhip_event_cb cb, void* user) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    return h->engine.processQueuedEvents(cb, user, true);
}
uint32_t elemhip_event_window_blocks(elemhip_t* h) { return h ? h->engine.eventWindowBlocks() : 0u; }

int elemhip_get_stats(elemhip_t* h, elemhip_stats* out) {
    if (!h || !out) return elemhip::kInvalidInstructionFormat;
    const elemhip::Stats& s = h->engine.stats();
    out->blocks_rendered = s.blocksRendered; out->plans_built = s.plansBuilt; out->last_plan_build_ms = s.lastPlanBuildMs;
    out->num_islands = s.numIslands; out->num_levels = s.numLevels; out->num_tasks = s.numTasks;
    out->num_nodes_in_plan = s.numNodesInPlan; out->max_lds_bytes = s.maxLdsBytes; out->num_hbm_buffers = s.numHbmBuffers;
    out->graph_replays = s.graphReplays; out->graph_captures = s.graphCaptures;
    out->batch_launches = s.batchLaunches;
    out->spec_launches = s.specLaunches; out->spec_shapes = s.specShapes; out->spec_islands = s.specIslands;
    out->last_jit_wait_ms = s.lastJitWaitMs; out->last_graph_capture_ms = s.lastGraphCaptureMs;
    out->resident_launches = s.residentLaunches; out->resident_blocks = s.residentBlocks;
    out->fft_launches = h->engine.fftLaunchCount(); out->fft_frames = h->engine.fftFrameCount();
    return elemhip::kOk;
}

int elemhip_time_launches(elemhip_t* h, size_t nOut, size_t numBlocks, float* msOut, size_t cap) {
    if (!h || !msOut) return -elemhip::kInvalidInstructionFormat;
    return h->engine.timeLaunches(nOut, numBlocks, msOut, cap);
}

int elemhip_get_launch_profile(elemhip_t* h, double* msOut, size_t cap, uint64_t* launchSets, uint64_t* blocks) {
    if (!h || !msOut) return -elemhip::kInvalidInstructionFormat;
    return h->engine.launchProfile(msOut, cap, launchSets, blocks);
}

int elemhip_trace_level(elemhip_t* h, size_t nOut, uint32_t level, unsigned long long* out, size_t cap) {
    if (!h || !out) return elemhip::kInvalidInstructionFormat;
    return h->engine.traceLevel(nOut, level, out, cap);
}

// Debug/test hook: JSON description of the current render plan. Returns bytes needed.
size_t elemhip_describe_plan(elemhip_t* h, char* buf, size_t cap) {
    if (!h) return 0;
    const std::string s = h->engine.describePlan();
    if (buf && cap) { const size_t n = s.size() < cap - 1 ? s.size() : cap - 1; std::memcpy(buf, s.data(), n); buf[n] = 0; }
    return s.size() + 1;
}

// Debug/test hook: the k-th specialised island shape of the newest plan. Returns the number of shapes (or -1);
// *state = 0 compiling, 1 ready, -1 failed; the program text / compiler log are copied when buffers are given.
int elemhip_spec_info(elemhip_t* h, size_t k, char* src, size_t srcCap, char* log, size_t logCap, int* state, uint32_t* islands) {
    if (!h) return -1;
    std::string s, l;
    const int n = h->engine.specInfo(k, src ? &s : nullptr, log ? &l : nullptr, state, islands);
    auto copy = [](const std::string& from, char* to, size_t cap) { if (to && cap) { const size_t m = from.size() < cap - 1 ? from.size() : cap - 1; std::memcpy(to, from.data(), m); to[m] = 0; } };
    copy(s, src, srcCap); copy(l, log, logCap);
    return n;
}

int elemhip_set_stream(elemhip_t* h, void* stream) {
    if (!h) return elemhip::kInvalidInstructionFormat;
    h->engine.setStream(static_cast<hipStream_t>(stream));
    return elemhip::kOk;
}

int elemhip_sum_buses(int deviceOrdinal, void* stream, float* dst, const float* const* partials, size_t nPartials, size_t nFloats) {
    if (!dst || !partials || nPartials == 0 || nPartials > 64) return elemhip::kInvalidInstructionFormat;
    if (hipSetDevice(deviceOrdinal) != hipSuccess) return elemhip::kHipError;
    if (elemhip::launch_bus_sum(static_cast<hipStream_t>(stream), dst, partials, (uint32_t)nPartials, nFloats) != hipSuccess) return elemhip::kHipError;
    return elemhip::kOk;
}

int elemhip_set_option(elemhip_t* h, const char* key, double value) {
    if (!h || !key) return elemhip::kInvalidInstructionFormat;
    return h->engine.setOption(key, value);
}

} // extern "C"
