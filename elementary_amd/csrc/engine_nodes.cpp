// engine_nodes.cpp — the instruction interpreter and the node table: node types, createNode / appendChild / setProperty,
// activateRoots, commit, apply, and the convolver's host side (setConvolverIr).
#include "engine_impl.h"
#include <complex>

#include "event_replay.h"

namespace elemhip {

// Registry: reference node-type names (DefaultNodeTypes.h:49-144, wasm/Main.cpp:47-61) -> opcode
static const std::unordered_map<std::string, uint16_t>& opTable() {
    static const std::unordered_map<std::string, uint16_t> t = {
        {"in", OP_IN}, {"sin", OP_SIN}, {"cos", OP_COS}, {"tan", OP_TAN}, {"tanh", OP_TANH}, {"asinh", OP_ASINH},
        {"ln", OP_LN}, {"log", OP_LOG}, {"log2", OP_LOG2}, {"ceil", OP_CEIL}, {"floor", OP_FLOOR}, {"round", OP_ROUND},
        {"sqrt", OP_SQRT}, {"exp", OP_EXP}, {"abs", OP_ABS},
        {"le", OP_LE}, {"leq", OP_LEQ}, {"ge", OP_GE}, {"geq", OP_GEQ}, {"pow", OP_POW}, {"eq", OP_EQ}, {"and", OP_AND}, {"or", OP_OR},
        {"add", OP_ADD}, {"sub", OP_SUB}, {"mul", OP_MUL}, {"div", OP_DIV}, {"mod", OP_MOD}, {"min", OP_MIN}, {"max", OP_MAX},
        {"root", OP_ROOT}, {"const", OP_CONST}, {"phasor", OP_PHASOR}, {"sphasor", OP_SPHASOR}, {"sr", OP_SR}, {"seq", OP_SEQ},
        {"counter", OP_COUNTER}, {"accum", OP_ACCUM}, {"latch", OP_LATCH}, {"maxhold", OP_MAXHOLD}, {"once", OP_ONCE}, {"rand", OP_RAND},
        {"delay", OP_DELAY}, {"sdelay", OP_SDELAY}, {"z", OP_Z},
        {"pole", OP_POLE}, {"env", OP_ENV}, {"biquad", OP_BIQUAD}, {"prewarp", OP_PREWARP}, {"mm1p", OP_MM1P}, {"svf", OP_SVF}, {"svfshelf", OP_SVFSHELF},
        {"tapIn", OP_TAPIN}, {"tapOut", OP_TAPOUT},
        {"blepsaw", OP_BLEPSAW}, {"blepsquare", OP_BLEPSQUARE}, {"bleptriangle", OP_BLEPTRIANGLE},
        {"mc.table", OP_TABLE}, {"mc.sample", OP_MCSAMPLE}, {"mc.sampleseq", OP_SAMPLESEQ}, {"time", OP_TIME}, {"metro", OP_METRO}, {"sampleseq", OP_SAMPLESEQ}, {"convolve", OP_CONVOLVE}, {"table", OP_TABLE}, {"seq2", OP_SEQ2}, {"sparseq2", OP_SPARSEQ2}, {"sparseq", OP_SPARSEQ}, {"capture", OP_CAPTURE}, {"mc.capture", OP_CAPTURE}, {"sample", OP_SAMPLE}, {"meter", OP_METER}, {"snapshot", OP_SNAPSHOT}, {"scope", OP_SCOPE},
        {"fft", OP_FFT},
    };
    return t;
}

// A new impulse response = a new convolver starting from silence (Convolve.h:47-51: a fresh
// TwoStageFFTConvolver per `path` assignment). Builds the conv:: state: header + IR partition spectra.
int Engine::setConvolverIr(Node& n, const ResourcePtr& res) {
    std::vector<float> h;
    if (res->numChannels()) h = resourceHost(res)[0];
    // trailing |h| < 1e-6 is dropped by the two-stage convolver as a whole and again by each of its
    // three uniform convolvers over ir[0:4096), ir[4096:8192), ir[8192:) (fftconv_oracle.h)
    size_t len = h.size();
    while (len > 0 && std::fabs(h[len - 1]) < 0.000001f) --len;
    h.resize(len);
    for (size_t lo : {(size_t)0, (size_t)4096}) {
        size_t hi = std::min(len, lo + 4096);
        while (hi > lo && std::fabs(h[hi - 1]) < 0.000001f) h[--hi] = 0.0f;
    }
    const uint32_t B = conv::kBlock, N = conv::kFft;
    const uint32_t P = (uint32_t)((len + B - 1) / B);
    const uint32_t older = P > 2 ? P - 2 : 0;
    const uint32_t S = std::min<uint32_t>(conv::kMaxSlices, std::max<uint32_t>(1, (older + conv::kSlicePartitions - 1) / conv::kSlicePartitions));
    // Long partitions (conv_long.inc): launch sets of a multiple of 8 blocks evaluate an IR of at least kLongMinP 512-partitions as
    // Q partitions of 4096 samples (8192-point spectra, G rows padded with zero rows to a multiple of the MAC's tap group) from a
    // ring of the node's last R input blocks in the time domain; both live behind `overlap`.
    constexpr uint32_t kLongMinP = 32;
    const uint32_t tapGroup = convolve_long_tap_group(), rowFloats = convolve_long_row_floats();
    const uint32_t Q = (convLong && P >= kLongMinP) ? (uint32_t)((len + 4095) / 4096) : 0u;
    const uint32_t Qp = (Q + tapGroup - 1) / tapGroup * tapGroup;
    const uint32_t R = Q ? 8u * Qp + 8u : 0u;
    const size_t words512 = conv::kHeaderDwords + 2 * ((size_t)2 * P + 2 * S + 1) * 512 + 1024;
    const size_t words = words512 + (size_t)R * 512 + (size_t)Qp * rowFloats;
    std::vector<uint32_t> blob(conv::kHeaderDwords + (size_t)P * 1024, 0u);
    blob[conv::H_P] = P; blob[conv::H_S] = S; blob[conv::H_Q] = Q; blob[conv::H_HISTBLKS] = R;
    if (++convUid == 0u) convUid = 1u;
    blob[conv::H_UID] = convUid;
    n.convQp = Qp; n.convHistBlocks = R; n.convP = P;
    convMaxQp = std::max(convMaxQp, Qp);
    convMinP = std::min(convMinP, P); convMaxP = std::max(convMaxP, P);   // (over the engine's lifetime: which MAC kernels a launch set needs)
    // IR partition spectra in double, scaled by 1/1024 (exact), rounded to float, Nyquist packed into bin 0
    std::vector<std::complex<double>> a(N), tw(N / 2);
    for (uint32_t k = 0; k < N / 2; ++k) { const double ang = -2.0 * 3.14159265358979323846 * k / N; tw[k] = {std::cos(ang), std::sin(ang)}; }
    for (uint32_t p = 0; p < P; ++p) {
        for (uint32_t i = 0; i < N; ++i) { const size_t j = (size_t)p * B + i; a[i] = (i < B && j < len) ? (double)h[j] : 0.0; }
        for (uint32_t i = 1, j = 0; i < N; ++i) {            // bit reversal
            uint32_t bit = N >> 1;
            for (; j & bit; bit >>= 1) j ^= bit;
            j ^= bit;
            if (i < j) std::swap(a[i], a[j]);
        }
        for (uint32_t m = 2; m <= N; m <<= 1)
            for (uint32_t s0 = 0; s0 < N; s0 += m)
                for (uint32_t k = 0; k < m / 2; ++k) {
                    const std::complex<double> u = a[s0 + k], t = a[s0 + k + m / 2] * tw[k * (N / m)];
                    a[s0 + k] = u + t; a[s0 + k + m / 2] = u - t;
                }
        float* dst = reinterpret_cast<float*>(blob.data() + conv::kHeaderDwords + (size_t)p * 1024);
        const double sc = 1.0 / (double)N;
        dst[0] = (float)(a[0].real() * sc); dst[1] = (float)(a[N / 2].real() * sc);
        for (uint32_t k = 1; k < N / 2; ++k) { dst[2 * k] = (float)(a[k].real() * sc); dst[2 * k + 1] = (float)(a[k].imag() * sc); }
    }
    // G_q = RFFT_8192([g_q | 0]) / 16384 in double, rounded to float: the device transforms return 16384 x the circular convolution (fft4096.h)
    std::vector<float> G((size_t)Qp * rowFloats, 0.0f);
    if (Q) {
        const uint32_t N8 = 8192;
        std::vector<std::complex<double>> a8(N8), tw8(N8 / 2);
        for (uint32_t k = 0; k < N8 / 2; ++k) { const double ang = -2.0 * 3.14159265358979323846 * k / N8; tw8[k] = {std::cos(ang), std::sin(ang)}; }
        for (uint32_t q = 0; q < Q; ++q) {
            for (uint32_t i = 0; i < N8; ++i) { const size_t j = (size_t)q * 4096 + i; a8[i] = (i < 4096 && j < len) ? (double)h[j] : 0.0; }
            for (uint32_t i = 1, j = 0; i < N8; ++i) {            // bit reversal
                uint32_t bit = N8 >> 1;
                for (; j & bit; bit >>= 1) j ^= bit;
                j ^= bit;
                if (i < j) std::swap(a8[i], a8[j]);
            }
            for (uint32_t m = 2; m <= N8; m <<= 1)
                for (uint32_t s0 = 0; s0 < N8; s0 += m)
                    for (uint32_t k = 0; k < m / 2; ++k) {
                        const std::complex<double> u = a8[s0 + k], t = a8[s0 + k + m / 2] * tw8[k * (N8 / m)];
                        a8[s0 + k] = u + t; a8[s0 + k + m / 2] = u - t;
                    }
            float* dst = G.data() + (size_t)q * rowFloats;
            for (uint32_t k = 0; k <= N8 / 2; ++k) { dst[2 * k] = (float)(a8[k].real() / 16384.0); dst[2 * k + 1] = (float)(a8[k].imag() / 16384.0); }
        }
    }
    int rc = allocRing(n, words);
    if (rc != kOk) return rc;
    const size_t gOff = (words512 + (size_t)R * 512) * 4;       // bytes: header + 512-partition state + input ring
    if (dry) { std::memcpy(n.ring.ptr, blob.data(), blob.size() * 4); if (Q) std::memcpy((char*)n.ring.ptr + gOff, G.data(), G.size() * 4); }
    else {
        HIP_OK(hipMemcpy(n.ring.ptr, blob.data(), blob.size() * 4, hipMemcpyHostToDevice));
        if (Q) HIP_OK(hipMemcpy((char*)n.ring.ptr + gOff, G.data(), G.size() * 4, hipMemcpyHostToDevice));
    }
    writeParamPtr(n, rec::CONV_STATE, n.ring.ptr);
    if (n.convSlices != S) { n.convSlices = S; planStale = true; }
    return kOk;
}

// ---- instructions ------------------------------------------------------------------------------
int Engine::createNode(int32_t id, const std::string& type) {   // Runtime.h:293-313
    auto ht = hostTypes.find(type);
    if (ht != hostTypes.end()) {               // a registered call-out type (Runtime.h:480-487)
        if (nodes.find(id) != nodes.end()) return kNodeAlreadyExists;
        Node n;
        n.id = id; n.op = OP_HOST; n.rec = allocRec();
        n.hostVt = ht->second.get();
        n.hostInst = n.hostVt->create ? n.hostVt->create(id, sampleRate, blockSize, n.hostVt->user) : nullptr;
        nodes.emplace(id, std::move(n));
        return kOk;
    }
    auto it = opTable().find(type);
    if (it == opTable().end()) return kUnknownNodeType;
    if (nodes.find(id) != nodes.end()) return kNodeAlreadyExists;
    Node n;
    n.id = id; n.op = it->second; n.rec = allocRec();
    n.mc = type.compare(0, 3, "mc.") == 0;
    uint32_t* r = shadow.data() + (size_t)n.rec * kRecDwords;
    switch (n.op) {
        case OP_CONST: r[rec::P0] = fbits(1.0f); break;                           // Core.h:166
        case OP_SR:    r[rec::P0] = fbits((float)sampleRate); break;              // Core.h:178
        case OP_IN:    r[rec::P0] = 0u; break;                                    // Math.h:125
        case OP_ROOT: {                                                           // Core.h:80-82
            n.gain = 0.0f; n.target = 1.0f; n.channel = -1;
            n.inStep = (float)msToStep(sampleRate, 20);
            n.outStep = (float)((double)(-1.0f) * msToStep(sampleRate, 20));
            n.step = (n.gain > n.target) ? n.outStep : n.inStep;
            r[rec::ROOT_CHANNEL] = (uint32_t)-1; r[rec::ROOT_TARGET] = fbits(n.target);
            r[rec::ROOT_STEP] = fbits(n.step); r[rec::ROOT_GAIN] = fbits(n.gain);
            break;
        }
        case OP_MAXHOLD: r[rec::P0] = 0xFFFFFFFFu; break;                         // Core.h:336
        case OP_SEQ:     r[rec::SEQ_HOLD] = 0; r[rec::SEQ_LOOP] = 1; break;       // Core.h:566-568
        case OP_SEQ2:    r[rec::SEQ_HOLD] = 0; r[rec::SEQ_LOOP] = 1; break;       // Seq2.h:157-159
        case OP_SPARSEQ:                                                          // SparSeq.h:340-368: edgeCount = -1, no loop points, no held event
            r[rec::SQ_EDGES] = (uint32_t)-1; r[rec::SQ_HOLD] = (uint32_t)-1;
            r[rec::SQ_LOOP_START] = r[rec::SQ_LOOP_END] = (uint32_t)-1;
            break;
        case OP_SCOPE:   // Analyzers.h:142-149: ringBuffer(4) of 8192 frames, channels = 1, size = 512
            n.props["channels"] = Value::number(1.0); n.props["size"] = Value::number(analyzerDefaultSize(OP_SCOPE));
            break;
        case OP_FFT:     // wasm/FFT.h:18-25: ringBuffer(1) of 8192 frames, size = 1024
            n.props["size"] = Value::number(analyzerDefaultSize(OP_FFT));
            break;
        case OP_SAMPLE:  // VariablePitchLerpReader(float sampleRate, ...): gainSmoothAlpha(1.0 - exp(-1.0 / (0.01 * sampleRate))), Sample.h:163
            r[rec::SMP_ALPHA] = fbits((float)(1.0 - std::exp(-1.0 / (0.01 * (double)(float)sampleRate)))); break;
        case OP_RAND:    r[rec::S0] = (uint32_t)std::rand(); break;               // Noise.h:42
        case OP_SAMPLESEQ:                                                        // SampleSeq.h:66-68: fade step 0.02
            r[rec::SSQ_PREV] = r[rec::SSQ_NEXT] = 0xFFFFFFFFu;
            r[rec::SSQ_READER0 + 2] = fbits(0.02f); r[rec::SSQ_READER0 + rec::SSQ_READER_DWORDS + 2] = fbits(0.02f);
            if (n.mc) {   // mc/SampleSeq.h:96: readers({MCBufferReader<float>(sr, 8.0), ...}) -> elem::GainFade(sr, 8 ms, 8 ms)
                const double fs = (double)(float)sampleRate;
                const float inS = (float)msToStep(fs, 8.0), outS = (float)((double)(-1.0f) * msToStep(fs, 8.0));
                r[rec::SSQ_FLAGS] = 4u;
                r[rec::SSQ_READER0 + 7] = fbits(inS); r[rec::SSQ_READER0 + rec::SSQ_READER_DWORDS + 7] = fbits(outS);
                r[rec::SSQ_READER0 + 2] = fbits(inS); r[rec::SSQ_READER0 + rec::SSQ_READER_DWORDS + 2] = fbits(inS);   // updateCurrentStep at rest
            }
            break;
        case OP_MCSAMPLE: writeParamF64(n, rec::MCS_RATE, 1.0); break;            // mc/Sample.h:162-164: playbackRate = 1.0
        case OP_METRO:                                                            // wasm/Metro.h:15
            writeParamI64(n, rec::P0, (int64_t)std::max(2.0, 1000.0 * 0.001 * sampleRate));
            n.props["interval"] = Value::number(1000.0);
            break;
        default: break;
    }
    auto ins = nodes.emplace(id, std::move(n));
    Node& nn = ins.first->second;
    int rc = kOk;
    if (nn.op == OP_DELAY || nn.op == OP_SDELAY) {                                // Delays.h:56, 183: the default size is the HOST's block
        rc = setProperty(id, "size", Value::number((double)hostBlockSize));
    } else if (nn.op == OP_TAPOUT) {                                              // Feedback.h:66-67
        rc = allocRing(nn, (size_t)blockSize);
        if (rc == kOk) writeParamPtr(nn, rec::TAP_PRIVATE, nn.ring.ptr);
        tapNodeIds.push_back(id);
    } else if (nn.op == OP_TAPIN) {
        tapNodeIds.push_back(id);
    } else if (nn.op == OP_METER || nn.op == OP_SNAPSHOT) {                       // per-block readout log (device.h EVT_LOG): 1024 entries of 4 dwords
        rc = allocRing(nn, (size_t)kEventLogEntries * 4u);
        if (rc == kOk) { writeParamPtr(nn, rec::EVT_LOG, nn.ring.ptr); writeParam(nn, rec::EVT_LOGMASK, kEventLogEntries - 1u); }
    } else if (nn.op == OP_SCOPE || nn.op == OP_FFT) {   // Analyzers.h:145: MultiChannelRingBuffer(4) x 8192; wasm/FFT.h:20: MultiChannelRingBuffer(1) x 8192
        // Option "event_history_blocks" = W: the device ring keeps W host blocks + 8192 frames. An event of the last block of a W-block
        // relay window reaches back at most 8191 frames before the window's first frame (event_replay.h), so every frame a per-block
        // relay would have handed on is still there after the window. The reference's positions stay mod 8192 (device.h SCP_MASK).
        // (a ring is kept to 2^24 frames per channel, 64 MB: a host block so long that fewer than W fit gets the window that does)
        nn.historyBlocks = (uint32_t)std::min<size_t>(eventHistoryBlocks, (((size_t)1 << 24) - evr::kRefRing) / (size_t)std::max(1, hostBlockSize));
        nn.ringFrames = nn.historyBlocks ? (uint32_t)bitceil((int)((size_t)nn.historyBlocks * (size_t)hostBlockSize + evr::kRefRing)) : evr::kRefRing;
        rc = allocRing(nn, (size_t)(nn.op == OP_SCOPE ? 4u : 1u) * nn.ringFrames);
        if (rc == kOk) { writeParamPtr(nn, rec::SCP_RING, nn.ring.ptr); writeParam(nn, rec::SCP_MASK, nn.ringFrames - 1u); }
        if (rc == kOk && nn.op == OP_FFT) rc = ensureFftTables((uint32_t)analyzerDefaultSize(OP_FFT));
    } else if (nn.op == OP_CAPTURE) {                                             // Capture.h:17: ringBuffer(1, bitceil(sr)); (mc.capture: at commit)
        // Option "capture_history_blocks" = W: the device ring keeps W host blocks of takes on top of the reference's bitceil(sr) frames
        // and a per-block log behind its last channel (device.h CAP_LOGMASK): everything a relay after every block would have drained
        // over a W-block window is still there after it. The reference's positions stay mod bitceil(sr) (CAP_REFMASK). Kept to 2^24
        // frames per channel like the scope ring.
        const size_t cap = (size_t)bitceil((int)(size_t)sampleRate), top = (size_t)1 << 24;
        nn.captureHistoryBlocks = cap >= top ? 0u : (uint32_t)std::min<size_t>(captureHistoryBlocks, (top - cap) / (size_t)std::max(1, hostBlockSize));
        nn.ringFrames = nn.captureHistoryBlocks ? (uint32_t)bitceil((int)((size_t)nn.captureHistoryBlocks * (size_t)hostBlockSize + cap)) : (uint32_t)cap;
        if (!nn.mc) {
            rc = allocRing(nn, (size_t)nn.ringFrames + captureLogFloats(nn));
            if (rc == kOk) { writeParamPtr(nn, rec::CAP_RING, nn.ring.ptr); writeCaptureRing(nn, cap); }
        }
    }
    return rc;
}

// capture / mc.capture: floats of the per-block log behind the ring's channels, and the ring's masks into the record
size_t Engine::captureLogFloats(const Node& n) const { return n.captureHistoryBlocks ? (size_t)kEventLogEntries * 4u : 0u; }
void Engine::writeCaptureRing(Node& n, size_t cap) {
    writeParam(n, rec::CAP_MASK, n.ringFrames - 1u);
    writeParam(n, rec::CAP_REFMASK, (uint32_t)(cap - 1));
    writeParam(n, rec::CAP_LOGMASK, n.captureHistoryBlocks ? kEventLogEntries - 1u : 0u);
}

int Engine::appendChild(int32_t parent, int32_t child, int32_t channel) {   // Runtime.h:335-366
    auto p = nodes.find(parent);
    if (p == nodes.end()) return kNodeNotFound;
    auto c = nodes.find(child);
    if (c == nodes.end()) return kNodeNotFound;
    p->second.inlets.push_back(Inlet{child, (uint32_t)channel});
    c->second.outlets.push_back(Outlet{parent, (uint32_t)channel});
    return kOk;
}

// A property that names a shared resource (`path`): kInvalidPropertyType unless a string, kInvalidPropertyValue unless known ...
int Engine::findResource(const Value& v, ResourcePtr& out) {
    if (!v.isString()) return kInvalidPropertyType;
    auto rit = resources.find(v.str);
    if (rit == resources.end()) return kInvalidPropertyValue;
    out = rit->second;
    return kOk;
}
// ... and the node takes it, channel 0 on the device
int Engine::bindResource(Node& n, const Value& v) {
    ResourcePtr r;
    int rc = findResource(v, r);
    if (rc == kOk) rc = ensureResourceOnDevice(r);
    if (rc == kOk) n.res = r;
    return rc;
}
static uint32_t resourceFrames(const Node& n) { return (uint32_t)n.res->frames(0); }

// `count` words into a fresh ring of the node (seq / sparseq / sparseq2 / sampleseq tables)
int Engine::uploadRing(Node& n, const void* words, size_t count) {
    int rc = allocRing(n, count);
    if (rc != kOk || !count) return rc;
    if (dry) std::memcpy(n.ring.ptr, words, count * 4);
    else HIP_OK(hipMemcpy(n.ring.ptr, words, count * 4, hipMemcpyHostToDevice));
    return kOk;
}

// sparseq2 / sampleseq `seq`: {time, value} objects -> [len doubles][len floats], sorted by time (SparSeq2.h:20-54, SampleSeq.h:181-255)
static bool timeValueTable(const Value& v, std::vector<uint32_t>& blob, size_t& len) {
    if (!v.isArray()) return false;
    std::map<double, float> events;                                 // std::map::insert keeps a key's first entry
    for (const Value& e : v.arr) {
        if (!e.isObject()) return false;
        const Value* val = e.find("value"); const Value* tm = e.find("time");
        if (!val || !tm || !val->isNumber() || !tm->isNumber()) return false;
        events.insert({tm->num, (float)val->num});
    }
    len = events.size();
    blob.assign(len * 3 + 2, 0u);
    size_t k = 0;
    for (auto& kv : events) { std::memcpy(&blob[2 * k], &kv.first, 8); std::memcpy(&blob[2 * len + k], &kv.second, 4); ++k; }
    return true;
}

int Engine::setProperty(int32_t id, const std::string& key, const Value& v) {   // Runtime.h:315-333
    auto it = nodes.find(id);
    if (it == nodes.end()) return kNodeNotFound;
    Node& n = it->second;
    if (n.op == OP_HOST) {                                         // GraphNode::setProperty of the user's node (GraphNode.h:49)
        if (n.hostVt && n.hostVt->setProperty) {
            std::string j;
            toJson(v, j);
            const int rc = n.hostVt->setProperty(n.hostInst, key.c_str(), j.c_str(), n.hostVt->user);
            if (rc != kOk) return rc;
        }
        n.props[key] = v;
        return kOk;
    }
    switch (n.op) {
        case OP_CONST:                                             // Core.h:142-152
            if (key == "value") {
                if (!v.isNumber()) return kInvalidPropertyType;
                writeParamF(n, rec::P0, (float)v.num);
            }
            break;
        case OP_IN:                                                // Math.h:95-105
            if (key == "channel") {
                if (!v.isNumber()) return kInvalidPropertyType;
                writeParam(n, rec::P0, (uint32_t)(int)v.num);
            }
            break;
        case OP_ROOT:                                              // Core.h:33-64
            if (key == "active") {
                if (!v.isBool()) return kInvalidPropertyType;
                n.target = v.b ? 1.0f : 0.0f;                      // fadeIn / fadeOut
                rootUpdateStep(n);
            }
            if (key == "channel") {
                if (!v.isNumber()) return kInvalidPropertyType;    // (reference: bad_variant_access)
                n.channel = (int)v.num;
                writeParam(n, rec::ROOT_CHANNEL, (uint32_t)n.channel);
            }
            if (key == "fadeInMs") {
                if (!v.isNumber()) return kInvalidPropertyType;
                n.inStep = (float)msToStep(sampleRate, v.num);
                rootUpdateStep(n);
            }
            if (key == "fadeOutMs") {
                if (!v.isNumber()) return kInvalidPropertyType;
                n.outStep = (float)((double)(-1.0f) * msToStep(sampleRate, v.num));
                rootUpdateStep(n);
            }
            break;
        case OP_MAXHOLD:                                           // Core.h:292-303
            if (key == "hold") {
                if (!v.isNumber()) return kInvalidPropertyType;
                const double h = sampleRate * 0.001 * v.num;
                writeParam(n, rec::P0, (uint32_t)h);
            }
            break;
        case OP_ONCE:                                              // Core.h:352-366
            if (key == "arm") {
                if (!v.isBool()) return kInvalidPropertyType;
                if (v.b) {
                    const uint32_t idx = n.rec * kRecDwords + rec::S2;
                    if (freshFlag[n.rec]) shadow[idx] = fbits(1.0f);
                    else patches.push_back(Patch{1u, idx, fbits(1.0f), 0u});
                }
            }
            break;
        case OP_SEQ2:                                              // Seq2.h:38-84 (same properties as seq)
        case OP_SEQ:                                               // Core.h:411-458
            if (key == "hold") { if (!v.isBool()) return kInvalidPropertyType; writeParam(n, rec::SEQ_HOLD, v.b ? 1u : 0u); }
            if (key == "loop") { if (!v.isBool()) return kInvalidPropertyType; writeParam(n, rec::SEQ_LOOP, v.b ? 1u : 0u); }
            if (key == "offset") {
                if (!v.isNumber()) return kInvalidPropertyType;
                if (v.num < 0.0) return kInvalidPropertyValue;
                writeParam(n, rec::SEQ_OFFSET, (uint32_t)(uint64_t)v.num);
            }
            if (key == "seq") {
                if (!v.isArray()) return kInvalidPropertyType;
                std::vector<float> data(v.arr.size());
                for (size_t i = 0; i < v.arr.size(); ++i) {
                    if (!v.arr[i].isNumber()) return kInvalidPropertyType;
                    data[i] = (float)v.arr[i].num;
                }
                int rc = uploadRing(n, data.data(), data.size());
                if (rc != kOk) return rc;
                writeParamPtr(n, rec::SEQ_PTR, n.ring.ptr);
                writeParam(n, rec::SEQ_LEN, (uint32_t)data.size());
                writeParam(n, rec::SEQ_PENDING, 1u);
            }
            break;
        case OP_RAND:                                              // Noise.h:13-23
            if (key == "seed") {
                if (!v.isNumber()) return kInvalidPropertyType;
                writeParam(n, rec::S0, (uint32_t)(int64_t)v.num);
            }
            break;
        case OP_DELAY:                                             // Delays.h:59-82
            if (key == "size") {
                if (!v.isNumber()) return kInvalidPropertyType;
                const int size = (int)v.num;
                if (size < 0) return kInvalidPropertyValue;
                int rc = allocRing(n, (size_t)size);
                if (rc != kOk) return rc;
                writeParamPtr(n, rec::RING_PTR, n.ring.ptr);
                writeParam(n, rec::RING_SIZE, (uint32_t)size);
                writeParam(n, rec::RING_RESET, 1u);
            }
            break;
        case OP_SDELAY:                                            // Delays.h:186-216
            if (key == "size") {
                if (!v.isNumber()) return kInvalidPropertyType;
                const int len = (int)v.num;
                const int size = bitceil(len + blockSize);
                if (size < 0) return kInvalidPropertyValue;
                int rc = allocRing(n, (size_t)size);
                if (rc != kOk) return rc;
                writeParamPtr(n, rec::RING_PTR, n.ring.ptr);
                writeParam(n, rec::RING_SIZE, (uint32_t)size);
                writeParam(n, rec::RING_LEN, (uint32_t)len);
                writeParam(n, rec::RING_RESET, 1u);
            }
            break;
        case OP_SVF:                                               // filters/SVF.h:30-46
            if (key == "mode") {
                if (!v.isString()) return kInvalidPropertyType;
                int m = -1;
                if (v.str == "lowpass") m = 0; if (v.str == "bandpass") m = 1; if (v.str == "highpass") m = 2;
                if (v.str == "notch") m = 3; if (v.str == "allpass") m = 4;
                if (m >= 0) writeParam(n, rec::P0, (uint32_t)m);
            }
            break;
        case OP_SVFSHELF:                                          // filters/SVFShelf.h:29-42
            if (key == "mode") {
                if (!v.isString()) return kInvalidPropertyType;
                int m = -1;
                if (v.str == "lowshelf") m = 0; if (v.str == "highshelf") m = 1;
                if (v.str == "bell" || v.str == "peak") m = 2;
                if (m >= 0) writeParam(n, rec::P0, (uint32_t)m);
            }
            break;
        case OP_MM1P:                                              // filters/MultiMode1p.h:48-62
            if (key == "mode") {
                if (!v.isString()) return kInvalidPropertyType;
                int m = -1;
                if (v.str == "lowpass") m = 0; if (v.str == "highpass") m = 2; if (v.str == "allpass") m = 4;
                if (m >= 0) writeParam(n, rec::P0, (uint32_t)m);
            }
            break;
        case OP_TAPIN: case OP_TAPOUT:                             // Feedback.h:24-38, 70-84
            if (key == "name") {
                if (!v.isString()) return kInvalidPropertyType;
                ResourcePtr r = tapResource(v.str);
                int rc = ensureResourceOnDevice(r);
                if (rc != kOk) return rc;
                n.res = r;
                writeParamPtr(n, rec::TAP_SHARED, dry ? r->dev.ptr : (const void*)(reinterpret_cast<const float*>(r->dev.ptr) + tapSliceOff));
            }
            break;
        case OP_SAMPLE:                                            // Sample.h:25-75
        case OP_MCSAMPLE:                                          // mc/Sample.h:22-76
            if (key == "path") {
                int rc = bindResource(n, v);
                if (rc != kOk) return rc;
                writeParamPtr(n, rec::SMP_BUF, n.res->dev.ptr);
                writeParam(n, rec::SMP_LEN, resourceFrames(n));
                writeParam(n, rec::SMP_PENDING, 1u);
                writeChannelBuffers(n);                            // mc.sample
            }
            if (key == "mode") {
                if (!v.isString()) return kInvalidPropertyType;
                if (v.str == "trigger") writeParam(n, rec::SMP_MODE, 0u);
                if (v.str == "gate") writeParam(n, rec::SMP_MODE, 1u);
                if (v.str == "loop") writeParam(n, rec::SMP_MODE, 2u);
            }
            if (key == "startOffset" || key == "stopOffset") {
                if (!v.isNumber()) return kInvalidPropertyType;
                const int vi = (int)v.num;
                if (vi < 0) return kInvalidPropertyValue;
                writeParam(n, key == "startOffset" ? rec::SMP_START : rec::SMP_STOP, (uint32_t)vi);
            }
            if (key == "playbackRate" && n.op == OP_MCSAMPLE) {
                if (!v.isNumber()) return kInvalidPropertyType;
                writeParamF64(n, rec::MCS_RATE, v.num);
            }
            break;
        case OP_SCOPE:                                             // Analyzers.h:151-173
            if (key == "size") { if (!v.isNumber()) return kInvalidPropertyType; if (v.num < 256 || v.num > 8192) return kInvalidPropertyValue; }
            if (key == "channels") { if (!v.isNumber()) return kInvalidPropertyType; if (v.num < 0 || v.num > 4) return kInvalidPropertyValue; }
            if (key == "name") { if (!v.isString()) return kInvalidPropertyType; }
            break;
        case OP_FFT:                                               // wasm/FFT.h:31-72 (a rejected value leaves the node as it was)
            if (key == "size") {
                if (!v.isNumber()) return kInvalidPropertyType;
                const int size = (int)v.num;
                if (size <= 0 || (size & (size - 1)) != 0 || size < 256 || size > 8192) return kInvalidPropertyValue;
                const int rc = ensureFftTables((uint32_t)size);
                if (rc != kOk) return rc;
            }
            if (key == "name") { if (!v.isString()) return kInvalidPropertyType; }
            break;
        case OP_TABLE:                                             // Table.h:20-33
            if (key == "path") {
                int rc = bindResource(n, v);
                if (rc != kOk) return rc;
                writeParamPtr(n, rec::TBL_BUF, n.res->dev.ptr);
                writeParam(n, rec::TBL_LEN, resourceFrames(n));
                writeChannelBuffers(n);                            // mc.table
            }
            break;
        case OP_SPARSEQ2:                                          // SparSeq2.h:20-54
            if (key == "seq") {
                std::vector<uint32_t> blob;
                size_t len = 0;
                if (!timeValueTable(v, blob, len)) return kInvalidPropertyType;
                int rc = uploadRing(n, blob.data(), blob.size());
                if (rc != kOk) return rc;
                writeParamPtr(n, rec::SPS_SEQ, n.ring.ptr);
                writeParam(n, rec::SPS_LEN, (uint32_t)len);
            }
            if (key == "interpolate") {
                if (!v.isNumber()) return kInvalidPropertyType;
                writeParam(n, rec::SPS_INTERP, (uint32_t)(int32_t)v.num);
            }
            break;
        case OP_SPARSEQ:                                           // SparSeq.h:40-131
            if (key == "offset") {
                if (!v.isNumber()) return kInvalidPropertyType;
                if (v.num < 0.0) return kInvalidPropertyValue;
                writeParam(n, rec::SQ_OFFSET, (uint32_t)(int32_t)(size_t)v.num);
            }
            if (key == "loop") {
                int32_t ls = -1, le = -1;
                if (!(v.type == Value::Null || (v.isBool() && !v.b))) {
                    if (!v.isArray()) return kInvalidPropertyType;
                    if (v.arr.size() < 2 || !v.arr[0].isNumber() || !v.arr[1].isNumber()) return kInvalidPropertyType;   // (the reference reads points[0], points[1] unchecked)
                    ls = (int32_t)v.arr[0].num; le = (int32_t)v.arr[1].num;
                }
                writeParam(n, rec::SQ_NEW_START, (uint32_t)ls);
                writeParam(n, rec::SQ_NEW_END, (uint32_t)le);
                writeParam(n, rec::SQ_LOOP_PENDING, 1u);
            }
            if (key == "follow") { if (!v.isBool()) return kInvalidPropertyType; writeParam(n, rec::SQ_FOLLOW, v.b ? 1u : 0u); }
            if (key == "interpolate") { if (!v.isNumber()) return kInvalidPropertyType; writeParam(n, rec::SQ_INTERP, (uint32_t)(int32_t)v.num); }
            if (key == "tickInterval") {
                if (!v.isNumber()) return kInvalidPropertyType;
                if (v.num < 0.0) return kInvalidPropertyValue;
                writeParamF64(n, rec::SQ_TICK, (double)(float)sampleRate * v.num);   // GraphNode<float>::getSampleRate() * ti
            }
            if (key == "seq") {
                if (!v.isArray()) return kInvalidPropertyType;
                std::map<int32_t, float> events;                                 // std::map::insert: the first event of a tick time stays
                for (const Value& e : v.arr) {
                    if (!e.isObject()) return kInvalidPropertyType;
                    const Value* val = e.find("value"); const Value* tm = e.find("tickTime");
                    if (!val || !tm || !val->isNumber() || !tm->isNumber()) return kInvalidPropertyType;
                    events.insert({(int32_t)tm->num, (float)val->num});
                }
                const size_t len = events.size();
                std::vector<uint32_t> blob(2 * len + 1, 0u);                     // [len int32 tick times][len floats]
                size_t k = 0;
                for (auto& kv : events) { std::memcpy(&blob[k], &kv.first, 4); std::memcpy(&blob[len + k], &kv.second, 4); ++k; }
                int rc = uploadRing(n, blob.data(), blob.size());
                if (rc != kOk) return rc;
                writeParamPtr(n, rec::SQ_SEQ, n.ring.ptr);
                writeParam(n, rec::SQ_LEN, (uint32_t)len);
                writeParam(n, rec::SQ_SEQ_PENDING, 1u);
            }
            break;
        case OP_CONVOLVE:                                          // wasm/Convolve.h:34-56
            if (key == "path") {
                ResourcePtr res;
                int rc = findResource(v, res);
                if (rc == kOk) rc = setConvolverIr(n, res);
                if (rc != kOk) return rc;
            }
            break;
        case OP_SAMPLESEQ:                                         // SampleSeq.h:181-255
            if (key == "duration") {
                if (!v.isNumber()) return kInvalidPropertyType;
                if (v.num <= 0.0) return kInvalidPropertyValue;
                writeParamF64(n, rec::SSQ_DUR, v.num);
            }
            if (key == "path") {
                int rc = bindResource(n, v);
                if (rc != kOk) return rc;
                writeParamPtr(n, rec::SSQ_BUF, n.res->dev.ptr);
                writeParam(n, rec::SSQ_BUFLEN, resourceFrames(n));
                writeParam(n, rec::SSQ_BUFPENDING, 1u);
                writeChannelBuffers(n);                            // mc.sampleseq
            }
            if (key == "seq") {
                std::vector<uint32_t> blob;
                size_t len = 0;
                if (!timeValueTable(v, blob, len)) return kInvalidPropertyType;
                int rc = uploadRing(n, blob.data(), blob.size());
                if (rc != kOk) return rc;
                writeParamPtr(n, rec::SSQ_SEQ, n.ring.ptr);
                writeParam(n, rec::SSQ_SEQLEN, (uint32_t)len);
                writeParam(n, rec::SSQ_SEQPENDING, 1u);
            }
            break;
        case OP_METRO:                                             // wasm/Metro.h:18-34
            if (key == "interval") {
                if (!v.isNumber()) return kInvalidPropertyType;
                if (0 >= v.num) return kInvalidPropertyValue;
                writeParamI64(n, rec::P0, (int64_t)std::max(2.0, v.num * 0.001 * sampleRate));
            }
            break;
        default: break;
    }
    n.props[key] = v;   // GraphNode::setProperty (GraphNode.h:108-111)
    return kOk;
}

// `malformedTail`: the id list was cut at a non-number entry. Like the reference (Runtime.h:375-380) the roots in front
// of it have been activated by then, and the call fails before anything is deactivated or swapped.
int Engine::activateRoots(const std::vector<int32_t>& ids, bool malformedTail) {   // Runtime.h:368-433
    std::set<int32_t> active;
    for (int32_t id : ids) {
        auto it = nodes.find(id);
        if (it == nodes.end()) return kNodeNotFound;
        if (it->second.op == OP_ROOT) {
            setProperty(id, "active", Value::boolean(true));
            active.insert(id);
        }
    }
    if (malformedTail) return kInvalidInstructionFormat;
    for (int32_t id : currentRoots) {
        auto it = nodes.find(id);
        if (it == nodes.end() || it->second.op != OP_ROOT) continue;
        Node& n = it->second;
        if (active.count(id) == 0) setProperty(id, "active", Value::boolean(false));
        const bool on = n.target > 0.5f;
        const bool settled = std::fabs(n.target - n.gain) <= 1e-6f;
        if (on || !settled) active.insert(id);          // stillRunning(): keep fading roots
    }
    currentRoots.swap(active);
    shouldRebuild = true;
    return kOk;
}

// `renderLock` holds `mu` on entry and on return; buildPlan releases it while it plans (the render thread keeps
// rendering the current plan meanwhile — the role of the reference's SPSC sequence queue, Runtime.h:207-216, 277-285).
int Engine::commit(std::unique_lock<std::mutex>& renderLock) {   // Runtime.h:202-206
    if (shouldRebuild || rebuildOwed || (planStale && (current || pending))) {
        planStale = false;
        auto t0 = std::chrono::steady_clock::now();
        auto p = buildPlan(renderLock);
        // (not a reference code path: its buildRenderSequence cannot fail. The roots stay swapped as in the reference;
        // the rebuild stays owed so that the next commit retries instead of rendering the old sequence forever.)
        if (!p) { rebuildOwed = true; return kUnsupportedGraph; }
        rebuildOwed = false;
        // mc.capture: the reference (re)creates the node's multi-channel ring whenever a render sequence that holds it is pushed
        // (GraphRenderSequence.h:165-169 sets `_internal:numChildren`, mc/Capture.h:21-31 allocates children - 1 channels of
        // bitceil(sr) frames): unread samples are dropped, the change detector and the relay flag live on
        bool ringsReset = false;
        for (int32_t id : p->mcCaptureIds) {
            auto it = nodes.find(id);
            if (it == nodes.end() || it->second.op != OP_CAPTURE || !it->second.mc) continue;
            Node& n = it->second;
            const size_t chans = n.inlets.size() > 1 ? n.inlets.size() - 1 : 0, cap = (size_t)bitceil((int)(size_t)sampleRate);
            if (chans == 0) continue;
            // (made under "capture_history_blocks": n.ringFrames frames per channel and the per-block log behind them, as the mono node's)
            const size_t floats = chans * (size_t)n.ringFrames + captureLogFloats(n);
            if (n.ring.bytes != floats * sizeof(float)) {
                const int rc = allocRing(n, floats);
                if (rc != kOk) return rc;
                writeParamPtr(n, rec::CAP_RING, n.ring.ptr);
                for (uint32_t cr : n.chanRecs) { writeRec(cr, rec::CAP_RING, shadow[(size_t)n.rec * kRecDwords + rec::CAP_RING]); writeRec(cr, rec::CAP_RING + 1, shadow[(size_t)n.rec * kRecDwords + rec::CAP_RING + 1]); }
            }
            writeCaptureRing(n, cap);
            writeParam(n, rec::CAP_CHANS, (uint32_t)chans);
            writeParam(n, rec::CAP_WRITE, 0u); writeParam(n, rec::CAP_READ, 0u);
            // (the device ring is addressed by CAP_ABS: back to the write position with it. A ring with history keeps counting — a
            //  relay after every block, which its relay reproduces, had drained everything before this commit.)
            if (!n.captureHistoryBlocks) { writeParam(n, rec::CAP_ABS, 0u); n.capRelayed = 0; }
            ringsReset = true;
        }
        // (the reference drops the unread samples when the sequence is PUSHED, not when it is first rendered: an event poll between
        //  this commit and the next block finds the new ring empty — the resets go to the device now, behind the blocks in flight)
        if (ringsReset && !dry) { const int rc = flushPending(); if (rc != kOk) return rc; }
        pending = p;
        shouldRebuild = false;
        st.plansBuilt++;
        st.lastPlanBuildMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return kOk;
}

int Engine::apply(const Value& batch) {   // Runtime.h:170-218
    std::lock_guard<std::mutex> control(ctl);
    std::unique_lock<std::mutex> lock(mu);
    if (!dry && hipSetDevice(device) != hipSuccess) return kHipError;
    residentStop();
    if (!batch.isArray()) return kInvalidInstructionFormat;
    shouldRebuild = false;   // a local in the reference: ACTIVATE_ROOTS and COMMIT must share a batch
    static const bool applyTiming = std::getenv("ELEMHIP_APPLY_TIMING") != nullptr;   // time per instruction kind of a batch, on stderr
    double kindUs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    struct Report {
        const double* us; bool on;
        ~Report() { if (on) std::fprintf(stderr, "[elemhip] apply: create %.1f delete %.1f append %.1f set %.1f activate %.1f commit %.1f us\n", us[0], us[1], us[2], us[3], us[4], us[5]); }
    } report{kindUs, applyTiming};
    for (const Value& next : batch.arr) {
        if (!next.isArray()) return kInvalidInstructionFormat;
        const auto& ar = next.arr;
        if (ar.empty() || !ar[0].isNumber()) return kInvalidInstructionFormat;
        const int cmd = (int)ar[0].num;
        const auto tCmd = applyTiming ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
        struct Acc {
            double* slot; std::chrono::steady_clock::time_point t0; bool on;
            ~Acc() { if (on) *slot += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); }
        } acc{&kindUs[(cmd >= 0 && cmd < 6) ? cmd : 7], tCmd, applyTiming};
        int res = kOk;
        static const Value undef;
        auto arg = [&](size_t i) -> const Value& { return i < ar.size() ? ar[i] : undef; };
        switch (cmd) {
            case 0:   // CREATE_NODE
                if (!arg(1).isNumber() || !arg(2).isString()) { res = kInvalidInstructionFormat; break; }
                res = createNode((int32_t)arg(1).num, arg(2).str);
                break;
            case 3:   // SET_PROPERTY
                if (!arg(1).isNumber() || !arg(2).isString()) { res = kInvalidInstructionFormat; break; }
                res = setProperty((int32_t)arg(1).num, arg(2).str, arg(3));
                break;
            case 2:   // APPEND_CHILD
                if (!arg(1).isNumber() || !arg(2).isNumber() || !arg(3).isNumber()) { res = kInvalidInstructionFormat; break; }
                res = appendChild((int32_t)arg(1).num, (int32_t)arg(2).num, (int32_t)arg(3).num);
                break;
            case 4: { // ACTIVATE_ROOTS
                if (!arg(1).isArray()) { res = kInvalidInstructionFormat; break; }
                std::vector<int32_t> ids;
                bool bad = false;
                for (const Value& v : arg(1).arr) { if (!v.isNumber()) { bad = true; break; } ids.push_back((int32_t)v.num); }
                // the reference activates the roots preceding a malformed id before failing
                res = activateRoots(ids, bad);
                shouldRebuild = true;
                break;
            }
            case 5:   // COMMIT_UPDATES
                res = commit(lock);
                break;
            default: break;
        }
        if (res != kOk) return res;
    }
    return kOk;
}

int Engine::registerNodeType(const std::string& type, const HostVTable& vt) {   // Runtime.h:480-487
    std::lock_guard<std::mutex> control(ctl);
    RenderGuard lock(*this);
    if (hostTypes.count(type) || opTable().count(type)) return kNodeTypeAlreadyExists;
    if (!vt.process) return kInvalidInstructionFormat;
    hostTypes.emplace(type, std::unique_ptr<HostVTable>(new HostVTable(vt)));
    return kOk;
}

} // namespace elemhip
