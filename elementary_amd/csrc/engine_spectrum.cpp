// engine_spectrum.cpp — the host side of the spectrum analyser (elemhip_spectrum_set; spectrum.h, spectrum.hip): the spec and its tables,
// the carried state's and the scratch buffers' life, the queue of emitted frames, the read-out, the flush and the reset. The set loop
// that launches the kernels is renderHostSets (engine_render.cpp); the host-block renderer runs the header's scalar twin on the same state.
#include "engine_impl.h"

namespace elemhip {

void Engine::spectrumFree(bool tables) {
    for (int k = 0; k < 2; ++k) {
        if (dSpcTail[k]) (void)hipFree(dSpcTail[k]);
        if (dSpcOut[k]) (void)hipFree(dSpcOut[k]);
        if (hSpcOut[k]) (void)hipHostFree(hSpcOut[k]);
        dSpcTail[k] = dSpcOut[k] = hSpcOut[k] = nullptr;
    }
    if (dSpcSums) (void)hipFree(dSpcSums);
    dSpcSums = nullptr; spcStateCap = spcOutCap = spcOutChannels = 0; spcTailCur = 0;
    if (tables) { if (dSpcTables) (void)hipFree(dSpcTables); dSpcTables = nullptr; }
}

// a new programme of `channels` channels (0: the count is set by the first analysed call); what was not read is dropped; `mu` held
int Engine::spectrumResetLocked(size_t channels) {
    spcChannels = 0; spcFrames = spcEmitted = 0; spcFlushed = false; spcQueueFirst = 0;
    spcQueue.clear();
    if (dry || !spcOn) return kOk;
    if (hipSetDevice(device) != hipSuccess) return kHipError;
    HIP_OK(hipStreamSynchronize(stream));
    if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
    const size_t T = spcPlan.size - 1u, cols = spcPlan.cols;
    if (channels > spcStateCap) {
        for (int k = 0; k < 2; ++k) { if (dSpcTail[k]) (void)hipFree(dSpcTail[k]); dSpcTail[k] = nullptr; }
        if (dSpcSums) (void)hipFree(dSpcSums);
        dSpcSums = nullptr; spcStateCap = 0;
        for (int k = 0; k < 2; ++k) HIP_OK(hipMalloc((void**)&dSpcTail[k], channels * T * sizeof(float)));
        HIP_OK(hipMalloc((void**)&dSpcSums, channels * cols * sizeof(double)));
        spcStateCap = channels;
    }
    if (channels) {
        for (int k = 0; k < 2; ++k) HIP_OK(hipMemset(dSpcTail[k], 0, channels * T * sizeof(float)));
        HIP_OK(hipMemset(dSpcSums, 0, channels * cols * sizeof(double)));
    }
    spcTailCur = 0;
    spcChannels = (uint32_t)channels;
    spcQueue.assign(channels, std::vector<float>());
    return kOk;
}

int Engine::ensureSpectrum(size_t channels, size_t setFrames) {
    if (channels != spcChannels || spcFlushed) { const int rc = spectrumResetLocked(channels); if (rc != kOk) return rc; }
    if (setFrames > spcOutCap || (setFrames && channels > spcOutChannels)) {
        HIP_OK(hipStreamSynchronize(stream));
        if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
        const size_t ch = std::max(channels, spcOutChannels), fr = std::max(setFrames, spcOutCap), bytes = ch * fr * spcPlan.cols * sizeof(float);
        for (int k = 0; k < 2; ++k) {
            if (dSpcOut[k]) (void)hipFree(dSpcOut[k]);
            if (hSpcOut[k]) (void)hipHostFree(hSpcOut[k]);
            dSpcOut[k] = hSpcOut[k] = nullptr;
        }
        spcOutCap = spcOutChannels = 0;
        for (int k = 0; k < 2; ++k) {
            HIP_OK(hipMalloc((void**)&dSpcOut[k], bytes));
            HIP_OK(hipHostMalloc((void**)&hSpcOut[k], bytes, hipHostMallocDefault));
        }
        spcOutCap = fr; spcOutChannels = ch;
    }
    return kOk;
}

int Engine::spectrumSet(const SpectrumSpec* spec) {
    RenderGuard lock(*this);
    if (spec && (!spec->window || !spectrum::spec_ok(spec->size, spec->hop, spec->bands, spec->bandFirst, spec->bandCount) || (spec->bands && !spec->weights)))
        return kInvalidPropertyValue;
    if (!dry && (spcOn || spec)) {
        if (hipSetDevice(device) != hipSuccess) return kHipError;
        HIP_OK(hipStreamSynchronize(stream));
        if (ioStream) HIP_OK(hipStreamSynchronize(ioStream));
        spectrumFree(true);
    }
    spcOn = false;
    (void)spectrumResetLocked(0);
    spcPlan = spcPlanDev = spectrum::Plan{};
    spcWindow.clear(); spcTwiddles.clear(); spcBandIdx.clear(); spcWeights.clear();
    if (!spec) return kOk;
    const uint32_t S = spec->size, B = spec->bands;
    spcWindow.assign(spec->window, spec->window + S);
    spcTwiddles.resize(2u * S);
    ffr::make_twiddles(S, reinterpret_cast<ffr::c2*>(spcTwiddles.data()));
    spcBandIdx.resize(3u * B);
    size_t nw = 0;
    for (uint32_t b = 0; b < B; ++b) { spcBandIdx[b] = spec->bandFirst[b]; spcBandIdx[B + b] = spec->bandCount[b]; spcBandIdx[2u * B + b] = (uint32_t)nw; nw += spec->bandCount[b]; }
    spcWeights.assign(spec->weights, spec->weights + (B ? nw : 0));
    spcCenter = spec->center ? 1u : 0u;
    spcPlan.size = S; spcPlan.hop = spec->hop; spcPlan.pad = spcCenter ? S / 2u : 0u; spcPlan.bands = B; spcPlan.cols = B ? B : S / 2u + 1u;
    spcPlan.window = spcWindow.data(); spcPlan.twiddles = spcTwiddles.data();
    spcPlan.bandFirst = spcBandIdx.data(); spcPlan.bandCount = spcBandIdx.data() + B; spcPlan.bandOffset = spcBandIdx.data() + 2u * B;
    spcPlan.weights = spcWeights.data();
    spcPlanDev = spcPlan;
    if (!dry) {
        // one allocation: window | twiddles | first, count, offset | weights
        const size_t oTw = S * sizeof(double), oIdx = oTw + 2u * S * sizeof(double), oW = oIdx + ((3u * B * sizeof(uint32_t) + 15u) & ~(size_t)15u);
        const size_t bytes = oW + std::max<size_t>(nw, 1) * sizeof(float);
        HIP_OK(hipMalloc((void**)&dSpcTables, bytes));
        HIP_OK(hipMemcpy(dSpcTables, spcWindow.data(), S * sizeof(double), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(dSpcTables + oTw, spcTwiddles.data(), 2u * S * sizeof(double), hipMemcpyHostToDevice));
        if (B) HIP_OK(hipMemcpy(dSpcTables + oIdx, spcBandIdx.data(), 3u * B * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (nw) HIP_OK(hipMemcpy(dSpcTables + oW, spcWeights.data(), nw * sizeof(float), hipMemcpyHostToDevice));
        spcPlanDev.window = reinterpret_cast<const double*>(dSpcTables); spcPlanDev.twiddles = reinterpret_cast<const double*>(dSpcTables + oTw);
        spcPlanDev.bandFirst = reinterpret_cast<const uint32_t*>(dSpcTables + oIdx); spcPlanDev.bandCount = spcPlanDev.bandFirst + B;
        spcPlanDev.bandOffset = spcPlanDev.bandFirst + 2u * B; spcPlanDev.weights = reinterpret_cast<const float*>(dSpcTables + oW);
    }
    spcOn = true;
    return kOk;
}

int Engine::spectrumReset() {
    if (dry) return kNoDevice;
    RenderGuard lock(*this);
    if (!spcOn) return kInvalidPropertyValue;
    return spectrumResetLocked(0);
}

int Engine::spectrumRead(SpectrumInfo* info, float* out, size_t capacity, double* sums, size_t sumCapacity) {
    if (dry) return kNoDevice;
    RenderGuard lock(*this);
    if (!spcOn) return kInvalidPropertyValue;
    const size_t ch = spcChannels, cols = spcPlan.cols, n = ch ? spcQueue[0].size() / cols : 0;
    if (info) *info = SpectrumInfo{(uint32_t)ch, (uint32_t)cols, spcPlan.size, spcPlan.hop, spcCenter, spcPlan.bands, spcFlushed ? 1u : 0u, 0u, spcQueueFirst, n, spcEmitted, spcFrames};
    if ((out && capacity < ch * n * cols) || (sums && sumCapacity < ch * cols)) return kInvalidPropertyValue;
    if (sums && ch) {
        // (every analysed call ends with both streams synchronised; a copy: the programme may go on)
        if (hipSetDevice(device) != hipSuccess) return kHipError;
        HIP_OK(hipStreamSynchronize(stream));
        HIP_OK(hipMemcpy(sums, dSpcSums, ch * cols * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (out) {
        for (size_t c = 0; c < ch; ++c) {
            if (n) std::memcpy(out + c * n * cols, spcQueue[c].data(), n * cols * sizeof(float));
            spcQueue[c].clear();
        }
        spcQueueFirst += n;
    }
    return kOk;
}

// the frames that zero padding completes, in chunks the first half holds; the programme ends
int Engine::spectrumFlush() {
    if (dry) return kNoDevice;
    RenderGuard lock(*this);
    if (!spcOn) return kInvalidPropertyValue;
    if (spcFlushed || !spcChannels) return kOk;
    const uint64_t total = spectrum::frames_total(spcFrames, spcPlan.size, spcPlan.hop, spcPlan.pad);
    if (hipSetDevice(device) != hipSuccess) return kHipError;
    const size_t ch = spcChannels, cols = spcPlan.cols;
    const size_t chunk = (size_t)std::min<uint64_t>(std::max<uint64_t>(total - spcEmitted, 1), std::max<size_t>(kSpcHalfBytes / (ch * cols * sizeof(float)), 1));
    int rc = ensureSpectrum(ch, std::max(chunk, spcOutCap));
    while (rc == kOk && spcEmitted < total) {
        const uint32_t count = (uint32_t)std::min<uint64_t>(total - spcEmitted, spcOutCap);
        SpectrumArgs a{};
        a.src = nullptr; a.tailIn = dSpcTail[spcTailCur]; a.tailOut = nullptr; a.out = dSpcOut[0]; a.sums = dSpcSums;
        a.n0 = spcFrames; a.j0 = spcEmitted; a.numFrames = count; a.validFrames = 0u; a.blockSize = (uint32_t)blockSize; a.numChannels = (uint32_t)ch;
        a.updateTail = 0u; a.plan = spcPlanDev;
        if (launch_spectrum(stream, a) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess ||
            hipMemcpy(hSpcOut[0], dSpcOut[0], ch * count * cols * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { rc = kHipError; break; }
        for (size_t c = 0; c < ch; ++c) spcQueue[c].insert(spcQueue[c].end(), hSpcOut[0] + c * count * cols, hSpcOut[0] + (c + 1) * count * cols);
        spcEmitted += count;
    }
    if (rc != kOk) { (void)spectrumResetLocked(spcChannels); return rc; }
    spcFlushed = true;
    return kOk;
}

} // namespace elemhip
