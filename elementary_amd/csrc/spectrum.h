// spectrum.h — the arithmetic of the spectrum analyser (spectrum.hip, elemhip_spectrum_set): an STFT of what the host-buffer render
// calls deliver, as power spectra or as band sums over them, with overlap carried across launch sets and calls.
//
// Per channel, frame j covers the delivered programme frames [j H - P, j H - P + S): S = 256 .. 4096 (ffr::size_ok), the hop H = 1 .. S,
// P = S / 2 when centred, else 0; samples outside the programme are zero. A sample (a float, widened) times its window entry is rounded
// ONCE, in double — not to float, as ffr::load_frame does for the `fft` node — then ffr::run_pass and the split step, all in double;
// the power re^2 + im^2 in double. Mode `power`: S / 2 + 1 columns per frame, each rounded to float once, at the store. Mode `bands`:
// B <= 512 rows of (first bin, count, count float weights); a column is the weighted sum of the row's bin powers, taken in double in
// ascending bin order by ONE lane, then rounded to float once: the bits do not depend on the launch. No logarithm here.
//
// A frame is emitted when its last sample has been delivered: after n frames frames_complete(n) are out. A flush pads with zeros up to
// frames_total(n). What is carried per channel is the last S - 1 delivered frames (`tail`; zero at a programme's start, which is also
// the padding in front of a centred programme) and a float64 running sum of every column over the floats just stored, in frame order.
//
// Written against plain pointers, as fft_frames.h is: the phases run on the device (buffers = LDS, one call per thread, __syncthreads
// between them) and on the host — tests/native/spectrum_host.cpp emulates the kThreads threads phase by phase, and analyse_host is the
// scalar twin the block-by-block host render (engine_host_blocks.cpp) runs on the same carried state.
#pragma once
#include <stdint.h>
#include <string.h>

#include "fft_frames.h"

namespace spectrum {

using ffr::c2;
using ffr::kThreads;
using ffr::pad;

constexpr uint32_t kMaxBands = 512;

// the tables of one analyser as a kernel (or the twin) reads them: device pointers in a launch, host pointers on the host
struct Plan {
    uint32_t size, hop, pad, cols, bands;     // pad = P; cols = bands, or size / 2 + 1 in power mode (bands = 0)
    const double* window;                     // [size]
    const double* twiddles;                   // exp(-2 pi i q / size), q < size, as (re, im) pairs (ffr::make_twiddles)
    const uint32_t* bandFirst;                // [bands]
    const uint32_t* bandCount;                // [bands]
    const uint32_t* bandOffset;               // [bands]: where the row's weights start in `weights`
    const float* weights;
};

// frames whose last sample lies among the first n delivered
LFFT_FD uint64_t frames_complete(uint64_t n, uint32_t S, uint32_t H, uint32_t P) { return n + P >= S ? (n + P - S) / H + 1u : 0u; }
// ... and the count a flush completes: centred, that of a centred STFT with constant padding; else the least that covers every sample
LFFT_FD uint64_t frames_total(uint64_t n, uint32_t S, uint32_t H, uint32_t P) {
    if (n == 0u) return 0u;
    return P ? n / H + 1u : (n > S ? (n - S + H - 1u) / H : 0u) + 1u;
}

// size, hop and the band rows of a spec (rows null: power mode)
inline bool spec_ok(uint32_t size, uint32_t hop, uint32_t bands, const uint32_t* first, const uint32_t* count) {
    if (!ffr::size_ok(size) || hop == 0u || hop > size || bands > kMaxBands) return false;
    if (bands && (!first || !count)) return false;
    for (uint32_t b = 0; b < bands; ++b)
        if (first[b] > size / 2u + 1u || count[b] > size / 2u + 1u - first[b]) return false;
    return true;
}

// ---- load: sample i of the frame is x(i) (a float); times the window in double, packed as z[n] = x[2n] + i x[2n + 1] ----
template <uint32_t M, class Fetch>
LFFT_FD void load_frame(Fetch x, const double* win, c2* a, uint32_t tid) {
    for (uint32_t n = tid; n < M; n += kThreads)
        a[pad(n)] = ffr::mk((double)x(2u * n) * win[2u * n], (double)x(2u * n + 1u) * win[2u * n + 1u]);
}

// ---- split + power: X[k] and its partner X[M - k] as ffr::store_bins forms them, |X|^2 in double into pw[0 .. M] ----
template <uint32_t M, class TP>
LFFT_FD void split_power(const c2* z, uint32_t tid, TP W, double* pw) {
    for (uint32_t k = tid; k <= M / 2u; k += kThreads) {
        const c2 A = z[pad(k)], B = z[pad((M - k) & (M - 1u))];
        const c2 s = A + ffr::cconj(B), it = ffr::mul_pi(ffr::cmul(W[k], A - ffr::cconj(B)));
        const c2 Xk = (s - it) * 0.5, Xmk = ffr::cconj(s + it) * 0.5;
        pw[k] = Xk.x * Xk.x + Xk.y * Xk.y;
        pw[M - k] = Xmk.x * Xmk.x + Xmk.y * Xmk.y;
    }
}
// where the powers go: the buffer the transform did not end in (M + 1 doubles of its 2 buf_stride)
template <uint32_t M> LFFT_FD double* power_buffer(c2* a, c2* b) { return reinterpret_cast<double*>((ffr::num_passes<M>() & 1u) ? a : b); }

// ---- store: one frame's columns, rounded to float once ----
LFFT_FD void store_columns(const Plan& p, const double* pw, uint32_t tid, float* out) {
    if (p.bands == 0u) {
        for (uint32_t k = tid; k < p.cols; k += kThreads) out[k] = (float)pw[k];
        return;
    }
    for (uint32_t b = tid; b < p.bands; b += kThreads) {
        const float* w = p.weights + p.bandOffset[b];
        const double* bin = pw + p.bandFirst[b];
        double acc = 0.0;
        for (uint32_t i = 0; i < p.bandCount[b]; ++i) acc += (double)w[i] * bin[i];
        out[b] = (float)acc;
    }
}

// ---- the carried frames: entry i of the tail behind a set of `valid` frames (x(q): the set's frame q) ----
template <class Src>
LFFT_FD float tail_next(const float* tailIn, uint32_t T, uint32_t valid, uint32_t i, Src x) {
    const int64_t q = (int64_t)i + (int64_t)valid - (int64_t)T;
    return q < 0 ? tailIn[i + valid] : x((uint32_t)q);
}

// ---- host side ----
// one frame through the kernel's phases, thread by thread
template <uint32_t M, class Fetch>
inline void frame_host(const Plan& p, Fetch x, c2* a, c2* b, float* out) {
    const c2* W = reinterpret_cast<const c2*>(p.twiddles);
    for (uint32_t tid = 0; tid < kThreads; ++tid) load_frame<M>(x, p.window, a, tid);
    for (uint32_t q = 0; q < ffr::num_passes<M>(); ++q)
        for (uint32_t tid = 0; tid < kThreads; ++tid) ffr::run_pass<M>(q, a, b, tid, W);
    double* pw = power_buffer<M>(a, b);
    for (uint32_t tid = 0; tid < kThreads; ++tid) split_power<M>(ffr::result<M>(a, b), tid, W, pw);
    for (uint32_t tid = 0; tid < kThreads; ++tid) store_columns(p, pw, tid, out);
}

// The scalar twin for one channel: `x` holds the nd frames delivered behind programme frame n0, `tail` (size - 1 floats, in-out) those
// in front of it. Frames [j0, j1) are transformed — the caller takes j0 = the frames emitted so far and j1 = frames_complete(n0 + nd),
// or frames_total(n0) with nd = 0 for a flush — into out[(j - j0) * cols ..], and `sums` (cols doubles, in-out) takes them in frame order.
inline void analyse_host(const Plan& p, float* tail, const float* x, size_t nd, uint64_t n0, uint64_t j0, uint64_t j1, float* out, double* sums) {
    const uint32_t T = p.size - 1u, stride = ffr::buf_stride(p.size);
    c2* a = new c2[2u * stride];
    c2* b = a + stride;
    for (uint64_t j = j0; j < j1; ++j) {
        const int64_t base = (int64_t)(j * p.hop) - (int64_t)p.pad - (int64_t)n0;
        auto fetch = [&](uint32_t i) -> float {
            const int64_t q = base + (int64_t)i;
            if (q < 0) { const int64_t t = q + (int64_t)T; return t >= 0 ? tail[t] : 0.0f; }
            return (uint64_t)q < nd ? x[q] : 0.0f;
        };
        float* o = out + (size_t)(j - j0) * p.cols;
        switch (p.size) {
            case 256u:  frame_host<128u>(p, fetch, a, b, o); break;
            case 512u:  frame_host<256u>(p, fetch, a, b, o); break;
            case 1024u: frame_host<512u>(p, fetch, a, b, o); break;
            case 2048u: frame_host<1024u>(p, fetch, a, b, o); break;
            default:    frame_host<2048u>(p, fetch, a, b, o); break;
        }
        for (uint32_t k = 0; k < p.cols; ++k) sums[k] += (double)o[k];
    }
    delete[] a;
    if (nd >= T) memcpy(tail, x + (nd - T), T * sizeof(float));
    else if (nd) { memmove(tail, tail + nd, (T - nd) * sizeof(float)); memcpy(tail + (T - nd), x, nd * sizeof(float)); }
}

} // namespace spectrum
