// fft_frames.h — the transform core of the `fft` analyzer node's relay (fft_frames.hip): the real FFT of one windowed frame of
// S = 256 .. 4096 samples as a packed complex FFT of M = S / 2 points (Stockham, radix-16 passes and one closing pass of radix
// 2, 4 or 8 where M is no power of 16, ping-pong between two padded LDS buffers) followed by the split step.
//
// The arithmetic is DOUBLE, the result rounded to float once, at the store. The reference's transform (audiofft, Ooura backend)
// works in double and rounds to float as well: its recorded spectra sit within half a float ulp of the exact DFT, and the event
// tolerance is twice that. The first build of this core ran fft4096.h's float butterflies and missed it by 3.5x (size 256:
// 8.2e-7 against a float64 DFT where the reference has 2.4e-7). The MI355X's fp64 vector rate is half its fp32 rate: the cost is
// LDS (16 bytes per point), not time — and a launch asks for the LDS of its LARGEST frame only (fft_frames.hip).
//
// Written against plain pointers, as fft4096.h is, so that the same code runs on the device (buffers = LDS, one call per thread,
// __syncthreads between the phases) and on the host (tests/native/fft_frames_host.cpp emulates the kThreads threads phase by
// phase and prints the spectra of given frames): the arithmetic the event tolerance rests on is testable without a GPU.
//
// Conventions. W[q] = exp(-2 pi i q / S), q < S (made in double on the host: every twiddle of every pass and of the split is ONE
// table entry). Output X[k] = sum_n x[n] exp(-2 pi i n k / S), k = 0 .. S / 2, unnormalised.
#pragma once
#include <math.h>

#include "fft4096.h"     // LFFT_FD, pad()

namespace ffr {

using lfft::pad;

typedef double c2 __attribute__((ext_vector_type(2)));   // x = re, y = im

LFFT_FD c2 mk(double re, double im) { c2 v; v.x = re; v.y = im; return v; }
LFFT_FD c2 cmul(c2 a, c2 b) { return mk(__builtin_fma(a.x, b.x, -(a.y * b.y)), __builtin_fma(a.x, b.y, a.y * b.x)); }
LFFT_FD c2 cconj(c2 a) { return mk(a.x, -a.y); }
LFFT_FD c2 mul_mi(c2 a) { return mk(a.y, -a.x); }      // a * -i
LFFT_FD c2 mul_pi(c2 a) { return mk(-a.y, a.x); }      // a * +i
// radix-4 butterfly, forward sign (lfft::bfly4 in double)
LFFT_FD void bfly4(c2& x0, c2& x1, c2& x2, c2& x3) {
    const c2 a0 = x0 + x2, a1 = x0 - x2, a2 = x1 + x3, a3 = mul_mi(x1 - x3);
    x0 = a0 + a2; x1 = a1 + a3; x2 = a0 - a2; x3 = a1 - a3;
}
// 16-point DFT in registers, natural order in and out (lfft::dft16 in double): n = n1 + 4 n2, m = 4 m1 + m2
LFFT_FD void dft16(c2 (&v)[16]) {
    const double c1 = 0.92387953251128673848, s1 = 0.38268343236508978178, r2 = 0.70710678118654752440;
    const c2 w1 = mk(c1, -s1), w2 = mk(r2, -r2), w3 = mk(s1, -c1), w6 = mk(-r2, -r2), w9 = mk(-c1, s1);
#pragma unroll
    for (int n1 = 0; n1 < 4; ++n1) bfly4(v[n1], v[n1 + 4], v[n1 + 8], v[n1 + 12]);
    v[1 + 4] = cmul(v[1 + 4], w1); v[1 + 8] = cmul(v[1 + 8], w2); v[1 + 12] = cmul(v[1 + 12], w3);
    v[2 + 4] = cmul(v[2 + 4], w2); v[2 + 8] = mul_mi(v[2 + 8]);   v[2 + 12] = cmul(v[2 + 12], w6);
    v[3 + 4] = cmul(v[3 + 4], w3); v[3 + 8] = cmul(v[3 + 8], w6); v[3 + 12] = cmul(v[3 + 12], w9);
    c2 o[16];
#pragma unroll
    for (int m2 = 0; m2 < 4; ++m2) {
        c2 y0 = v[4 * m2], y1 = v[4 * m2 + 1], y2 = v[4 * m2 + 2], y3 = v[4 * m2 + 3];
        bfly4(y0, y1, y2, y3);
        o[m2] = y0; o[4 + m2] = y1; o[8 + m2] = y2; o[12 + m2] = y3;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = o[i];
}

constexpr uint32_t kThreads = 128;                // M / 16 butterflies of the largest transform
constexpr uint32_t kMaxM = 2048;
constexpr uint32_t kBuf = kMaxM + kMaxM / 16;     // one padded buffer (c2 elements of 16 bytes); the transform uses two: 68 KB of LDS
LFFT_FD constexpr uint32_t buf_stride(uint32_t size) { return size / 2u + size / 32u; }   // ... of a size-`size` frame: pad(M - 1) < M + M / 16
constexpr uint32_t kRing = 8192;                  // frames of the reference's ring (MultiChannelRingBuffer.h:17), the default capacity

LFFT_FD bool size_ok(uint32_t size) { return size == 256u || size == 512u || size == 1024u || size == 2048u || size == 4096u; }

// R-point DFT in registers, natural order in and out, forward sign
template <uint32_t R> LFFT_FD void dft(c2 (&v)[R]);
template <> LFFT_FD void dft<2>(c2 (&v)[2]) { const c2 a = v[0] + v[1], b = v[0] - v[1]; v[0] = a; v[1] = b; }
template <> LFFT_FD void dft<4>(c2 (&v)[4]) { bfly4(v[0], v[1], v[2], v[3]); }
template <> LFFT_FD void dft<8>(c2 (&v)[8]) {
    const double r2 = 0.70710678118654752440;
    bfly4(v[0], v[2], v[4], v[6]);                                       // even samples -> E[m] in v[0], v[2], v[4], v[6]
    bfly4(v[1], v[3], v[5], v[7]);                                       // odd samples  -> O[m] in v[1], v[3], v[5], v[7]
    const c2 o0 = v[1], o1 = cmul(v[3], mk(r2, -r2)), o2 = mul_mi(v[5]), o3 = cmul(v[7], mk(-r2, -r2));   // O[m] W8^m
    const c2 e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6];
    v[0] = e0 + o0; v[1] = e1 + o1; v[2] = e2 + o2; v[3] = e3 + o3;
    v[4] = e0 - o0; v[5] = e1 - o1; v[6] = e2 - o2; v[7] = e3 - o3;
}
template <> LFFT_FD void dft<16>(c2 (&v)[16]) { dft16(v); }

// ---- load: frame samples [read, read + 2 M) of the ring (wrapped at `mask` + 1 frames: 8192, or the longer history ring of a node
// made under "event_history_blocks"), times the window in double, rounded to FLOAT as the reference hands them to its transform
// (FFT.h:114-120 with FloatType = double), packed as z[n] = x[2n] + i x[2n + 1] ----
template <uint32_t M>
LFFT_FD void load_frame(const float* ring, uint32_t read, const double* win, c2* a, uint32_t tid, uint32_t mask = kRing - 1u) {
    for (uint32_t n = tid; n < M; n += kThreads) {
        const float x0 = ring[(read + 2u * n) & mask], x1 = ring[(read + 2u * n + 1u) & mask];
        a[pad(n)] = mk((double)(float)((double)x0 * win[2u * n]), (double)(float)((double)x1 * win[2u * n + 1u]));
    }
}

// ---- one Stockham pass of radix R behind passes of total radix Ns: butterfly j of M / R reads in[j + r M / R], multiplies by
// exp(-2 pi i r k / (Ns R)), k = j mod Ns, and writes the R-point DFT to out[(j - k) R + k + r Ns] ----
template <uint32_t M, uint32_t R, uint32_t Ns, class TP>
LFFT_FD void pass(const c2* in, c2* out, uint32_t tid, TP W) {
    constexpr uint32_t T = M / R, step = 2u * M / (Ns * R);              // the twiddle as an index into W: r k step < 2 M
    for (uint32_t j = tid; j < T; j += kThreads) {
        c2 v[R];
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) v[r] = in[pad(j + r * T)];
        const uint32_t k = j & (Ns - 1u);
        if (Ns > 1u) {
#pragma unroll
            for (uint32_t r = 1; r < R; ++r) v[r] = cmul(v[r], W[r * k * step]);
        }
        dft<R>(v);
        const uint32_t base = (j - k) * R + k;
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) out[pad(base + r * Ns)] = v[r];
    }
}

template <uint32_t M> constexpr uint32_t num_passes() { return M <= 256u ? 2u : 3u; }
// pass p of the M-point transform: even passes read `a` and write `b`, odd ones the other way; a barrier belongs between two passes
template <uint32_t M, class TP>
LFFT_FD void run_pass(uint32_t p, c2* a, c2* b, uint32_t tid, TP W) {
    static_assert(M == 128u || M == 256u || M == 512u || M == 1024u || M == 2048u, "complex lengths of the real sizes 256 .. 4096");
    if (p == 0u) pass<M, 16u, 1u>(a, b, tid, W);
    else if (p == 1u) { if constexpr (M == 128u) pass<M, 8u, 16u>(b, a, tid, W); else pass<M, 16u, 16u>(b, a, tid, W); }
    else if constexpr (M > 256u) pass<M, M / 256u, 256u>(a, b, tid, W);
}
// where the transform ends up
template <uint32_t M> LFFT_FD c2* result(c2* a, c2* b) { return (num_passes<M>() & 1u) ? b : a; }

// ---- split + store: X[k] = ((Z[k] + conj Z[M-k]) - i w^k (Z[k] - conj Z[M-k])) / 2 and its partner X[M-k] from the same product
// (fft4096.h split_forward), rounded to float; re / im receive bins 0 .. M ----
template <uint32_t M, class TP>
LFFT_FD void store_bins(const c2* z, uint32_t tid, TP W, float* re, float* im) {
    for (uint32_t k = tid; k <= M / 2u; k += kThreads) {
        const c2 A = z[pad(k)], B = z[pad((M - k) & (M - 1u))];
        const c2 s = A + cconj(B), it = mul_pi(cmul(W[k], A - cconj(B)));
        const c2 Xk = (s - it) * 0.5, Xmk = cconj(s + it) * 0.5;
        re[k] = (float)Xk.x; im[k] = (float)Xk.y;
        re[M - k] = (float)Xmk.x; im[M - k] = (float)Xmk.y;
    }
}

// ---- host side: the two tables of one size, made in double ----
// Blackman-Harris, the argument i / (size - 1) (FFT.h:51-65 as Runtime<double> evaluates it)
inline void make_window(uint32_t size, double* win) {
    const double a0 = 0.35875, a1 = 0.48829, a2 = 0.14128, a3 = 0.01168, pi = 3.1415926535897932385;
    for (uint32_t i = 0; i < size; ++i) {
        const double t = (double)i / (double)(size - 1u);
        win[i] = a0 - a1 * cos(2.0 * pi * t) + a2 * cos(4.0 * pi * t) - a3 * cos(6.0 * pi * t);
    }
}
inline void make_twiddles(uint32_t size, c2* W) {
    const double pi = 3.1415926535897932385;
    for (uint32_t q = 0; q < size; ++q) { const double a = -2.0 * pi * (double)q / (double)size; W[q] = mk(cos(a), sin(a)); }
}

} // namespace ffr
