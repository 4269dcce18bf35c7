// resample.h — the arithmetic and the lane schedule of the delivery-rate converter (resample.hip, Engine option "resample_rate"): a
// polyphase Kaiser-windowed sinc that turns the frames a launch set rendered at the engine's rate `fin` into frames at the delivery
// rate `fout`, where the set's output lies in HBM. Nothing here knows which side is the engine's: a plan is made from two integral
// rates, and the input-rate converter (resample_in.hip, option "input_rate") takes the same plan, tables and tap sum with fin = the
// input's rate; what that side adds — the pull schedule, its scalar loop — is the last section below.
//
// The plan.  g = gcd(fin, fout), L = fout / g, M = fin / g, s = min(1, L / M), half width W = Z / s input frames (Z = 32), Wc = ceil(W),
// T = 2 Wc taps per phase, latency Do = ceil(Wc L / M) OUTPUT frames. Prototype g(t) = s sinc(s t) I0(beta sqrt(1 - (t / W)^2)) / I0(beta)
// for |t| < W, else 0, beta = 0.1102 (100 - 8.7); h[p][k] = float32(g(p / L + Wc - 1 - k)), computed in double, I0 by its power series
// to convergence, no per-phase renormalisation.
//
// Output n of the programme (n >= 0): a = (n - Do) M, i0 = floor(a / L), p = a - i0 L, y[n] = sum_k h[p][k] x[i0 - Wc + 1 + k], x[j] = 0
// for j < 0. The largest input index used is <= floor(n M / L): after t input frames exactly ceil(t L / M) outputs exist, and a call
// that consumes inputs [t0, t1) delivers outputs [ceil(t0 L / M), ceil(t1 L / M)) — however the programme is cut, the same bits.
// The smallest index used by an output of that stretch is >= t0 - H with H = T + ceil(M / L) + 1: the frames carried per channel.
//
// Limits: L <= 1024 and T <= 1024 (the table, and a tile's stretch in LDS), and L <= 8 M: a launch set holds up to 2^29 frames
// and the kernels count a set's frames in 32 bits, so a set may grow eightfold at most on its way out. A rate that is not integral
// has no plan either.
//
// Tables, in OUTPUT order: n = q L + r gives p = ((r - Do) M) mod L and i0 = q M + rowBase[r], rowBase[r] = floor((r - Do) M / L) — no
// division inside the tap loop — and the coefficients lie [k][r], so consecutive lanes (consecutive n) read consecutive floats.
//
// The tap sum is tap_sum() below and nothing else: k ascending, float32, acc = fmaf(h, x, acc) — one rounding per tap, on the device one
// v_fma_f32. The kernel and resample_host() both call it, so device and host leave the same bits. Non-finite inputs propagate.
//
// Plain C++ for host and device alike: tests/native/resample_host.cpp runs the kernel's schedule with these functions lane by lane
// against resample_host(), the scalar loop's production twin, which the engine uses where a render's floats are already on the host.
#ifndef ELEMHIP_RESAMPLE_H
#define ELEMHIP_RESAMPLE_H
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RS_FD __host__ __device__ __forceinline__
#else
#define RS_FD inline
#endif

namespace resample {

constexpr uint32_t kZ = 32;               // zero crossings of the prototype on either side, at the lower of the two rates
constexpr uint32_t kMaxL = 1024, kMaxT = 1024, kMaxGrowth = 8;
constexpr uint32_t kTile = 256;           // output frames per workgroup: one lane each
constexpr uint32_t kGroup = 4;            // channels a lane sums side by side: one coefficient load serves them all

struct Plan { uint32_t L, M, Wc, T, Do, H; };

RS_FD uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1u) / b; }
RS_FD int64_t floor_div(int64_t a, int64_t b) { const int64_t q = a / b; return (a % b != 0 && (a < 0) != (b < 0)) ? q - 1 : q; }
// outputs that exist after `t` input frames of the programme
RS_FD uint64_t outputs_before(const Plan& p, uint64_t t) { return ceil_div(t * p.L, p.M); }

// ---- the plan and the tables (host) -------------------------------------------------------------------------------------------------
inline bool make_plan(double fin, double fout, Plan& p) {
    if (!(fin >= 1.0 && fout >= 1.0 && fin <= 2147483647.0 && fout <= 2147483647.0) || fin != floor(fin) || fout != floor(fout)) return false;
    uint64_t a = (uint64_t)fin, b = (uint64_t)fout;
    while (b) { const uint64_t r = a % b; a = b; b = r; }
    const uint64_t L = (uint64_t)fout / a, M = (uint64_t)fin / a;
    if (L > kMaxL || L > (uint64_t)kMaxGrowth * M) return false;
    const uint64_t Wc = L >= M ? kZ : ceil_div((uint64_t)kZ * M, L);
    if (2u * Wc > kMaxT) return false;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.Wc = (uint32_t)Wc; p.T = (uint32_t)(2u * Wc);
    p.Do = (uint32_t)ceil_div(Wc * L, M);
    p.H = p.T + (uint32_t)ceil_div(M, L) + 1u;
    return true;
}
inline double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 1000; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term <= 1e-18 * sum) break;
    }
    return sum;
}
inline double prototype(const Plan& p, double t) {
    const double pi = 3.14159265358979323846, beta = 0.1102 * (100.0 - 8.7);
    const double s = p.L >= p.M ? 1.0 : (double)p.L / (double)p.M, W = (double)kZ / s;
    if (!(fabs(t) < W)) return 0.0;
    const double u = t / W, x = s * t;
    return s * (x == 0.0 ? 1.0 : sin(pi * x) / (pi * x)) * bessel_i0(beta * sqrt(1.0 - u * u)) / bessel_i0(beta);
}
RS_FD int32_t row_base(const Plan& p, uint32_t r) { return (int32_t)floor_div(((int64_t)r - (int64_t)p.Do) * (int64_t)p.M, (int64_t)p.L); }
RS_FD uint32_t row_phase(const Plan& p, uint32_t r) { return (uint32_t)(((int64_t)r - (int64_t)p.Do) * (int64_t)p.M - (int64_t)row_base(p, r) * (int64_t)p.L); }
// table[T * L] as [k][r], rowBase[L]
inline void make_tables(const Plan& p, float* table, int32_t* rowBase) {
    for (uint32_t r = 0; r < p.L; ++r) {
        rowBase[r] = row_base(p, r);
        const double frac = (double)row_phase(p, r) / (double)p.L;
        for (uint32_t k = 0; k < p.T; ++k) table[(size_t)k * p.L + r] = (float)prototype(p, frac + (double)p.Wc - 1.0 - (double)k);
    }
}

// ---- the tap sum --------------------------------------------------------------------------------------------------------------------
// acc[c] = sum over k ascending of coef[k * stride] * x(c, k), C channels side by side on one coefficient
template <int C, class Fetch>
RS_FD void tap_sum(const float* coef, uint32_t stride, uint32_t T, Fetch x, float* acc) {
    for (int c = 0; c < C; ++c) acc[c] = 0.0f;
    for (uint32_t k = 0; k < T; ++k) {
        const float h = coef[(size_t)k * stride];
        for (int c = 0; c < C; ++c) acc[c] = fmaf(h, x(c, k), acc[c]);
    }
}

// ---- where an output finds its inputs -----------------------------------------------------------------------------------------------
// i0 of output n: its taps read the programme's frames i0 - Wc + 1 .. i0 + Wc
RS_FD int64_t centre(const Plan& p, const int32_t* rowBase, uint64_t n) { return (int64_t)(n / p.L) * (int64_t)p.M + (int64_t)rowBase[n % p.L]; }

// ---- a launch set: [block][channel][blockSize] in, the same layout out ---------------------------------------------------------------
// the programme's frame t0 + rel, for a set that starts at t0 and holds validIn frames: from the set, or from the H carried frames
// in front of it (oldest first); beyond either — which no output of the set reaches — silence
RS_FD float input_at(const float* src, uint32_t bs, uint32_t nCh, uint32_t c, uint32_t validIn, const float* hist, uint32_t H, int64_t rel) {
    if (rel >= 0) {
        const uint32_t f = (uint32_t)rel;
        return rel < (int64_t)validIn ? src[((size_t)(f / bs) * nCh + c) * bs + f % bs] : 0.0f;
    }
    return rel + (int64_t)H >= 0 ? hist[(int64_t)H + rel] : 0.0f;
}
// the carried frames behind a set of validIn frames: slot j (oldest first)
RS_FD float history_next(const float* src, uint32_t bs, uint32_t nCh, uint32_t c, const float* old, uint32_t validIn, uint32_t H, uint32_t j) {
    const uint64_t at = (uint64_t)validIn + j;
    if (at >= H) { const uint32_t f = (uint32_t)(at - H); return src[((size_t)(f / bs) * nCh + c) * bs + f % bs]; }
    return old[at];
}
// A tile = kTile consecutive outputs of the set, lane <-> output, kGroup channels. Its input stretch — from the first tap of its first
// output to the last tap of its last — is staged once per channel in an LDS row; lane and tap then read row[skew(base + k)].
// skew(i) = i + i / 32 pads one dword per 32: ds_read_b32 banks are (address / 4) mod 32 per 32-lane half, and at M / L = 4
// neighbouring lanes read 4 dwords apart — unpadded, 8 banks for 32 lanes (4-way); padded, lane l's address is 4 l + l / 8 + const, 32
// distinct banks. What remains: at ratios under 2 the lanes' distances alternate (1 and 2 at 3:2; mostly 1 at 160:147), 32 lanes cover
// 35 to 48 dwords plus a pad or two, so up to half the banks serve two lanes (2-way for that half-wave's read); when upsampling
// neighbours share an address, which broadcasts. The staging writes are consecutive: one 2-way clash per pad crossed.
RS_FD uint32_t skew(uint32_t i) { return i + (i >> 5); }
RS_FD uint32_t span_max(const Plan& p) { return (uint32_t)ceil_div((uint64_t)(kTile - 1u) * p.M, p.L) + 1u + p.T; }
RS_FD uint32_t row_floats(const Plan& p) { return skew(span_max(p)) + 1u; }
struct Tile { int64_t jlo; uint32_t span; };      // the programme's frame in row slot 0; slots in use
// fFirst: the tile's first output, counted from the set's first (n0); validOut: outputs of the set; fFirst < validOut
RS_FD Tile tile_of(const Plan& p, const int32_t* rowBase, uint64_t n0, uint32_t fFirst, uint32_t validOut) {
    const uint32_t last = (validOut - fFirst < kTile ? validOut : fFirst + kTile) - 1u;
    Tile t;
    t.jlo = centre(p, rowBase, n0 + fFirst) - (int64_t)p.Wc + 1;
    t.span = (uint32_t)(centre(p, rowBase, n0 + last) + (int64_t)p.Wc - t.jlo + 1);
    return t;
}
// row slot of tap 0 of output n of that tile
RS_FD uint32_t lane_base(const Plan& p, const int32_t* rowBase, const Tile& t, uint64_t n) {
    return (uint32_t)(centre(p, rowBase, n) - (int64_t)p.Wc + 1 - t.jlo);
}

// ---- the scalar loop ----------------------------------------------------------------------------------------------------------------
// One channel: x holds the programme's frames [t0, t0 + n), hist the H frames in front of t0 (zeros at a reset) and, on return, the H
// frames in front of t0 + n. y receives outputs [outputs_before(t0), outputs_before(t0 + n)); returns how many.
inline size_t resample_host(const Plan& p, const float* table, const int32_t* rowBase, float* hist, const float* x, size_t n, uint64_t t0, float* y) {
    const uint64_t n0 = outputs_before(p, t0), n1 = outputs_before(p, t0 + n);
    for (uint64_t m = n0; m < n1; ++m) {
        const int64_t rel0 = centre(p, rowBase, m) - (int64_t)p.Wc + 1 - (int64_t)t0;
        tap_sum<1>(table + m % p.L, p.L, p.T, [&](int, uint32_t k) {
            const int64_t j = rel0 + (int64_t)k;
            return j >= 0 ? x[j] : (j + (int64_t)p.H >= 0 ? hist[(int64_t)p.H + j] : 0.0f);
        }, y + (m - n0));
    }
    if (n >= p.H) memcpy(hist, x + (n - p.H), p.H * sizeof(float));
    else if (n) { memmove(hist, hist + n, (p.H - n) * sizeof(float)); memcpy(hist + (p.H - n), x, n * sizeof(float)); }
    return (size_t)(n1 - n0);
}

// ---- the input side: the engine pulls (resample_in.hip, Engine option "input_rate") -------------------------------------------------
// The plan is made with fin = the input's rate and fout = the engine's. The engine renders whole calls of engine frames, so a call of
// `numFrames` outputs that starts at the programme's output n0 consumes the inputs [inputs_before(n0), inputs_before(n0 + numFrames)):
// inputs_before(n) is the smallest t for which output n - 1 exists, the smallest t with outputs_before(t) >= n. Output n - 1 reads no
// index above floor((n - 1) M / L) = inputs_before(n) - 1 (see above), so nothing reads past what the call was given.
// The smallest index an output of that call reads is centre(n0) - Wc + 1 = floor((n0 - Do) M / L) - Wc + 1, and inputs_before(n0) minus
// that is floor((n0 - 1) M / L) - floor((n0 - Do) M / L) + Wc <= ceil((Do - 1) M / L) + Wc <= 2 Wc = T, because (Do - 1) M / L < Wc by
// Do = ceil(Wc L / M). T <= H: the plan's H carried frames more than suffice on this side too.
// 32-bit counts: a set's input stretch is about M / L times its engine frames, so a plan with M > kMaxGrowth L is refused here.
RS_FD uint64_t inputs_before(const Plan& p, uint64_t n) { return n == 0u ? 0u : (n - 1u) * p.M / p.L + 1u; }
inline bool make_plan_in(double fin, double fout, Plan& p) {
    Plan q;
    if (!make_plan(fin, fout, q) || q.M > (uint64_t)kMaxGrowth * q.L) return false;
    p = q;
    return true;
}
// the carried frames behind a stretch of validIn frames, slot j (oldest first); at(f) is the stretch's frame f
template <class At>
RS_FD float history_pull(At at, const float* old, uint32_t validIn, uint32_t H, uint32_t j) {
    const uint64_t i = (uint64_t)validIn + j;
    return i >= H ? at((uint32_t)(i - H)) : old[i];
}
// A tile of the input-side kernel = kTile consecutive engine frames of the set, one stream, C channels of it; tile_of, lane_base, skew and
// row_floats are the ones above with n0 = the set's first engine frame. Of the row slots [0, span) the slots [lo, hi) come from the
// set's stretch of the stream (slot i <-> frame rel0 + i of the stretch, rel0 = jlo - t0), the slots below lo from the carried frames;
// slots from hi on lie behind the stretch, where no output of the set reaches: silence.
struct StreamPart { uint32_t lo, hi; };
RS_FD StreamPart stream_part(int64_t rel0, uint32_t span, uint32_t validIn) {
    StreamPart s;
    s.lo = rel0 >= 0 ? 0u : (-rel0 < (int64_t)span ? (uint32_t)(-rel0) : span);
    const int64_t end = (int64_t)validIn - rel0;
    s.hi = end <= (int64_t)s.lo ? s.lo : (end < (int64_t)span ? (uint32_t)end : span);
    return s;
}
// a carried frame: the programme's frame t0 + rel, rel < 0
RS_FD float carried_at(const float* hist, uint32_t H, int64_t rel) { return rel + (int64_t)H >= 0 ? hist[(int64_t)H + rel] : 0.0f; }
// LDS of the input-side kernel: C padded rows, then (16-byte aligned) the image of a narrow stream's stretch — G <= C channels of up to
// 4 bytes, so it is sized by C and never by the stream's width; a wider stream is read sample by sample and has no image
RS_FD uint32_t in_image_offset(const Plan& p, uint32_t C) { return (C * row_floats(p) * 4u + 15u) & ~15u; }
RS_FD uint32_t in_lds_bytes(const Plan& p, uint32_t C) { return in_image_offset(p, C) + span_max(p) * C * 4u + 32u; }

// The scalar pull loop, one channel: y receives the outputs [n0, n0 + numFrames); x holds the programme's frames from
// inputs_before(n0) on, hist the H frames in front of them (zeros at a reset) and, on return, the H frames in front of what the
// next call takes. Returns the frames consumed.
inline size_t resample_in_host(const Plan& p, const float* table, const int32_t* rowBase, float* hist, const float* x, uint64_t n0, size_t numFrames, float* y) {
    const uint64_t t0 = inputs_before(p, n0);
    const size_t n = (size_t)(inputs_before(p, n0 + numFrames) - t0);
    for (uint64_t m = n0; m < n0 + numFrames; ++m) {
        const int64_t rel0 = centre(p, rowBase, m) - (int64_t)p.Wc + 1 - (int64_t)t0;
        tap_sum<1>(table + m % p.L, p.L, p.T, [&](int, uint32_t k) {
            const int64_t j = rel0 + (int64_t)k;
            return j >= 0 ? x[j] : (j + (int64_t)p.H >= 0 ? hist[(int64_t)p.H + j] : 0.0f);
        }, y + (m - n0));
    }
    if (n >= p.H) memcpy(hist, x + (n - p.H), p.H * sizeof(float));
    else if (n) { memmove(hist, hist + n, (p.H - n) * sizeof(float)); memcpy(hist + (p.H - n), x, n * sizeof(float)); }
    return n;
}

} // namespace resample

#endif // ELEMHIP_RESAMPLE_H
