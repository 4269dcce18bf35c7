// flac_lpc.h — the LPC subframes of FLAC delivery (option "flac_lpc_order" = P, 1 .. 12; 0: none): which orders are priced, the window, the
// autocorrelation, the recursion, the quantisation and the residual, stated once for the encode kernel (flac_encode.hip) and its scalar
// twin (flac_encode.h, which includes this file and adds the pricing, the decision and the bits).
//
//   orders     P, and ceil(P / 2) where that differs: lpc_orders(). An order needs a residual: order < n. Nothing estimates an order's worth
//              from its prediction error; each priced order is counted to the bit like a FIXED order.
//   window     Welch, as a Q15 integer: w(i) = floor(32767 ((n + 1)^2 - (2i - n + 1)^2) / (n + 1)^2), the numerator being 4 (i + 1) (n - i).
//              The windowed sample is (s w) >> 15, an int32 (s has 25 bits at most).
//   lags       0 .. P of the windowed samples, int64 (2^48 x 4096 fits): integer sums, so lanes may add them in any order.
//   recursion  Levinson-Durbin in double on ONE lane (the twin executes the same statements): only + - x / in the order written, no
//              contraction (-ffp-contract=off, host and device), no library call but floor(). The lags enter as doubles, exactly:
//              where lag 0 (the largest) has more than 53 bits, all lags are shifted right (arithmetically) by its excess first.
//              No candidate where lag 0 is zero; an order at which the error is not a positive finite number is dropped with all above it.
//   quantise   precision q = lpc_precision(bits, n) <= 15; shift = q - 1 - e, cmax = m 2^e with m in [0.5, 1) the largest |coefficient|,
//              clamped to 15 from above, the order dropped where it is negative; rounding floor(x + 0.5) with the error fed forward
//              coefficient by coefficient, clamped to q bits two's complement.
//   residual   s[i] - ((sum of c[j] s[i - 1 - j]) >> shift), the sum in int64 as the decoder forms it (flac_decode.h, lpc_sample).
//              Outside (INT32_MIN, INT32_MAX] it is reported as INT32_MIN, whose zigzag 0xFFFFFFFF no admissible residual has: the
//              partition tree's maximum carries it to the root, and the decision drops the candidate.
#ifndef ELEMHIP_FLAC_LPC_H
#define ELEMHIP_FLAC_LPC_H
#include <stdint.h>

#include "pcm_pack.h"

namespace flac_encode {

constexpr uint32_t kLpcMaxOrder = 12;          // the RFC 9639 subset's limit up to 48 kHz, kept at every rate
constexpr uint32_t kLpcLags = kLpcMaxOrder + 1u;
constexpr uint32_t kLpcSlots = 2;              // priced LPC orders of a subframe, ascending
constexpr uint32_t kLpcOverflow = 0xFFFFFFFFu; // zigzag(INT32_MIN): a residual that no subframe may hold
constexpr uint32_t LPC_OK = 0, LPC_ZERO_LAG = 1, LPC_ERROR = 2, LPC_SHIFT = 3;      // why a priced order has no candidate

PCM_CX bool lpc_order_ok(uint32_t P) { return P <= kLpcMaxOrder; }
struct LpcOrders { uint32_t count, order[kLpcSlots]; };
PCM_CX LpcOrders lpc_orders(uint32_t P, uint32_t n) {
    const uint32_t h = (P + 1u) / 2u;
    const bool half = h != P && h >= 1u && h < n, full = P >= 1u && P < n;
    return LpcOrders{(half ? 1u : 0u) + (full ? 1u : 0u), {half ? h : full ? P : 0u, half && full ? P : 0u}};
}
// Coefficient bits: 12 at 16 bits and 14 at 24 for blocks above 2304 samples, one less per halving of the block down to 7 and 9 at 192
// and below — a short block cannot pay for precise coefficients (o q bits of every subframe).
PCM_CX uint32_t lpc_precision(uint32_t bits, uint32_t n) {
    return (bits == 16u ? 7u : 9u) + (n > 192u ? 1u : 0u) + (n > 384u ? 1u : 0u) + (n > 576u ? 1u : 0u) + (n > 1152u ? 1u : 0u) + (n > 2304u ? 1u : 0u);
}

PCM_FD int32_t lpc_window(uint32_t i, uint32_t n) {
    const uint64_t d = (uint64_t)(n + 1u) * (n + 1u);
    return (int32_t)((32767ull * 4ull * (uint64_t)(i + 1u) * (uint64_t)(n - i)) / d);
}
PCM_FD int32_t lpc_windowed(int32_t s, uint32_t i, uint32_t n) { return (int32_t)(((int64_t)s * lpc_window(i, n)) >> 15); }

// acc[lag] += the products x[i] x[i - lag] of the samples i = begin, begin + stride, ... (x: the windowed samples as stored words)
PCM_FD void lpc_lags(const uint32_t* x, uint32_t n, uint32_t maxLag, uint32_t begin, uint32_t stride, int64_t (&acc)[kLpcLags]) {
    for (uint32_t i = begin; i < n; i += stride) {
        const int64_t xi = (int32_t)x[i];
#pragma unroll
        for (uint32_t lag = 0; lag < kLpcLags; ++lag)
            if (lag <= maxLag && lag <= i) acc[lag] += xi * (int64_t)(int32_t)x[i - lag];
    }
}

// what one lane works in (the kernel: shared memory) and what it publishes
struct LpcScratch { int64_t lag[kLpcLags]; double r[kLpcLags], a[kLpcMaxOrder], t[kLpcMaxOrder]; };
struct LpcPlan {
    uint32_t count, precision, order[kLpcSlots], shift[kLpcSlots], drop[kLpcSlots];
    int16_t coef[kLpcSlots][kLpcMaxOrder];
};

PCM_FD bool lpc_finite(double x) { return x - x == 0.0; }

// coefficients a[0 .. o) -> q-bit integers and their shift; returns LPC_OK or LPC_SHIFT
PCM_FD uint32_t lpc_quantise(const double* a, uint32_t o, uint32_t q, int16_t* out, uint32_t* shiftOut) {
    double cmax = 0.0;
    for (uint32_t j = 0; j < o; ++j) { const double m = a[j] < 0.0 ? 0.0 - a[j] : a[j]; cmax = m > cmax ? m : cmax; }
    int32_t e = 0;
    if (cmax == 0.0) e = -16;
    while (cmax >= 1.0) { cmax = cmax * 0.5; ++e; }
    while (cmax < 0.5 && e > -16) { cmax = cmax * 2.0; --e; }      // (from -16 down the shift is 15 whatever e is)
    int32_t shift = (int32_t)q - 1 - e;
    if (shift > 15) shift = 15;
    if (shift < 0) return LPC_SHIFT;
    const double scale = (double)(1u << shift), hi = (double)((1 << (q - 1u)) - 1), lo = 0.0 - (double)(1 << (q - 1u));
    double err = 0.0;
    for (uint32_t j = 0; j < o; ++j) {
        err = err + a[j] * scale;
        double v = __builtin_floor(err + 0.5);
        v = v > hi ? hi : v; v = v < lo ? lo : v;
        out[j] = (int16_t)(int32_t)v;
        err = err - v;
    }
    *shiftOut = (uint32_t)shift;
    return LPC_OK;
}

// ws.lag[0 .. P] -> the plan of a subframe of n samples: one recursion, both priced orders
PCM_FD void lpc_design(LpcScratch& ws, uint32_t P, uint32_t n, uint32_t bits, LpcPlan& plan) {
    const LpcOrders po = lpc_orders(P, n);
    plan.count = po.count; plan.precision = lpc_precision(bits, n);
    plan.order[0] = po.order[0]; plan.order[1] = po.order[1];
    for (uint32_t i = 0; i < kLpcSlots; ++i) { plan.shift[i] = 0u; plan.drop[i] = LPC_OK; }
    if (po.count == 0u) return;
    if (ws.lag[0] == 0) { for (uint32_t i = 0; i < po.count; ++i) plan.drop[i] = LPC_ZERO_LAG; return; }
    const uint32_t top = po.count == 2u ? po.order[1] : po.order[0];
    uint32_t down = 0;
    while (((uint64_t)ws.lag[0] >> down) >> 53) ++down;
    for (uint32_t k = 0; k <= top; ++k) ws.r[k] = (double)(ws.lag[k] >> down);
    double err = ws.r[0];
    uint32_t slot = 0;
    for (uint32_t k = 0; k < top; ++k) {            // order k + 1 from order k
        double acc = ws.r[k + 1u];
        for (uint32_t j = 0; j < k; ++j) acc = acc - ws.a[j] * ws.r[k - j];
        const double refl = acc / err;
        for (uint32_t j = 0; j < k; ++j) ws.t[j] = ws.a[j] - refl * ws.a[k - 1u - j];
        for (uint32_t j = 0; j < k; ++j) ws.a[j] = ws.t[j];
        ws.a[k] = refl;
        err = err * (1.0 - refl * refl);
        if (!(err > 0.0) || !lpc_finite(err)) { for (uint32_t i = slot; i < po.count; ++i) plan.drop[i] = LPC_ERROR; return; }
        if (k + 1u == plan.order[slot]) {
            plan.drop[slot] = lpc_quantise(ws.a, k + 1u, plan.precision, plan.coef[slot], &plan.shift[slot]);
            ++slot;
        }
    }
}

struct LpcResidual {
    const int32_t* s; const int16_t* c; uint32_t order, shift;
    PCM_FD int32_t operator()(uint32_t i) const {
        int64_t sum = 0;
        for (uint32_t j = 0; j < order; ++j) sum += (int64_t)c[j] * (int64_t)s[i - 1u - j];
        const int64_t r = (int64_t)s[i] - (sum >> shift);
        return r <= (int64_t)INT32_MIN || r > (int64_t)INT32_MAX ? INT32_MIN : (int32_t)r;
    }
};
// bits in front of an LPC residual's partitions: header byte, warm-up, precision, shift, coefficients, coding method and partition order
PCM_CX uint32_t lpc_base(uint32_t bps, uint32_t order, uint32_t q) { return 8u + bps * order + 4u + 5u + q * order + 6u; }

} // namespace flac_encode

#endif // ELEMHIP_FLAC_LPC_H
