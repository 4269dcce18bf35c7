// tests/native/spectrum_host.cpp — the spectrum analyser's frame kernel (elementary_amd/csrc/spectrum.h, spectrum.hip) run on the HOST:
// the 128 threads of a workgroup are emulated phase by phase (every phase between two barriers is a loop over tid), with a loop of
// its own — not spectrum::analyse_host, whose bits it must print.
//   spectrum_host <size> <hop> <center 0|1> <programme.f32> <window.f64> <power.f32> <bins.f64>
// programme.f32: one channel's delivered frames; every analyser frame of the flushed programme is gathered by index with zero fill,
// windowed and transformed as the kernel does it. power.f32 receives size/2+1 float columns per frame (power mode); bins.f64 the
// split step's X[k] as (re, im) doubles, size/2+1 pairs per frame — what the tolerance constant of tests/spectrum_reference.py is
// measured on.
//   clang++ -std=c++17 -O2 -ffp-contract=off -I elementary_amd/csrc tests/native/spectrum_host.cpp -o spectrum_host
// The same file builds with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "spectrum.h"

using namespace ffr;

static std::vector<char> slurp(const char* path) {
    std::vector<char> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); std::exit(2); }
    char tmp[65536];
    for (size_t got; (got = std::fread(tmp, 1, sizeof tmp, f)) > 0;) v.insert(v.end(), tmp, tmp + got);
    std::fclose(f);
    return v;
}

// the split step once more, keeping X instead of |X|^2: the same expressions as spectrum::split_power
template <uint32_t M>
static void split_bins(const c2* z, uint32_t tid, const c2* W, double* bins) {
    for (uint32_t k = tid; k <= M / 2u; k += kThreads) {
        const c2 A = z[pad(k)], B = z[pad((M - k) & (M - 1u))];
        const c2 s = A + cconj(B), it = mul_pi(cmul(W[k], A - cconj(B)));
        const c2 Xk = (s - it) * 0.5, Xmk = cconj(s + it) * 0.5;
        bins[2u * k] = Xk.x; bins[2u * k + 1u] = Xk.y;
        bins[2u * (M - k)] = Xmk.x; bins[2u * (M - k) + 1u] = Xmk.y;
    }
}

template <uint32_t M>
static void frame(const spectrum::Plan& p, const std::vector<float>& x, int64_t first, float* power, double* bins) {
    const uint32_t stride = buf_stride(2u * M);
    std::vector<c2> a(stride, mk(1e300, 1e300)), b(stride, mk(1e300, 1e300));      // (a read of an entry nobody wrote would show)
    const c2* W = reinterpret_cast<const c2*>(p.twiddles);
    auto fetch = [&](uint32_t i) -> float {
        const int64_t q = first + (int64_t)i;
        return q >= 0 && q < (int64_t)x.size() ? x[(size_t)q] : 0.0f;
    };
    for (uint32_t tid = 0; tid < kThreads; ++tid) spectrum::load_frame<M>(fetch, p.window, a.data(), tid);
    for (uint32_t q = 0; q < num_passes<M>(); ++q)
        for (uint32_t tid = 0; tid < kThreads; ++tid) run_pass<M>(q, a.data(), b.data(), tid, W);
    const c2* z = result<M>(a.data(), b.data());
    for (uint32_t tid = 0; tid < kThreads; ++tid) split_bins<M>(z, tid, W, bins);
    double* pw = spectrum::power_buffer<M>(a.data(), b.data());
    for (uint32_t tid = 0; tid < kThreads; ++tid) spectrum::split_power<M>(z, tid, W, pw);
    for (uint32_t tid = 0; tid < kThreads; ++tid) spectrum::store_columns(p, pw, tid, power);
}

int main(int argc, char** argv) {
    if (argc != 8) { std::fprintf(stderr, "usage: %s size hop center programme.f32 window.f64 power.f32 bins.f64\n", argv[0]); return 2; }
    const uint32_t size = (uint32_t)std::atoi(argv[1]), hop = (uint32_t)std::atoi(argv[2]), center = (uint32_t)std::atoi(argv[3]);
    if (!spectrum::spec_ok(size, hop, 0u, nullptr, nullptr)) { std::fprintf(stderr, "bad size or hop\n"); return 2; }
    const std::vector<char> xb = slurp(argv[4]), wb = slurp(argv[5]);
    std::vector<float> x(xb.size() / 4u);
    std::vector<double> win(size), tw(2u * size);
    if (wb.size() != size * sizeof(double)) { std::fprintf(stderr, "the window must hold `size` doubles\n"); return 2; }
    if (!x.empty()) memcpy(x.data(), xb.data(), x.size() * 4u);
    memcpy(win.data(), wb.data(), wb.size());
    make_twiddles(size, reinterpret_cast<c2*>(tw.data()));
    const uint32_t P = center ? size / 2u : 0u, cols = size / 2u + 1u;
    const spectrum::Plan p{size, hop, P, cols, 0u, win.data(), tw.data(), nullptr, nullptr, nullptr, nullptr};
    const uint64_t n = spectrum::frames_total(x.size(), size, hop, P);
    std::vector<float> power(n * cols);
    std::vector<double> bins(n * 2u * cols);
    for (uint64_t j = 0; j < n; ++j) {
        const int64_t first = (int64_t)(j * hop) - (int64_t)P;
        float* o = power.data() + j * cols;
        double* bn = bins.data() + j * 2u * cols;
        switch (size) {
            case 256:  frame<128>(p, x, first, o, bn); break;
            case 512:  frame<256>(p, x, first, o, bn); break;
            case 1024: frame<512>(p, x, first, o, bn); break;
            case 2048: frame<1024>(p, x, first, o, bn); break;
            default:   frame<2048>(p, x, first, o, bn); break;
        }
    }
    FILE* f = std::fopen(argv[6], "wb");
    if (!f) return 2;
    std::fwrite(power.data(), 4, power.size(), f);
    std::fclose(f);
    f = std::fopen(argv[7], "wb");
    if (!f) return 2;
    std::fwrite(bins.data(), 8, bins.size(), f);
    std::fclose(f);
    std::printf("{\"size\": %u, \"hop\": %u, \"frames\": %llu}\n", size, hop, (unsigned long long)n);
    return 0;
}
