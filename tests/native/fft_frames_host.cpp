// tests/native/fft_frames_host.cpp — the transform core of the `fft` node's relay (elementary_amd/csrc/fft_frames.h) run on the HOST:
// the 128 threads of a workgroup are emulated phase by phase (every phase between two barriers is a loop over tid).
//   fft_frames_host <size> <frames.f32> <spectra.f32>
// frames.f32: n frames of `size` raw float32 samples; every frame is laid into an 8192-frame ring so that it WRAPS, windowed and
// transformed as the kernel does it; spectra.f32 receives real[size/2+1] | imag[size/2+1] per frame.
//   clang++ -std=c++17 -O2 -ffp-contract=off -I elementary_amd/csrc tests/native/fft_frames_host.cpp -o fft_frames_host
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fft_frames.h"

using namespace ffr;

template <uint32_t M>
static void transform(const float* ring, uint32_t read, const double* win, const c2* W, float* re, float* im) {
    std::vector<c2> a(kBuf, mk(0, 0)), b(kBuf, mk(0, 0));
    for (uint32_t tid = 0; tid < kThreads; ++tid) load_frame<M>(ring, read, win, a.data(), tid);
    for (uint32_t p = 0; p < num_passes<M>(); ++p)
        for (uint32_t tid = 0; tid < kThreads; ++tid) run_pass<M>(p, a.data(), b.data(), tid, W);
    const c2* z = result<M>(a.data(), b.data());
    for (uint32_t tid = 0; tid < kThreads; ++tid) store_bins<M>(z, tid, W, re, im);
}

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: %s size frames.f32 spectra.f32\n", argv[0]); return 2; }
    const uint32_t size = (uint32_t)std::atoi(argv[1]);
    if (!size_ok(size)) { std::fprintf(stderr, "size must be 256, 512, 1024, 2048 or 4096\n"); return 2; }
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<float> frames;
    float tmp[4096];
    for (size_t got; (got = std::fread(tmp, 4, 4096, f)) > 0;) frames.insert(frames.end(), tmp, tmp + got);
    std::fclose(f);
    const size_t n = frames.size() / size;
    std::vector<double> win(size);
    std::vector<c2> W(size);
    make_window(size, win.data());
    make_twiddles(size, W.data());
    const uint32_t bins = size / 2u + 1u;
    std::vector<float> out(n * 2u * bins), ring(kRing);
    for (size_t k = 0; k < n; ++k) {
        const uint32_t read = (kRing - size / 2u + 37u * (uint32_t)k) & (kRing - 1u);     // the frame crosses the end of the ring
        for (auto& v : ring) v = 1e9f;                                                     // (a read outside the frame would show)
        for (uint32_t i = 0; i < size; ++i) ring[(read + i) & (kRing - 1u)] = frames[k * size + i];
        float* re = out.data() + k * 2u * bins;
        float* im = re + bins;
        switch (size) {
            case 256:  transform<128>(ring.data(), read, win.data(), W.data(), re, im); break;
            case 512:  transform<256>(ring.data(), read, win.data(), W.data(), re, im); break;
            case 1024: transform<512>(ring.data(), read, win.data(), W.data(), re, im); break;
            case 2048: transform<1024>(ring.data(), read, win.data(), W.data(), re, im); break;
            default:   transform<2048>(ring.data(), read, win.data(), W.data(), re, im); break;
        }
    }
    f = std::fopen(argv[3], "wb");
    if (!f) return 2;
    std::fwrite(out.data(), 4, out.size(), f);
    std::fclose(f);
    std::printf("{\"size\": %u, \"frames\": %zu}\n", size, n);
    return 0;
}
