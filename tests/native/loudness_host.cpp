// loudness_host.cpp — elementary_amd/csrc/loudness.h compiled for the host: the loudness kernels' schedule (loudness.hip) emulated
// thread by thread — the peaks kernel frame by frame, pass one and pass two segment by segment, the scan wave by wave with its
// 64 lanes' shuffles, the combine sub-block by sub-block — over launch sets laid out [block][channel][blockSize], against the
// header's scalar loop meter_host(). Block sizes 32, 341, 350 and 512; sets of 1, 3 and 8 blocks; programmes that end on a block and
// 37 frames into one; a programme cut into 1, 2 and 5 calls; three sample rates (hops of 400, 800 and 4410 frames).
// Every programme's frames go to <dir>/<name>.f32 (planar float32, the unique channels) so that the test can hold the printed
// series to its own reference; the anchors of the standards are generated here too. Usage: loudness_host <dir>; prints one JSON line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "loudness.h"

namespace ld = loudness;

struct Meter {
    ld::Plan plan;
    std::vector<ld::ChannelState> st;
    std::vector<std::vector<double>> series;
    uint64_t frames = 0;
    Meter(double sr, size_t ch) : st(ch), series(ch) { ld::make_plan(sr, plan); std::memset(st.data(), 0, ch * sizeof(ld::ChannelState)); }
};

// one launch set, as launch_loudness runs it: `src` = [block][nCh][bs], `valid` delivered frames
static void emulate_set(Meter& m, const float* src, uint32_t bs, uint32_t nCh, uint32_t valid) {
    const ld::Plan& p = m.plan;
    const uint32_t q0 = (uint32_t)(m.frames % p.hop), numSegs = ld::segment_count(valid, p.L);
    std::vector<double> segState((size_t)numSegs * 4), segEnergy((size_t)numSegs * 2);
    for (uint32_t c = 0; c < nCh; ++c) {
        ld::ChannelState& st = m.st[c];
        // peaks: thread <-> frame, the carried frames as the previous set left them
        double best = ld::bits_double(st.truePeakBits);
        uint32_t sample = st.samplePeakBits;
        for (uint32_t f = 0; f < valid; ++f) {
            double w[ld::kPhaseTaps];
            for (uint32_t k = 0; k < ld::kPhaseTaps; ++k) w[k] = ld::window_frame(src, bs, nCh, c, st.hist, f, k);
            const double v = ld::peak_at(p, w);
            best = v > best ? v : best;
            const float xf = (float)w[0];
            uint32_t a; std::memcpy(&a, &xf, 4); a &= 0x7FFFFFFFu;
            sample = a > sample ? a : sample;
        }
        st.truePeakBits = ld::double_bits(best); st.samplePeakBits = sample;
        // pass one: thread <-> segment (the last one's end state is never used)
        for (uint32_t k = 0; k + 1 < numSegs; ++k) ld::pass_one(p, ld::cursor_at(src, bs, nCh, c, k * p.L), p.L, &segState[4 * (size_t)k]);
        // scan: one wave, 64 segments per step
        double seed[4] = {st.s[0], st.s[1], st.s[2], st.s[3]};
        for (uint32_t k0 = 0; k0 < numSegs; k0 += 64u) {
            double v[64][4];
            for (uint32_t lane = 0; lane < 64u; ++lane)
                for (int r = 0; r < 4; ++r) v[lane][r] = k0 + lane + 1u < numSegs ? segState[4 * (size_t)(k0 + lane) + r] : 0.0;
            ld::scan_fold(p.power[0], v[0], seed);
            for (uint32_t i = 0; i < ld::kScanSteps; ++i) {
                double o[64][4];
                std::memcpy(o, v, sizeof v);                       // (a shuffle reads every lane's value of before the step)
                for (uint32_t lane = 1u << i; lane < 64u; ++lane) ld::scan_fold(p.power[i], v[lane], o[lane - (1u << i)]);
            }
            for (uint32_t lane = 0; lane < 64u && k0 + lane < numSegs; ++lane)
                for (int r = 0; r < 4; ++r) segState[4 * (size_t)(k0 + lane) + r] = lane == 0u ? seed[r] : v[lane - 1u][r];
            for (int r = 0; r < 4; ++r) seed[r] = v[63][r];
        }
        float next[ld::kHistory];
        for (uint32_t j = 0; j < ld::kHistory; ++j) next[j] = ld::history_next(src, bs, nCh, c, st.hist, valid, j);
        std::memcpy(st.hist, next, sizeof next);
        // pass two: thread <-> segment
        for (uint32_t k = 0; k < numSegs; ++k) {
            double s[4];
            std::memcpy(s, &segState[4 * (size_t)k], sizeof s);
            ld::pass_two(p, ld::cursor_at(src, bs, nCh, c, k * p.L), ld::segment_frames(k, valid, p.L), ld::segment_first(k, q0, p.hop, p.L), s, &segEnergy[2 * (size_t)k]);
            if (k + 1 == numSegs) std::memcpy(st.s, s, sizeof s);
        }
        // combine: thread <-> sub-block
        const double carried = st.partial;
        const uint32_t touched = ld::subblocks_touched(q0, valid, p.hop), complete = ld::subblocks_complete(q0, valid, p.hop);
        for (uint32_t j = 0; j < touched; ++j) {
            const double sum = ld::subblock_sum(segEnergy.data(), j, carried, q0, valid, p.hop, p.L);
            if (j < complete) m.series[c].push_back(sum / (double)p.hop); else st.partial = sum;
        }
        if (touched == complete) st.partial = 0.0;
    }
    m.frames += valid;
}

// a call of `n` frames of planar `x` (rows `stride` apart) as renderHostSets cuts it: sets of `setBlocks` blocks, the frames behind
// the call's last one poisoned (nobody may read them)
static void emulate_call(Meter& m, const float* x, size_t stride, uint32_t nCh, size_t n, uint32_t bs, uint32_t setBlocks) {
    const size_t numBlocks = (n + bs - 1) / bs;
    std::vector<float> set((size_t)setBlocks * nCh * bs);
    for (size_t b0 = 0; b0 < numBlocks; b0 += setBlocks) {
        const size_t nb = std::min<size_t>(setBlocks, numBlocks - b0), valid = std::min(nb * bs, n - b0 * bs);
        for (size_t b = 0; b < nb; ++b)
            for (uint32_t c = 0; c < nCh; ++c)
                for (uint32_t f = 0; f < bs; ++f) {
                    const size_t at = (b0 + b) * bs + f;
                    set[(b * nCh + c) * bs + f] = at < n ? x[c * stride + at] : 1.0e30f;
                }
        emulate_set(m, set.data(), bs, nCh, (uint32_t)valid);
    }
}

static void scalar_call(Meter& m, const float* x, size_t stride, uint32_t nCh, size_t n) {
    for (uint32_t c = 0; c < nCh; ++c) ld::meter_host(m.plan, m.st[c], x + c * stride, n, m.frames, [&](double ms) { m.series[c].push_back(ms); });
    m.frames += n;
}

static std::string num(double v) {
    char buf[40];
    if (std::isinf(v)) return v < 0 ? "\"-inf\"" : "\"inf\"";
    std::snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}
static std::string results(const Meter& m) {
    std::string s = "\"series\":[";
    for (size_t c = 0; c < m.series.size(); ++c) {
        s += c ? ",[" : "[";
        for (size_t j = 0; j < m.series[c].size(); ++j) { if (j) s += ","; s += num(m.series[c][j]); }
        s += "]";
    }
    s += "],\"true_peak\":[";
    for (size_t c = 0; c < m.st.size(); ++c) { if (c) s += ","; s += num(ld::peak_with_tail(m.plan, m.st[c])); }
    s += "],\"sample_peak\":[";
    for (size_t c = 0; c < m.st.size(); ++c) { float f; std::memcpy(&f, &m.st[c].samplePeakBits, 4); if (c) s += ","; s += num((double)f); }
    s += "],\"frames\":" + std::to_string(m.frames);
    return s;
}
static std::string gated(const Meter& m) {
    const size_t ch = m.series.size(), n = ch ? m.series[0].size() : 0;
    std::vector<double> flat(ch * n);
    for (size_t c = 0; c < ch && n; ++c) std::memcpy(flat.data() + c * n, m.series[c].data(), n * sizeof(double));
    const ld::Gated g = ld::gate(flat.data(), ch, n, nullptr);
    return "\"integrated\":" + num(g.integrated) + ",\"momentary_max\":" + num(g.momentaryMax) + ",\"short_term_max\":" + num(g.shortTermMax);
}

struct Emu { uint32_t bs, setBlocks, calls; };
static std::string g_dir, g_json;
static bool g_first = true;

// the unique channels `uniq` [u][frames] and which of them each channel is; the scalar loop over the whole programme, then every
// emulation over the programme cut into calls
static void programme(const std::string& name, double sr, const std::vector<std::vector<float>>& uniq, const std::vector<int>& map, const std::vector<Emu>& emus) {
    const size_t n = uniq[0].size(), ch = map.size();
    FILE* f = std::fopen((g_dir + "/" + name + ".f32").c_str(), "wb");
    if (!f) { std::perror("fopen"); std::exit(2); }
    for (const auto& u : uniq) if (std::fwrite(u.data(), 4, n, f) != n) { std::perror("fwrite"); std::exit(2); }
    std::fclose(f);
    std::vector<float> x(ch * n);
    for (size_t c = 0; c < ch; ++c) std::memcpy(x.data() + c * n, uniq[(size_t)map[c]].data(), n * 4);
    Meter scalar(sr, ch);
    scalar_call(scalar, x.data(), n, (uint32_t)ch, n);
    g_json += std::string(g_first ? "" : ",") + "{\"name\":\"" + name + "\",\"sr\":" + num(sr) + ",\"hop\":" + std::to_string(scalar.plan.hop) +
              ",\"unique\":" + std::to_string(uniq.size()) + ",\"map\":[";
    g_first = false;
    for (size_t c = 0; c < ch; ++c) g_json += (c ? "," : "") + std::to_string(map[c]);
    g_json += "]," + results(scalar) + "," + gated(scalar) + ",\"emulations\":[";
    for (size_t e = 0; e < emus.size(); ++e) {
        Meter m(sr, ch);
        // uneven cuts: call i of `calls` ends at n * (i + 1)^2 / calls^2, moved off block boundaries
        size_t at = 0;
        for (uint32_t i = 0; i < emus[e].calls; ++i) {
            size_t end = i + 1 == emus[e].calls ? n : n * (i + 1) * (i + 1) / ((size_t)emus[e].calls * emus[e].calls) + 5;
            if (end > n) end = n;
            emulate_call(m, x.data() + at, n, (uint32_t)ch, end - at, emus[e].bs, emus[e].setBlocks);
            at = end;
        }
        g_json += std::string(e ? "," : "") + "{\"bs\":" + std::to_string(emus[e].bs) + ",\"set_blocks\":" + std::to_string(emus[e].setBlocks) +
                  ",\"calls\":" + std::to_string(emus[e].calls) + "," + results(m) + "}";
    }
    g_json += "]}";
}

static std::vector<float> tone(double sr, double freq, double amp, size_t n, double phase = 0.0) {
    std::vector<float> x(n);
    const double pi = 3.14159265358979323846;
    for (size_t i = 0; i < n; ++i) x[i] = (float)(amp * std::sin(2.0 * pi * freq * (double)i / sr + phase));
    return x;
}
static double db(double d) { return std::pow(10.0, d / 20.0); }

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: loudness_host <dir>\n"); return 2; }
    g_dir = argv[1];
    g_json = "{\"programmes\":[";
    const double pi = 3.14159265358979323846;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();

    // ---- the lane schedule: noise, three channels (the third with non-finite frames), every block size / end / rate ----
    const uint32_t sizes[4] = {32, 341, 350, 512};
    for (uint32_t bs : sizes)
        for (uint32_t cut = 0; cut < 2; ++cut) {
            const size_t n = (size_t)21 * bs + (cut ? 37 : 0);
            std::vector<std::vector<float>> u(3, std::vector<float>(n));
            uint32_t state = 12345u + bs * 7u + cut;
            for (auto& chn : u)
                for (size_t i = 0; i < n; ++i) { state = state * 1664525u + 1013904223u; chn[i] = ((float)(int32_t)(state >> 8) * (1.0f / 8388608.0f) - 1.0f) * 0.7f; }
            for (size_t i = 0; i < n; ++i) u[1][i] *= (float)(0.5 + 0.5 * std::sin(2.0 * pi * (double)i / 997.0));
            u[2][n / 3] = nan; u[2][n / 2] = inf; u[2][n - 2] = -inf; u[2][7] = nan;
            std::vector<Emu> emus;
            for (uint32_t sb : {1u, 3u, 8u}) for (uint32_t calls : {1u, 2u, 5u}) emus.push_back(Emu{bs, sb, calls});
            for (double sr : {4000.0, 8000.0, 44100.0})
                programme("noise_" + std::to_string(bs) + (cut ? "_cut_" : "_whole_") + std::to_string((int)sr), sr, u, {0, 1, 2}, emus);
        }
    // ---- a non-finite frame meters as 0 ----
    {
        std::vector<float> a = tone(8000.0, 440.0, 0.5, 4000), b = a;
        for (size_t i : {100u, 1999u, 2000u, 3999u}) { a[i] = i & 1u ? nan : inf; b[i] = 0.0f; }
        programme("nonfinite_a", 8000.0, {a}, {0}, {Emu{128, 3, 2}});
        programme("nonfinite_b", 8000.0, {b}, {0}, {Emu{128, 3, 2}});
    }
    // ---- silence, and a programme shorter than a gating block ----
    programme("silence", 48000.0, {std::vector<float>(48000, 0.0f)}, {0}, {Emu{512, 8, 2}});
    programme("short", 48000.0, {tone(48000.0, 1000.0, 0.5, 16800)}, {0}, {Emu{512, 8, 1}});
    // ---- anchors of the standards, 48 kHz ----
    const double sr = 48000.0;
    const std::vector<Emu> big = {Emu{512, 8, 2}};
    programme("sine_997_0dbfs", sr, {tone(sr, 997.0, 1.0, 20 * 48000)}, {0}, big);
    programme("tech3341_case1", sr, {tone(sr, 1000.0, db(-23.0), 20 * 48000)}, {0, 0}, big);
    for (int k = 3; k <= 4; ++k) {
        const double ends = k == 3 ? -36.0 : -72.0;
        std::vector<float> x = tone(sr, 1000.0, 1.0, 80 * 48000);
        for (size_t i = 0; i < x.size(); ++i) x[i] = (float)((double)x[i] * db(i < 10u * 48000u || i >= 70u * 48000u ? ends : -23.0));
        programme("tech3341_case" + std::to_string(k), sr, {x}, {0, 0}, big);
    }
    // ---- true peak: 4800-frame tones of amplitude 0.5 with a 480-frame raised-cosine fade at both ends ----
    const double tp[4][2] = {{sr / 4.0, 45.0}, {sr / 4.0, 67.0}, {sr / 6.0, 0.0}, {sr / 8.0, 45.0}};
    for (int k = 0; k < 4; ++k) {
        std::vector<float> x = tone(sr, tp[k][0], 0.5, 4800, tp[k][1] * pi / 180.0);
        for (size_t i = 0; i < 480; ++i) {
            const double g = 0.5 * (1.0 - std::cos(pi * (double)i / 480.0));
            x[i] = (float)((double)x[i] * g); x[4799 - i] = (float)((double)x[4799 - i] * g);
        }
        programme("true_peak_" + std::to_string(k), sr, {x}, {0}, {Emu{341, 3, 2}, Emu{512, 8, 1}});
    }
    // ---- the coefficients at 48 kHz ----
    const ld::Biquad s = ld::shelf_coeffs(48000.0), h = ld::highpass_coeffs(48000.0);
    g_json += "],\"shelf\":[" + num(s.b0) + "," + num(s.b1) + "," + num(s.b2) + "," + num(s.a1) + "," + num(s.a2) + "],\"highpass\":[" +
              num(h.b0) + "," + num(h.b1) + "," + num(h.b2) + "," + num(h.a1) + "," + num(h.a2) + "]}";
    std::puts(g_json.c_str());
    return 0;
}
