// Host driver of elementary_amd/csrc/event_fold.h for tests/test_event_fold_host.py: one request per input line, every number an
// unsigned integer (floats travel as their bit patterns). A window is "<sliced> <windowBlocks> <n> <hostEnds x n>".
//     wraps <pushes>                                             -> "<0|1>"
//     block <window> <fromEnd>                                   -> "<host block>"
//     meter <window> <blockwise> <take> <(min max) x take>       -> "g <block> <min> <max>" per readout, "end"
//     snap  <window> <blk> <take> <(block value pushes) x take>  -> "s <block> <value>" per readout, "end"
//     scope <size> <n> <(block first) x n>                       -> "r <first> <frames> <at>" per run, "e <block> <first> <run> <offset>"
//                                                                   per emit, "end <span>"
//     avail <w> <r> <mask>                                       -> "<entries>"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "event_fold.h"

static unsigned long long num() { unsigned long long v = 0; if (std::scanf("%llu", &v) != 1) std::exit(2); return v; }
static evf::Window window() {
    evf::Window w;
    w.sliced = num() != 0; w.windowBlocks = num();
    for (unsigned long long n = num(); n; --n) w.hostEnds.push_back(num());
    return w;
}
static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "wraps")) std::printf("%d\n", evf::wraps_to_empty((uint32_t)num()) ? 1 : 0);
        else if (!std::strcmp(cmd, "block")) { const evf::Window w = window(); std::printf("%llu\n", (unsigned long long)w.block_of(num())); }
        else if (!std::strcmp(cmd, "meter")) {
            const evf::Window w = window();
            const bool blockwise = num() != 0;
            const uint32_t take = (uint32_t)num();
            std::vector<uint32_t> e((size_t)take * 4, 0u);
            for (uint32_t k = 0; k < take; ++k) { e[4 * k + 1] = (uint32_t)num(); e[4 * k + 2] = (uint32_t)num(); }
            for (const evf::MeterOut& g : evf::fold_meter(w, e.data(), take, blockwise)) std::printf("g %llu %u %u\n", (unsigned long long)g.block, bits(g.mn), bits(g.mx));
            std::printf("end\n");
        } else if (!std::strcmp(cmd, "snap")) {
            const evf::Window w = window();
            const uint32_t blk = (uint32_t)num(), take = (uint32_t)num();
            std::vector<uint32_t> e((size_t)take * 4, 0u);
            for (uint32_t k = 0; k < take; ++k) { e[4 * k] = (uint32_t)num(); e[4 * k + 1] = (uint32_t)num(); e[4 * k + 2] = (uint32_t)num(); }
            for (const evf::SnapshotOut& s : evf::fold_snapshot(w, e.data(), take, blk)) std::printf("s %llu %u\n", (unsigned long long)s.block, bits(s.value));
            std::printf("end\n");
        } else if (!std::strcmp(cmd, "scope")) {
            const uint64_t size = num();
            evf::ScopeRuns sr;
            for (unsigned long long n = num(); n; --n) { const uint64_t block = num(), first = num(); sr.add(block, first, size); }
            sr.layout();
            for (const evf::ScopeRuns::Run& r : sr.runs) std::printf("r %llu %llu %zu\n", (unsigned long long)r.first, (unsigned long long)r.frames, r.at);
            for (const evf::ScopeRuns::Emit& e : sr.emits) std::printf("e %llu %llu %zu %zu\n", (unsigned long long)e.block, (unsigned long long)e.first, e.run, sr.offset(e));
            std::printf("end %zu\n", sr.span);
        } else if (!std::strcmp(cmd, "avail")) { const uint32_t w = (uint32_t)num(), r = (uint32_t)num(), mask = (uint32_t)num(); std::printf("%u\n", evf::capture_avail(w, r, mask)); }
        else return 2;
        std::fflush(stdout);
    }
    return 0;
}
