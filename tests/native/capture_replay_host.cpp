// Host driver of elementary_amd/csrc/capture_replay.h for tests/test_capture_history_host.py: one relay window per input line,
//     <frames relayed> <pending ready flag: 0 / 1> <engine slices per host block> <entries> then per entry <block counter> <F mod 2^32> <E>
// — the node's per-block log as the kernels write it, oldest first, one entry per ENGINE block. Answered by one line
// "t <host block of the window> <take end>" per event and a closing "end <frames relayed>". The caller carries that count into the
// next window's line.
#include <cstdio>
#include <cinttypes>
#include <vector>

#include "capture_replay.h"

int main() {
    unsigned long long relayed;
    unsigned pending, perHost, take;
    while (std::scanf("%llu %u %u %u", &relayed, &pending, &perHost, &take) == 4) {
        std::vector<uint32_t> e((size_t)take * 4u, 0u);
        for (unsigned k = 0; k < take; ++k)
            if (std::scanf("%u %u %u", &e[4 * k], &e[4 * k + 1], &e[4 * k + 2]) != 3) return 1;
        evf::Window w;
        w.sliced = perHost > 1u; w.windowBlocks = take;
        if (w.sliced) for (unsigned s = perHost; s < take + perHost; s += perHost) w.hostEnds.push_back(s < take ? s : take);
        const std::vector<cpr::Entry> blocks = cpr::fold(w, e.data(), take);
        std::vector<cpr::Take> takes;
        const uint64_t end = cpr::replay(blocks.data(), blocks.size(), relayed, pending != 0u, takes);
        for (const cpr::Take& t : takes) std::printf("t %llu %llu\n", (unsigned long long)t.block, (unsigned long long)t.end);
        std::printf("end %llu\n", (unsigned long long)end);
        std::fflush(stdout);
    }
    return 0;
}
