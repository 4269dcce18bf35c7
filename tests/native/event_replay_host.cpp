// Host driver of elementary_amd/csrc/event_replay.h for tests/test_event_history_host.py: one relay window per input line,
//     <frames written> <read position> <block> <size> <cmp: 0 = more than (scope), 1 = at least (fft)> <blocks>
// answered by one line "e <block of the window> <first frame>" per emitted frame and a closing "end <frames written> <read position>".
// The caller carries the end positions into the next window's line.
#include <cstdio>
#include <cinttypes>

#include "event_replay.h"

int main() {
    unsigned long long written;
    unsigned read, block, size, cmp, blocks;
    while (std::scanf("%llu %u %u %u %u %u", &written, &read, &block, &size, &cmp, &blocks) == 6) {
        evr::Pos p;
        p.written = written; p.read = read;
        p = evr::replay(p, block, size, cmp ? evr::kAtLeast : evr::kMoreThan, blocks,
                        [](uint32_t b, uint64_t first) { std::printf("e %u %lld\n", b, (long long)first); });
        std::printf("end %llu %u\n", (unsigned long long)p.written, p.read);
        std::fflush(stdout);
    }
    return 0;
}
