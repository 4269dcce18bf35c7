"""The true-peak limiter, timed: the C4 workload (128 instances, mono roots, launch sets of 1024 blocks of 512 frames at 48000 Hz) in
one process, specialize 2, delivered as s16 (two channels per stream, no float crosses the host link) with option "limiter" off and
on — a look-ahead of 1.5 ms (72 frames), channels linked in pairs, 12 dB of gain so that the limiter works most of the time.
Two engines, one per leg, warmed by a call of the same size; then ROUNDS rounds that ALTERNATE the legs (off, on, off, on, ...), so
that drift of clocks and of the host hits both alike; per leg the median and the spread (min .. max) over the rounds, per launch set.
Prints the bytes the limiter's kernels move per set and the time they take at the 8 TB/s the project's rooflines use. (on - off) is
NOT the kernels' own time: they run on the render's stream while the previous set's copy-out and delivery go on. The kernels' own
time per set is delegated to a kernel trace of a run of its own: `--kernel-only` renders a few limited sets and nothing else
(rocprofv3 --kernel-trace --stats -- python tools/limiter_probe.py --kernel-only: the elemhip_limiter_* rows, mean duration per
dispatch = per set)."""
import sys, time; sys.path.insert(0, '.')
from elementary_amd import graphs
from elementary_amd.runtime import Runtime

kernel_only = "--kernel-only" in sys.argv
ROUNDS, N_OUT, BATCH, SETS, BS, RATE = 9, 128, 1024, 3, 512, 48000.0
LOOKAHEAD_MS, LINK, GAIN_DB = 1.5, 2, 12.0


def engine(limit):
    rt = Runtime(RATE, BS, device=0); rt.set_option("specialize", 2); rt.set_option("batch_blocks", BATCH)
    assert rt.render(*[graphs.c4_instance(k) for k in range(N_OUT)])["result"] == 0
    rt.process_blocks_host(None, N_OUT, 64 * BS)                 # root fades settle: launch sets from here on
    if limit:
        rt.set_option("limiter_lookahead_ms", LOOKAHEAD_MS); rt.set_option("limiter_link", LINK); rt.set_option("limiter_gain_db", GAIN_DB)
        rt.set_option("limiter", 1)
    return rt


frames = SETS * BATCH * BS
call = lambda rt: rt.process_blocks_pcm(None, N_OUT // 2, 2, frames, "s16")
if kernel_only:
    rt = engine(True)
    call(rt); call(rt)
    print(rt.limiter_read())
    sys.exit(0)

legs = {"off": engine(False), "on": engine(True)}
for rt in legs.values():
    call(rt)                                                     # warm-up: buffers allocated, kernels loaded
times = {name: [] for name in legs}
for _ in range(ROUNDS):
    for name, rt in legs.items():
        t0 = time.perf_counter(); call(rt); times[name].append((time.perf_counter() - t0) / SETS)
for name, ts in times.items():
    s = sorted(ts)
    print(f"C4 pcm s16 G=2 at 48000, limiter {name:<3s}  ms per set of {BATCH} blocks, by round: {' '.join(f'{1e3 * t:7.3f}' for t in ts)}   "
          f"median {1e3 * s[len(s) // 2]:7.3f}  min {1e3 * s[0]:7.3f}  max {1e3 * s[-1]:7.3f}", flush=True)
off, on = sorted(times["off"])[ROUNDS // 2], sorted(times["on"])[ROUNDS // 2]
got = legs["on"].limiter_read()
samples, groups = N_OUT * BATCH * BS, got["groups"]
# detect reads the set (4 B a sample) and writes dm (8 B a frame and group); release reads and writes it; apply reads d and the set
# and writes the limited set
moved = samples * 4 * 3 + groups * BATCH * BS * 8 * 4
print(f"set time on / off {on / off:5.3f}   (on - off) {1e3 * (on - off):7.3f} ms per set; D = {got['lookahead_frames']}, {groups} groups; "
      f"limited share {float(got['limited_frames'].sum()) / (groups * got['frames']):.3f}; the kernels move {moved / 1e6:.0f} MB per set: "
      f"{1e3 * moved / 8e12:.3f} ms at 8 TB/s")
print("the kernels' own time per set: see the kernel trace of `--kernel-only` (not timed here)")
