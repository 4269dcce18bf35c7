"""The loudness meter, timed: elemhip_process_blocks_pcm (s16, two channels per stream, no float crosses the host link) on the C4
workload (128 instances, mono roots, launch sets of 1024 blocks) with option "loudness_meter" off and on, in one process, specialize 2,
three repetitions of every leg, each after a warm-up call of the same size. Prints the time per launch set off and on and their
ratio, the bytes the meter's kernels read per set (three passes over the set's output: peaks, pass one, pass two) and the time those
bytes take at the 8 TB/s the project's rooflines use. (on - off) is NOT the kernels' own time: they run on the render's stream while
the previous set's copy-out and delivery go on. The kernels' own time per set is delegated to a kernel trace of a run of its own:
`--meter-only` renders a few metered sets and nothing else (rocprofv3 --kernel-trace --stats -- python tools/loudness_probe.py
--meter-only: the five elemhip_loudness_* rows, mean duration per dispatch = per set)."""
import sys, time; sys.path.insert(0, '.')
from elementary_amd import graphs
from elementary_amd.runtime import Runtime

meter_only = "--meter-only" in sys.argv
REPS, N_OUT, BATCH, SETS, BS = 3, 128, 1024, 3, 512


def engine(meter):
    rt = Runtime(48000.0, BS, device=0); rt.set_option("specialize", 2); rt.set_option("batch_blocks", BATCH)
    if meter:
        rt.set_option("loudness_meter", 1)
    assert rt.render(*[graphs.c4_instance(k) for k in range(N_OUT)])["result"] == 0
    rt.process_blocks_host(None, N_OUT, 64 * BS)                 # root fades settle: launch sets from here on
    return rt


def timed(fn):
    fn()
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter(); fn(); out.append(time.perf_counter() - t0)
    return out


frames = SETS * BATCH * BS
if meter_only:
    rt = engine(True)
    rt.process_blocks_pcm(None, N_OUT // 2, 2, frames, "s16"); rt.process_blocks_pcm(None, N_OUT // 2, 2, frames, "s16")
    print(rt.loudness_read()["sub_blocks"], "sub-blocks metered")
    sys.exit(0)
med = {}
for meter in (False, True):
    rt = engine(meter)
    ts = timed(lambda: rt.process_blocks_pcm(None, N_OUT // 2, 2, frames, "s16"))
    med[meter] = sorted(ts)[1] / SETS
    print(f"C4 pcm s16 G=2, loudness_meter {'on ' if meter else 'off'}  ms per call {' '.join(f'{1e3 * t:8.2f}' for t in ts)}   "
          f"median per set of {BATCH} blocks {1e3 * med[meter]:7.3f} ms", flush=True)
    if meter:
        got = rt.loudness_read()
        print(f"   metered {got['frames']} frames x {got['channels']} channels, {got['sub_blocks']} sub-blocks")
read = 3 * N_OUT * BATCH * BS * 4
print(f"set time on / off {med[True] / med[False]:5.3f}   (on - off) {1e3 * (med[True] - med[False]):7.3f} ms per set")
print("the kernels' own time per set: see the kernel trace of `--meter-only` (not timed here)")
print(f"the meter's kernels read {read / 1e6:.0f} MB per set: {1e3 * read / 8e12:.3f} ms at 8 TB/s")
