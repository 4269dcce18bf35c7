"""Delivery at another sample rate, timed: the C4 workload (128 instances, mono roots, launch sets of 1024 blocks of 512 frames) in
one process, specialize 2, three repetitions of every leg, each after a warm-up call of the same size.
  pcm      elemhip_process_blocks_pcm (s16, two channels per stream, no float crosses the host link) at 48000 Hz with option
           "resample_rate" off and at 44100: the time per launch set and their ratio
  floats   the oversampling case: the engine at 176400 Hz delivering planar floats at 176400 (option off: what a caller who
           decimates on the CPU receives) against the same engine delivering 44100 (a quarter of the floats cross the host link)
Prints the bytes the converter's kernel moves per set (the set's output read once, the converted set written once; the table and
the overlap between tiles stay in L2) and the time they take at the 8 TB/s the project's rooflines use. (on - off) is NOT the
kernel's own time: it runs on the render's stream while the previous set's copy-out and delivery go on. The kernel's own time per
set is delegated to a kernel trace of a run of its own: `--kernel-only [rate-in rate-out]` renders a few converted sets and nothing
else (rocprofv3 --kernel-trace --stats -- python tools/resample_probe.py --kernel-only: the elemhip_resample rows, mean duration
per dispatch = per set)."""
import sys, time; sys.path.insert(0, '.')
from elementary_amd import graphs
from elementary_amd.runtime import Runtime

kernel_only = "--kernel-only" in sys.argv
REPS, N_OUT, BATCH, SETS, BS = 3, 128, 1024, 3, 512


def engine(fin, fout):
    rt = Runtime(float(fin), BS, device=0); rt.set_option("specialize", 2); rt.set_option("batch_blocks", BATCH)
    assert rt.render(*[graphs.c4_instance(k) for k in range(N_OUT)])["result"] == 0
    rt.process_blocks_host(None, N_OUT, 64 * BS)                 # root fades settle: launch sets from here on
    if fout:
        rt.set_option("resample_rate", fout)
    return rt


def timed(fn):
    fn()
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter(); fn(); out.append(time.perf_counter() - t0)
    return out


frames = SETS * BATCH * BS
if kernel_only:
    rates = [int(a) for a in sys.argv[1:] if a.isdigit()] or [48000, 44100]
    rt = engine(rates[0], rates[1])
    rt.process_blocks_pcm(None, N_OUT // 2, 2, frames, "s16"); rt.process_blocks_pcm(None, N_OUT // 2, 2, frames, "s16")
    print(rt.resample_read())
    sys.exit(0)


def leg(name, fin, fout, call):
    rt = engine(fin, fout)
    ts = timed(lambda: call(rt))
    med = sorted(ts)[1] / SETS
    print(f"{name:<44s} ms per call {' '.join(f'{1e3 * t:8.2f}' for t in ts)}   median per set of {BATCH} blocks {1e3 * med:7.3f} ms", flush=True)
    if fout:
        got = rt.resample_read()
        moved = N_OUT * BATCH * BS * 4 * (1.0 + got["up"] / got["down"])
        print(f"   {got['up']}/{got['down']}, {got['taps']} taps; the kernel moves {moved / 1e6:.0f} MB per set: {1e3 * moved / 8e12:.3f} ms at 8 TB/s; "
              f"{got['taps'] * N_OUT * BATCH * BS * got['up'] / got['down'] / 1e9:.2f} G fused multiply-adds per set")
    return med


pcm = lambda rt: rt.process_blocks_pcm(None, N_OUT // 2, 2, frames, "s16")
host = lambda rt: rt.process_blocks_host(None, N_OUT, frames)
off = leg("C4 pcm s16 G=2 at 48000, resample_rate off", 48000, 0, pcm)
on = leg("C4 pcm s16 G=2 at 48000, resample_rate 44100", 48000, 44100, pcm)
print(f"set time on / off {on / off:5.3f}   (on - off) {1e3 * (on - off):7.3f} ms per set")
off4 = leg("C4 floats at 176400, resample_rate off", 176400, 0, host)
on4 = leg("C4 floats at 176400, resample_rate 44100", 176400, 44100, host)
print(f"oversampled render, set time delivering 44100 / delivering 176400 {on4 / off4:5.3f}   ({1e3 * (on4 - off4):+8.3f} ms per set)")
print("the kernel's own time per set: see the kernel trace of `--kernel-only` (not timed here)")
