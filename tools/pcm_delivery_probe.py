"""Delivery of an offline render, timed: elemhip_process_blocks_host (planar float32) against elemhip_process_blocks_pcm on the C4
workload (128 instances, mono roots, launch sets of 1024 blocks) and on C2 (2 channels, sets of 256). One process, specialize 2,
three repetitions of every leg, each after a warm-up call of the same size. `--float-only` runs just the float legs (the yardstick on
a tree without PCM delivery); `--pack-only` renders a few PCM sets and nothing else, for a kernel trace of its own."""
import sys, time; sys.path.insert(0, '.')
import numpy as np
from elementary_amd import graphs
from elementary_amd.runtime import Runtime

float_only, pack_only = "--float-only" in sys.argv, "--pack-only" in sys.argv
REPS = 3


def timed(fn):
    fn()
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter(); fn(); out.append(time.perf_counter() - t0)
    return out


def workload(name, roots, n_out, batch, sets):
    rt = Runtime(48000.0, 512, device=0); rt.set_option("specialize", 2); rt.set_option("batch_blocks", batch)
    assert rt.render(*roots)["result"] == 0
    frames = sets * batch * 512
    rt.process_blocks_host(None, n_out, 64 * 512)                # root fades settle: launch sets from here on
    if pack_only:
        rt.process_blocks_pcm(None, n_out, 1, frames, "s16"); rt.process_blocks_pcm(None, n_out, 1, frames, "s16")
        return
    out = np.zeros((n_out, frames), np.float32)
    legs = [("float planar (process_blocks_host)", lambda: rt.process_blocks_host(None, n_out, frames, out=out))]
    if not float_only:
        legs += [("pcm s16 G=1", lambda: rt.process_blocks_pcm(None, n_out, 1, frames, "s16")),
                 ("pcm s16 G=2", lambda: rt.process_blocks_pcm(None, n_out // 2, 2, frames, "s16")),
                 ("pcm f32 G=2", lambda: rt.process_blocks_pcm(None, n_out // 2, 2, frames, "f32")),
                 ("pcm s16 G=2 + planar floats", lambda: rt.process_blocks_pcm(None, n_out // 2, 2, frames, "s16", want_float=True)),
                 ("pcm s16 G=2 dither", lambda: rt.process_blocks_pcm(None, n_out // 2, 2, frames, "s16", dither_seed=1))]
    base = None
    for label, fn in legs:
        ts = timed(fn)
        rate = [n_out * frames / t / 1e9 for t in ts]
        med = sorted(ts)[1]
        base = med if base is None else base
        print(f"{name} {label:32s} ms {' '.join(f'{1e3 * t:8.2f}' for t in ts)}   G instance-samples/s {' '.join(f'{r:6.3f}' for r in rate)}"
              f"   median / float {med / base:5.3f}", flush=True)


workload("C4", [graphs.c4_instance(k) for k in range(128)], 128, 1024, 3)
workload("C2", graphs.c2_graph(), 2, 256, 8)
