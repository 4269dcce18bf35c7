"""FLAC delivery of an offline render, timed: elemhip_process_blocks_flac (16 bits) against elemhip_process_blocks_pcm (s16) in the same
process, on the C4 workload (128 instances, mono streams, launch sets of 1024 blocks) and on a 2-channel render (C2, one stereo stream,
sets of 256). Rounds alternate the two legs after a warm-up call of each (a host clock around calls that end with both streams
synchronised); the medians are compared. Reported besides: the bytes that crossed the host link per leg (PCM: the packed streams;
FLAC: the frames and their length table) and the compression ratio on the probe's programme.

`--flac-only` renders a few FLAC sets and nothing else: the run for a kernel trace of its own (rocprofv3 --kernel-trace --stats),
where elemhip_flac_stage, elemhip_flac_encode and elemhip_flac_assemble show their own times."""
import sys, time; sys.path.insert(0, '.')
from elementary_amd import graphs
from elementary_amd.runtime import Runtime

flac_only = "--flac-only" in sys.argv
ROUNDS = 5


def workload(name, roots, S, G, batch, sets, flac_frame):
    rt = Runtime(48000.0, 512, device=0); rt.set_option("specialize", 2); rt.set_option("batch_blocks", batch); rt.set_option("flac_frame", flac_frame)
    assert rt.render(*roots)["result"] == 0
    n_out, frames = S * G, sets * batch * 512
    rt.process_blocks_host(None, n_out, 64 * 512)                # root fades settle: launch sets from here on

    def pcm():
        streams, _, _ = rt.process_blocks_pcm(None, S, G, frames, "s16")
        return sum(a.nbytes for a in streams)

    def flac():
        streams, _ = rt.process_blocks_flac(None, S, G, frames, 16)
        return sum(len(b) for b in streams) + 4 * S * (frames // flac_frame + 1)

    flac()                                                       # warm-up (and the buffers' allocation)
    if flac_only:
        flac()
        return
    pcm()
    t = {"pcm": [], "flac": []}
    nbytes = {}
    for _ in range(ROUNDS):
        for label, fn in (("pcm", pcm), ("flac", flac)):
            t0 = time.perf_counter(); nbytes[label] = fn(); t[label].append(time.perf_counter() - t0)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    for label in ("pcm", "flac"):
        print(f"{name} flac_frame {flac_frame} {label:5s} ms/set {' '.join(f'{1e3 * x / sets:8.2f}' for x in t[label])}   median {1e3 * med[label] / sets:8.2f}"
              f"   G instance-samples/s {n_out * frames / med[label] / 1e9:6.3f}   bytes over the link per call {nbytes[label]}", flush=True)
    print(f"{name} flac_frame {flac_frame} median flac / pcm {med['flac'] / med['pcm']:5.3f}   compression flac / s16 {nbytes['flac'] / nbytes['pcm']:5.3f}", flush=True)


workload("C4", [graphs.c4_instance(k) for k in range(128)], 128, 1, 1024, 2, 4096)
workload("C2", graphs.c2_graph(), 1, 2, 256, 8, 4096)
