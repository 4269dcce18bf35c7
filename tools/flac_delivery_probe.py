"""FLAC delivery of an offline render, timed: elemhip_process_blocks_flac (16 bits) against elemhip_process_blocks_pcm (s16) in the same
process, on the C4 workload (128 instances, mono streams, launch sets of 1024 blocks) and on a 2-channel render (C2, one stereo stream,
sets of 256). Rounds alternate the two legs after a warm-up call of each (a host clock around calls that end with both streams
synchronised); the medians are compared. Reported besides: the bytes that crossed the host link per leg (PCM: the packed streams;
FLAC: the frames and their length table) and the compression ratio on the probe's programme.

`--flac-only` renders a few FLAC sets and nothing else: the run for a kernel trace of its own (rocprofv3 --kernel-trace --stats),
where elemhip_flac_stage, elemhip_flac_encode and elemhip_flac_assemble show their own times.

`--lpc-order P` (1 .. 12) compares FLAC delivery with option flac_lpc_order = P against FLAC delivery without (order 0) instead: two
engines that render the same programme, the legs alternating in the same way, set time and bytes of one relative to the other. With
`--flac-only` only the engine with the order renders.

`--md5` compares FLAC delivery with option flac_md5 = 1 (the STREAMINFO MD5 carried on the GPU, flac_md5.hip) against FLAC delivery
without it in the same way; with `--flac-only` only the engine with the option renders (the run for elemhip_flac_md5's own time in a
kernel trace). `--md5-baseline` times FLAC16 delivery alone, no option touched, round by round: run in this tree and in a checkout of
the parent commit, alternately, it shows whether the option's being off costs anything."""
import sys, time; sys.path.insert(0, '.')
from elementary_amd import graphs
from elementary_amd.runtime import Runtime

flac_only = "--flac-only" in sys.argv
lpc_order = int(sys.argv[sys.argv.index("--lpc-order") + 1]) if "--lpc-order" in sys.argv else 0
md5, md5_baseline = "--md5" in sys.argv, "--md5-baseline" in sys.argv
ROUNDS = 5


def engine(roots, n_out, batch, flac_frame, order, key="flac_lpc_order"):
    rt = Runtime(48000.0, 512, device=0); rt.set_option("specialize", 2); rt.set_option("batch_blocks", batch); rt.set_option("flac_frame", flac_frame)
    if order:
        rt.set_option(key, order)
    assert rt.render(*roots)["result"] == 0
    rt.process_blocks_host(None, n_out, 64 * 512)                # root fades settle: launch sets from here on
    return rt


def lpc_workload(name, roots, S, G, batch, sets, flac_frame):
    """Two engines that differ in one option (flac_lpc_order = P, or with --md5 flac_md5 = 1) against its being off."""
    n_out, frames = S * G, sets * batch * 512
    key, tag, lpc_order = ("flac_md5", "md5_", 1) if md5 else ("flac_lpc_order", "lpc", globals()["lpc_order"])
    legs = {f"{tag}{lpc_order}": engine(roots, n_out, batch, flac_frame, lpc_order, key)}
    if not flac_only:
        legs[f"{tag}0"] = engine(roots, n_out, batch, flac_frame, 0)

    def flac(rt):
        streams, _ = rt.process_blocks_flac(None, S, G, frames, 16)
        return sum(len(b) for b in streams)

    for rt in legs.values():
        flac(rt)                                                 # warm-up (and the buffers' allocation)
    if flac_only:
        flac(legs[f"{tag}{lpc_order}"])
        return
    t = {k: [] for k in legs}
    nbytes = {k: 0 for k in legs}
    for _ in range(ROUNDS):
        for label in (f"{tag}0", f"{tag}{lpc_order}"):
            t0 = time.perf_counter(); nbytes[label] += flac(legs[label]); t[label].append(time.perf_counter() - t0)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    for label in (f"{tag}0", f"{tag}{lpc_order}"):
        print(f"{name} flac_frame {flac_frame} {label:6s} ms/set {' '.join(f'{1e3 * x / sets:8.2f}' for x in t[label])}   median {1e3 * med[label] / sets:8.2f}"
              f"   frame bytes over {ROUNDS} calls {nbytes[label]}", flush=True)
    a, b = f"{tag}{lpc_order}", f"{tag}0"
    print(f"{name} flac_frame {flac_frame} median {a} / {b} {med[a] / med[b]:5.3f}   bytes {a} / {b} {nbytes[a] / nbytes[b]:5.3f}"
          f"   {a} / s16 {nbytes[a] / (2.0 * n_out * frames * ROUNDS):5.3f}", flush=True)


def workload(name, roots, S, G, batch, sets, flac_frame):
    if lpc_order or md5:
        return lpc_workload(name, roots, S, G, batch, sets, flac_frame)
    n_out, frames = S * G, sets * batch * 512
    rt = engine(roots, n_out, batch, flac_frame, 0)

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
    if md5_baseline:
        t = []
        for _ in range(ROUNDS):
            t0 = time.perf_counter(); flac(); t.append(time.perf_counter() - t0)
        print(f"{name} flac_frame {flac_frame} flac16 ms/set {' '.join(f'{1e3 * x / sets:8.2f}' for x in t)}   median {1e3 * sorted(t)[len(t) // 2] / sets:8.2f}", flush=True)
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
