"""Noise-shaped s16 delivery of an offline render, timed: elemhip_process_blocks_pcm (s16, dithered) with the `fweighted9` filter set
(Runtime.noise_shape; noise_shape.hip) against the same delivery without it, on the C4 workload (128 instances, mono streams, launch
sets of 1024 blocks) and on a 2-channel render (C2, one stereo stream, sets of 256). Two engines render the same programme; rounds
alternate the two legs after a warm-up call of each (a host clock around calls that end with both streams synchronised); the medians
are compared, and the difference is put per frame of one channel.

`--shaped-only` renders a few shaped sets and nothing else: the run for a kernel trace of its own (rocprofv3 --kernel-trace --stats),
where elemhip_noise_shape shows its own time per set."""
import sys, time; sys.path.insert(0, '.')
from elementary_amd import graphs
from elementary_amd.noise_shape import PRESETS
from elementary_amd.runtime import Runtime

shaped_only = "--shaped-only" in sys.argv
ROUNDS = 5


def engine(roots, n_out, batch, shape):
    rt = Runtime(48000.0, 512, device=0); rt.set_option("specialize", 2); rt.set_option("batch_blocks", batch)
    if shape:
        rt.noise_shape(PRESETS["fweighted9"])
    assert rt.render(*roots)["result"] == 0
    rt.process_blocks_host(None, n_out, 64 * 512)                # root fades settle: launch sets from here on
    return rt


def workload(name, roots, S, G, batch, sets):
    n_out, frames = S * G, sets * batch * 512
    legs = {"shaped": engine(roots, n_out, batch, True)}
    if not shaped_only:
        legs["plain"] = engine(roots, n_out, batch, False)

    def pcm(rt):
        rt.process_blocks_pcm(None, S, G, frames, "s16", dither_seed=1)

    for rt in legs.values():
        pcm(rt)                                                  # warm-up (and the buffers' allocation)
    if shaped_only:
        pcm(legs["shaped"])
        return
    t = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for label in ("plain", "shaped"):
            t0 = time.perf_counter(); pcm(legs[label]); t[label].append(time.perf_counter() - t0)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    for label in ("plain", "shaped"):
        print(f"{name} s16 {label:6s} ms/set {' '.join(f'{1e3 * x / sets:8.2f}' for x in t[label])}   median {1e3 * med[label] / sets:8.2f}", flush=True)
    extra = (med["shaped"] - med["plain"]) / sets
    got = legs["shaped"].noise_shape_read()
    print(f"{name} s16 median shaped / plain {med['shaped'] / med['plain']:5.3f}   + {1e3 * extra:7.2f} ms/set = {1e9 * extra / (batch * 512):7.1f} ns per frame"
          f" ({n_out} channels side by side: {1e9 * extra / (batch * 512 * n_out):6.2f} ns per frame and channel)   saturated {int(got['saturated'].sum())}", flush=True)


workload("C4", [graphs.c4_instance(k) for k in range(128)], 128, 1, 1024, 2)
workload("C2", graphs.c2_graph(), 1, 2, 256, 8)
