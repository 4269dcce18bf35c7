"""Input of an offline render, timed: elemhip_process_blocks_host (planar float32 input, the path the parent commit has) against
elemhip_process_blocks_pcm_io with s16 / s24 / f32 input (interleaved, unpacked on the GPU), on two graphs of 8 input channels: a
gain per channel, and the C3 convolution reverb at a reduced impulse-response length. One process, the same frames in every leg
(the float leg is handed the decoded streams, so the outputs are bit-identical and are compared once); 5 warm-up calls, then 20 timed
rounds in which the legs ALTERNATE, so drift of the shared host falls on all of them alike; a host clock around calls that end in a
device synchronise. Reported per leg: median, min and max in ms, and the median as a ratio to the float leg. `--unpack-only` renders
a few PCM-fed calls and nothing else, for a kernel trace of its own; `--out FILE` also writes the report there."""
import sys, time; sys.path.insert(0, '.')
import numpy as np
from elementary_amd import el, graphs
from elementary_amd.runtime import Runtime

unpack_only = "--unpack-only" in sys.argv
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
WARM, ROUNDS, CH, BS = 5, 20, 8, 512
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def streams_of(fmt, frames, seed):
    """One stream of CH channels at a quarter of full scale."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.25, 0.25, size=(frames, CH))
    if fmt == "s16":
        return [np.rint(x * 32767).astype(np.int16)]
    if fmt == "s24":
        v = np.rint(x * 8388607).astype(np.int64) % (1 << 24)
        return [np.stack([v % 256, (v // 256) % 256, v // 65536], axis=-1).astype(np.uint8)]
    return [x.astype(np.float32)]


def decoded(streams, fmt):
    a = streams[0]
    if fmt == "s16":
        return np.ascontiguousarray((a.astype(np.float64) / 32768.0).astype(np.float32).T)
    if fmt == "s24":
        b = a.astype(np.int64)
        v = b[..., 0] + 256 * b[..., 1] + 65536 * b[..., 2]
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        return np.ascontiguousarray((v.astype(np.float64) / 8388608.0).astype(np.float32).T)
    return np.ascontiguousarray(a.T)


def workload(name, roots, batch, sets, resources=None):
    frames = sets * batch * BS
    legs = {}
    for fmt in ("s16", "s24", "f32"):
        legs[fmt] = streams_of(fmt, frames, 5)
    x = decoded(legs["s16"], "s16")                              # the float leg's input: what the s16 leg's kernel decodes to

    def engine():
        rt = Runtime(48000.0, BS, device=0); rt.set_option("specialize", 2); rt.set_option("batch_blocks", batch)
        for k, v in (resources or {}).items():
            rt.add_shared_resource(k, v)
        assert rt.render(*roots)["result"] == 0
        rt.process_blocks_host(None, CH, 64 * BS)               # root fades settle: launch sets from here on
        return rt

    if unpack_only:
        rt = engine()
        for fmt in ("s16", "s24", "f32"):
            rt.process_blocks_pcm_io(legs[fmt], fmt, CH); rt.process_blocks_pcm_io(legs[fmt], fmt, CH)
        return
    # one engine per leg, so that every leg renders the same history; the outputs of the float and the s16 leg are the same bits
    rts = {k: engine() for k in ("float", "s16", "s24", "f32")}
    calls = {"float": lambda: rts["float"].process_blocks_host(x, CH, frames)}         # (every leg allocates its output, as the PCM legs do)
    for fmt in ("s16", "s24", "f32"):
        calls[fmt] = lambda fmt=fmt: rts[fmt].process_blocks_pcm_io(legs[fmt], fmt, CH)
    a, b = calls["float"](), calls["s16"]()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "the s16 leg and the float leg differ"
    for _ in range(WARM - 1):
        for fn in calls.values():
            fn()
    ts = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, fn in calls.items():
            t0 = time.perf_counter(); fn(); ts[k].append(time.perf_counter() - t0)
    base = float(np.median(ts["float"]))
    in_bytes = {"float": 4, "s16": 2, "s24": 3, "f32": 4}
    say(f"{name}: {CH} inputs -> {CH} outputs, {frames} frames per call ({sets} sets of {batch} blocks), {WARM} warm-up calls, {ROUNDS} timed rounds, legs alternating")
    for k, v in ts.items():
        med = float(np.median(v))
        say(f"  {k + ' input':12s} {in_bytes[k] * CH * frames / 1e6:8.1f} MB in   median {1e3 * med:8.3f} ms   min {1e3 * min(v):8.3f}   max {1e3 * max(v):8.3f}"
            f"   median / float {med / base:5.3f}")
    s16 = float(np.median(ts["s16"]))
    say(f"  s16 input is {'NOT slower' if s16 <= base else 'SLOWER'} than float input by the medians ({1e3 * s16:.3f} ms against {1e3 * base:.3f} ms)")


def gains():
    return [el.mul(0.5 + 0.1 * c, el.in_({"channel": c})) for c in range(CH)]


workload("gain per channel", gains(), 256, 8)
IR = 16384                                                        # (the C3 response cut from 96000 taps)
workload(f"C3 reverb, {IR}-tap responses", graphs.c3_graph(CH), 256, 4, {f"ir{c}": graphs.c3_impulse_response(c, IR)[None, :] for c in range(CH)})
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
