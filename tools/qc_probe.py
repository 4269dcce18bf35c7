"""The inspector, timed: elemhip_process_blocks_pcm (s16, two channels per stream, no float crosses the host link) on a C4 set (128
instances, mono roots, launch sets of 1024 blocks of 512) and on a C2 set (the 256-voice graph, two channels) with the inspector off and
on, in one process, specialize 2. Two variants: the defaults (no overview, no pairs), and a bucket of 1000 frames with one pair per two
channels. Every leg is timed in alternating rounds (off, on, on+, off, ...) after a warm-up call each, and the medians are compared.
(on - off) is NOT the kernels' own time: they run on the render's stream while the previous set's copy-out and delivery go on. With
--kernels only the "on+" legs run, two calls each, for a kernel trace taken from outside (rocprofv3 --kernel-trace --stats -- python
tools/qc_probe.py --kernels): the kernels' own durations. Writes profiles/r07/qc.txt when run with --write."""
import os, sys, time; sys.path.insert(0, '.')
from elementary_amd import graphs
from elementary_amd.runtime import Runtime

ROUNDS, BATCH, BS = 5, 1024, 512
VARIANTS = {"off": None, "on (defaults)": {}, "on+ (bucket 1000, pairs)": {"bucket": 1000, "pairs": True}}
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def engine(roots, sr, n_out, variant):
    rt = Runtime(sr, BS, device=0); rt.set_option("specialize", 2); rt.set_option("batch_blocks", BATCH)
    assert rt.render(*roots)["result"] == 0
    rt.process_blocks_host(None, n_out, 64 * BS)                 # root fades settle: launch sets from here on
    if variant is not None:
        spec = dict(variant)
        if spec.pop("pairs", False):
            spec["pairs"] = [(c, c + 1) for c in range(0, n_out - 1, 2)]
        rt.qc(spec)
    return rt


def probe(name, roots, sr, n_out, sets, only=None):
    frames = sets * BATCH * BS
    rts = {k: engine(roots, sr, n_out, v) for k, v in VARIANTS.items() if only is None or k == only}
    call = {k: (lambda rt=rt: rt.process_blocks_pcm(None, n_out // 2, 2, frames, "s16")) for k, rt in rts.items()}
    ts = {k: [] for k in rts}
    for k in rts:
        call[k]()                                                # warm-up: buffers sized, kernels loaded
        if VARIANTS[k] is not None:
            rts[k].qc_read()
    for _ in range(ROUNDS if only is None else 2):
        for k in rts:
            t0 = time.perf_counter(); call[k](); ts[k].append(time.perf_counter() - t0)
            if VARIANTS[k] is not None:
                rts[k].qc_read()                                 # (drained outside the timed stretch)
    med = {k: sorted(v)[len(v) // 2] / sets for k, v in ts.items()}
    for k in rts:
        extra = ""
        if VARIANTS[k] is not None and "off" in med:
            extra = f"   on / off {med[k] / med['off']:5.3f}   (on - off) {1e3 * (med[k] - med['off']):7.3f} ms per {BATCH} blocks"
        spread = 1e3 * (max(ts[k]) - min(ts[k])) / sets
        say(f"{name} pcm s16 G=2, {k:26s} ms per call {' '.join(f'{1e3 * t:8.2f}' for t in ts[k])}   median per {BATCH} blocks {1e3 * med[k]:7.3f} ms"
            f"   spread {spread:6.3f} ms{extra}")
    floats_mb = n_out * BATCH * BS * 4 / 1e6
    say(f"{name}: the inspector reads {floats_mb:.1f} MB of floats per {BATCH} blocks once; s16 delivery moves {floats_mb / 2:.1f} MB to the host")


only = "on+ (bucket 1000, pairs)" if "--kernels" in sys.argv else None
say(f"qc_probe: medians of {ROUNDS if only is None else 2} alternating rounds, batch_blocks {BATCH}, block {BS}")
probe("C4", [graphs.c4_instance(k) for k in range(128)], graphs.C4_SAMPLE_RATE, 128, 2, only)
probe("C2", graphs.c2_graph(), graphs.C2_SAMPLE_RATE, 2, 2, only)
if "--write" in sys.argv:
    out = os.path.join("profiles", "r07", "qc.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out)
