"""The spectrum analyser, timed: elemhip_process_blocks_pcm (s16, two channels per stream, no float crosses the host link) on a C4 set
(128 instances, mono roots, launch sets of 1024 blocks of 512) and on a C2 set (the 256-voice graph, two channels) with the analyser off
and on, in one process, specialize 2. Two variants: 40 mel bands at S = 1024, H = 256, and power at S = 4096, H = 1024. Every leg is
timed in alternating rounds (off, mel, power, off, ...) after a warm-up call each, and the medians are compared. Prints the time per
launch set of every leg, on / off, the frames and bytes the analyser delivers per set and the set size the pinned halves allow (256 MB
a half: C4 power at S = 4096 does not fit a set of 1024 blocks, so its sets are smaller). (on - off) is NOT the kernels' own time:
they run on the render's stream while the previous set's copy-out and delivery go on. Writes profiles/r07/spectrum.txt when run with
--write."""
import os, sys, time; sys.path.insert(0, '.')
from elementary_amd import graphs
from elementary_amd import spectrum as sp
from elementary_amd.runtime import Runtime

ROUNDS, BATCH, BS = 5, 1024, 512
VARIANTS = {"off": None, "mel40 S=1024 H=256": (1024, 256, 40), "power S=4096 H=1024": (4096, 1024, None)}
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def engine(roots, sr, n_out, variant):
    rt = Runtime(sr, BS, device=0); rt.set_option("specialize", 2); rt.set_option("batch_blocks", BATCH)
    assert rt.render(*roots)["result"] == 0
    rt.process_blocks_host(None, n_out, 64 * BS)                 # root fades settle: launch sets from here on
    if variant:
        size, hop, mel = variant
        rt.spectrum(size, hop, "hann", sp.mel_bands(sr, size, mel) if mel else None)
    return rt


def probe(name, roots, sr, n_out, sets):
    frames = sets * BATCH * BS
    rts = {k: engine(roots, sr, n_out, v) for k, v in VARIANTS.items()}
    call = {k: (lambda rt=rt: rt.process_blocks_pcm(None, n_out // 2, 2, frames, "s16")) for k, rt in rts.items()}
    ts = {k: [] for k in rts}
    for k in rts:
        call[k]()                                                # warm-up: buffers sized, kernels loaded
        if VARIANTS[k]:
            rts[k].spectrum_read(sums=False)
    for _ in range(ROUNDS):
        for k in rts:
            t0 = time.perf_counter(); call[k](); ts[k].append(time.perf_counter() - t0)
            if VARIANTS[k]:
                rts[k].spectrum_read(sums=False)                 # (drained outside the timed stretch)
    med = {k: sorted(v)[len(v) // 2] / sets for k, v in ts.items()}
    for k in rts:
        extra = ""
        if VARIANTS[k]:
            size, hop, mel = VARIANTS[k]
            cols = mel or size // 2 + 1
            per_set = BATCH * BS // hop
            mb = n_out * per_set * cols * 4 / 1e6
            extra = (f"   on / off {med[k] / med['off']:5.3f}   (on - off) {1e3 * (med[k] - med['off']):7.3f} ms per {BATCH} blocks   "
                     f"{per_set} frames x {cols} columns x {n_out} channels = {mb:.1f} MB per {BATCH} blocks"
                     f"{' (over a 256 MB half: smaller sets)' if mb > 256 else ''}")
        say(f"{name} pcm s16 G=2, {k:22s} ms per call {' '.join(f'{1e3 * t:8.2f}' for t in ts[k])}   median per {BATCH} blocks {1e3 * med[k]:7.3f} ms{extra}")
    floats_mb = n_out * BATCH * BS * 4 / 1e6
    say(f"{name}: planar float delivery would move {floats_mb:.1f} MB per {BATCH} blocks, s16 {floats_mb / 2:.1f} MB")


say(f"spectrum_probe: medians of {ROUNDS} alternating rounds, batch_blocks {BATCH}, block {BS}")
probe("C4", [graphs.c4_instance(k) for k in range(128)], graphs.C4_SAMPLE_RATE, 128, 2)
probe("C2", graphs.c2_graph(), graphs.C2_SAMPLE_RATE, 2, 2)
if "--write" in sys.argv:
    out = os.path.join("profiles", "r07", "spectrum.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out)
