"""Inputs at another sample rate, timed: the C4 workload (128 instances, mono roots, launch sets of 1024 blocks of 512 frames) with a
stereo input mixed under every root, in one process, specialize 2, three repetitions of every leg, each after a warm-up call of the
same size. The engine runs at 176400 Hz and delivers planar floats.
  off      the input as s16 at the ENGINE's rate, option "input_rate" off: what a caller who upsamples on the CPU hands over
           (the unpack kernel in front of every set, four times the bytes across the host link)
  on       the input as s16 at 44100 with option "input_rate" 44100: a quarter of the bytes cross, resample_in.hip converts them in
           front of every set
Prints the time per launch set of both and their ratio, the bytes the converter's kernel moves per set (the stretch read once, the
set's input half written once; the table and the overlap between tiles stay in L2) and the time they take at the 8 TB/s the
project's rooflines use. (on - off) is NOT the kernel's own time: it runs on the render's stream in front of the set's first level
while the previous set's copy-out goes on. The kernel's own time per set is delegated to a kernel trace of a run of its own:
`--kernel-only` renders a few converted sets and nothing else (rocprofv3 --kernel-trace --stats -- python
tools/input_resample_probe.py --kernel-only: the elemhip_resample_in rows, mean duration per dispatch = per set).
`--out FILE` also writes what was printed to FILE."""
import sys, time; sys.path.insert(0, '.')
import numpy as np
from elementary_amd import el, graphs
from elementary_amd.runtime import Runtime

kernel_only = "--kernel-only" in sys.argv
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
REPS, N_OUT, N_IN, BATCH, SETS, BS, SR, FIN = 3, 128, 2, 1024, 3, 512, 176400, 44100
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def engine(fin):
    rt = Runtime(float(SR), BS, device=0); rt.set_option("specialize", 2); rt.set_option("batch_blocks", BATCH)
    roots = [el.add(graphs.c4_instance(k), el.mul(0.1, el.in_({"channel": k % N_IN}))) for k in range(N_OUT)]
    assert rt.render(*roots)["result"] == 0
    rt.process_blocks_host(np.zeros((N_IN, 64 * BS), dtype=np.float32), N_OUT, 64 * BS)      # root fades settle: launch sets from here on
    if fin:
        rt.set_option("input_rate", fin)
    return rt


def timed(fn):
    fn()
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter(); fn(); out.append(time.perf_counter() - t0)
    return out


frames = SETS * BATCH * BS
rng = np.random.default_rng(7)


def stream(n):
    return [rng.integers(-20000, 20000, size=(n, N_IN), dtype=np.int16)]


if kernel_only:
    rt = engine(FIN)
    for _ in range(2):
        rt.process_blocks_pcm_io(stream(rt.input_resample_frames(frames)), "s16", num_outputs=N_OUT, num_frames=frames)
    print(rt.input_resample_read())
    sys.exit(0)


def leg(name, fin):
    rt = engine(fin)
    x = stream(frames // 4 + 8 if fin else frames)
    ts = timed(lambda: rt.process_blocks_pcm_io([x[0][:rt.input_resample_frames(frames)]], "s16", num_outputs=N_OUT, num_frames=frames))
    med = sorted(ts)[1] / SETS
    say(f"{name:<52s} ms per call {' '.join(f'{1e3 * t:8.2f}' for t in ts)}   median per set of {BATCH} blocks {1e3 * med:7.3f} ms")
    if fin:
        got = rt.input_resample_read()
        moved = N_IN * BATCH * BS * (2.0 * got["down"] / got["up"] + 4.0)
        say(f"   {got['up']}/{got['down']}, {got['taps']} taps; the kernel moves {moved / 1e6:.2f} MB per set: {1e3 * moved / 8e12:.4f} ms at 8 TB/s; "
            f"{got['taps'] * N_IN * BATCH * BS / 1e9:.3f} G fused multiply-adds per set; {N_IN * BATCH * BS * 2 * got['down'] / got['up'] / 1e6:.2f} MB "
            f"cross the host link per set instead of {N_IN * BATCH * BS * 2 / 1e6:.2f}")
    return med


off = leg("C4 + s16 stereo input at 176400, input_rate off", 0)
on = leg("C4 + s16 stereo input at 44100, input_rate 44100", FIN)
say(f"set time on / off {on / off:5.3f}   (on - off) {1e3 * (on - off):+8.3f} ms per set")
say("the kernel's own time per set: see the kernel trace of `--kernel-only` (not timed here)")
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
