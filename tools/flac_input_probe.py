"""FLAC input of an offline render, timed: a launch-set call fed with FLAC16 (elemhip_process_blocks_pcm_io, input format 4: the frames
cross the host link compressed and are decoded on the GPU, elementary_amd/csrc/flac_decode.hip) against the same call fed with the
s16 streams of the same samples (the parent commit's path), on two graphs: a gain per channel over 32 mono streams — the host-input
limit; C4's 128 voices take no host inputs — and the same over one stereo stream. One process, one engine per leg with the same
history, the outputs compared once (they are the same bits); 5 warm-up calls, then 20 timed rounds in which the legs ALTERNATE; a
host clock around calls that end in a device synchronise. Reported per leg: median, min and max in ms, the median as a ratio to the
s16 leg, and the bytes that cross the host link. What is timed is a whole call of four launch sets of 256 blocks, not one set: the
sets of a call overlap (copy, decode and render of neighbouring sets run side by side), so a per-set figure is the call's divided by
four. The three kernels' own times are NOT printed here: they come from a kernel trace of `--decode-only`, which renders a few
FLAC-fed calls and nothing else. `--out FILE` also writes the report there.
`--md5`: the FLAC-fed call alone, with engine option flac_in_md5 = 1 (the decoded samples' STREAMINFO MD5 on the GPU,
elementary_amd/csrc/flac_in_md5.hip) against the same without — two engines, the slots reset in front of every call so that every call
hashes the whole programme, the legs alternating, medians; the digests are checked against hashlib once. The chain is serial inside a
stream: the delivery kernel's 0.85 us per 64-byte block (profiles/r07/flac_md5.txt) is the prediction to compare with."""
import sys, time; sys.path.insert(0, '.')
import numpy as np
from elementary_amd import el
from elementary_amd.runtime import FlacChunk, Runtime, flac_encode, flac_index

decode_only = "--decode-only" in sys.argv
md5_legs = "--md5" in sys.argv
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
WARM, ROUNDS, BS, FF = 5, 20, 512, 4096
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def programme(frames, channels, seed):
    """Music-like codes at a quarter of full scale: a few partials and a little noise, so that the encoder's FIXED predictors bite."""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)
    x = sum(a * np.sin(t * f + p) for a, f, p in zip((0.12, 0.07, 0.04), (0.011, 0.047, 0.13), rng.uniform(0, 6, 3)))
    return np.stack([np.rint((x + 0.002 * rng.standard_normal(frames)) * 32767 * (0.8 + 0.2 * c / max(channels, 1))).astype(np.int32) for c in range(channels)])


def workload(name, streams, G, batch, sets):
    frames = sets * batch * BS
    n_in = streams * G
    codes = [programme(frames, G, 11 + s) for s in range(streams)]
    pcm = [np.ascontiguousarray(c.T.astype(np.int16)) for c in codes]
    chunks = []
    for c in codes:
        data, _ = flac_encode(c, bits=16, flac_frame=FF, sample_rate=48000)
        off, first = flac_index(data, G, 16, FF)
        chunks.append(FlacChunk(np.frombuffer(data, dtype=np.uint8), off, first, G, 16, frames, 0, frames))

    def engine(md5=0):
        rt = Runtime(48000.0, BS, device=0); rt.set_option("specialize", 2); rt.set_option("batch_blocks", batch)
        if md5:
            rt.set_option("flac_in_md5", 1)
        assert rt.render(*[el.mul(0.5 + 0.01 * c, el.in_({"channel": c})) for c in range(n_in)])["result"] == 0
        rt.process_blocks_host(None, n_in, 64 * BS)             # root fades settle: launch sets from here on
        return rt

    if decode_only:
        rt = engine()
        for _ in range(3):
            rt.process_blocks_pcm_io(chunks, "flac", n_in, frames)
        return
    if md5_legs:
        import hashlib
        rts = {"flac_in_md5 0": engine(), "flac_in_md5 1": engine(1)}

        def call(k):
            rts[k].flac_in_md5_reset()
            return rts[k].process_blocks_pcm_io(chunks, "flac", n_in, frames)
        a, b = call("flac_in_md5 0"), call("flac_in_md5 1")
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "the option changed a rendered sample"
        got = rts["flac_in_md5 1"].flac_in_md5()
        assert got["state"] == [2] * streams and got["md5"] == [hashlib.md5(p.tobytes()).digest() for p in pcm], "a digest is not hashlib's"
        for _ in range(WARM - 1):
            for k in rts:
                call(k)
        ts = {k: [] for k in rts}
        for _ in range(ROUNDS):
            for k in rts:
                t0 = time.perf_counter(); call(k); ts[k].append(time.perf_counter() - t0)
        base = float(np.median(ts["flac_in_md5 0"]))
        blocks = frames * G * 2 // 64
        say(f"{name}: {streams} streams x {G} channels, {frames} frames per call ({sets} sets of {batch} blocks), FLAC frames of {FF}, {WARM} warm-up calls, "
            f"{ROUNDS} timed rounds, legs alternating; {blocks} MD5 blocks per stream and call")
        for k, v in ts.items():
            med = float(np.median(v))
            say(f"  {k:14s} median {1e3 * med:8.3f} ms   min {1e3 * min(v):8.3f}   max {1e3 * max(v):8.3f}   median / off {med / base:5.3f}"
                + (f"   (+{1e3 * (med - base):.3f} ms = {1e6 * (med - base) / blocks:.3f} us per 64-byte block of one stream)" if k.endswith("1") else ""))
        return
    rts = {"s16": engine(), "flac16": engine()}
    calls = {"s16": lambda: rts["s16"].process_blocks_pcm_io(pcm, "s16", n_in, frames),
             "flac16": lambda: rts["flac16"].process_blocks_pcm_io(chunks, "flac", n_in, frames)}
    a, b = calls["s16"](), calls["flac16"]()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "the FLAC leg and the s16 leg differ"
    for _ in range(WARM - 1):
        for fn in calls.values():
            fn()
    ts = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, fn in calls.items():
            t0 = time.perf_counter(); fn(); ts[k].append(time.perf_counter() - t0)
    base = float(np.median(ts["s16"]))
    crossing = {"s16": sum(p.nbytes for p in pcm), "flac16": sum(c.data.nbytes for c in chunks)}
    say(f"{name}: {streams} streams x {G} channels, {frames} frames per call ({sets} sets of {batch} blocks), FLAC frames of {FF}, {WARM} warm-up calls, "
        f"{ROUNDS} timed rounds, legs alternating")
    for k, v in ts.items():
        med = float(np.median(v))
        say(f"  {k + ' input':13s} {crossing[k] / 1e6:8.2f} MB in ({crossing[k] / crossing['s16']:5.3f} of s16)   median {1e3 * med:8.3f} ms   min {1e3 * min(v):8.3f}"
            f"   max {1e3 * max(v):8.3f}   median / s16 {med / base:5.3f}")


workload("32 mono streams, gain per channel", 32, 1, 256, 4)
workload("one stereo stream, gain per channel", 1, 2, 256, 4)
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
