"""Loads the same material as a shared resource three ways and prints, for each, the load time, the bytes that cross the host link and
the time from the start of the load to the first rendered block of a graph that plays every channel of it:

  floats   decoded on the host (numpy) and handed to add_shared_resource — uploaded as float32 on first use
  s16      the file's int16 samples through add_shared_resource_pcm, decoded on the GPU
  flac16   the FLAC frames of the same samples through add_shared_resource_pcm, decoded on the GPU

    python tools/resource_load_probe.py [--channels 8] [--frames 96000] [--file-rate 0] [--repeat 5]

--file-rate other than 0 adds the rate conversion to the two GPU ways (the float way has none: its floats play at the wrong pitch).
Times are wall-clock medians over --repeat fresh engines, after one warm-up engine per way."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def material(frames, channels, seed=3):
    """A decaying noise burst per channel, what an impulse response looks like to an entropy coder."""
    rng = np.random.default_rng(seed)
    env = np.exp(-np.arange(frames) / (frames / 6.0))[:, None]
    return np.rint(rng.normal(0.0, 0.2, size=(frames, channels)).clip(-1, 1) * env * 32767).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--frames", type=int, default=96000)
    ap.add_argument("--file-rate", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--block", type=int, default=512)
    ap.add_argument("--rate", type=int, default=48000)
    args = ap.parse_args()

    import torch  # noqa: F401   (before libelemhip.so: both bind the HIP runtime torch ships)
    from elementary_amd import el
    from elementary_amd.runtime import FlacChunk, Runtime, flac_encode, flac_index

    G, N = args.channels, args.frames
    pcm = material(N, G)
    t = time.perf_counter()
    data, _ = flac_encode(pcm.T.astype(np.int32), 16, 4096, args.rate)
    encode_s = time.perf_counter() - t
    off, first = flac_index(data, G, 16, 4096)
    chunk = FlacChunk(np.frombuffer(data, dtype=np.uint8), off, first, G, 16, N, 0, N)
    rate = args.file_rate or None

    def floats(rt):
        x = np.ascontiguousarray((pcm.astype(np.float32) / np.float32(32768.0)).T)      # the host decode is part of this way
        assert rt.add_shared_resource("/p/x", x)
        return 4 * N * G

    def s16(rt):
        assert rt.add_shared_resource_pcm("/p/x", pcm, "s16", G, sample_rate=rate)
        return 2 * N * G

    def flac16(rt):
        assert rt.add_shared_resource_pcm("/p/x", chunk, sample_rate=rate)
        return len(data) + 32 * (len(off) - 1) + 32

    print(f"material: {G} channels x {N} frames of s16 ({2 * N * G} bytes; FLAC16 {len(data)} bytes, encoded on the host in {encode_s:.3f} s); "
          f"engine {args.rate} Hz, block {args.block}, file rate {args.file_rate or args.rate} Hz")
    print(f"{'way':8s} {'load ms':>10s} {'link bytes':>12s} {'first block ms':>15s}")
    for name, load in (("floats", floats), ("s16", s16), ("flac16", flac16)):
        loads, firsts, link = [], [], 0
        for rep in range(args.repeat + 1):
            rt = Runtime(args.rate, args.block, device=0)
            t0 = time.perf_counter()
            link = load(rt)
            t1 = time.perf_counter()
            roots = el.mc.sample({"path": "/p/x", "channels": G, "mode": "loop"}, 1.0)
            assert rt.render(*roots)["result"] == 0
            rt.process(None, G, args.block)
            t2 = time.perf_counter()
            if rep:                                  # (the first engine of a way warms the library up)
                loads.append((t1 - t0) * 1e3)
                firsts.append((t2 - t0) * 1e3)
            rt.close()
        print(f"{name:8s} {statistics.median(loads):10.3f} {link:12d} {statistics.median(firsts):15.3f}")


if __name__ == "__main__":
    main()
