"""The yardstick of PCM delivery: a numpy restatement of the hash, the TPDF dither keyed on absolute time and the quantiser,
written from the specification and NOT from elementary_amd/csrc/pcm_pack.h. ``pack`` / ``stats`` apply it to planar floats the
way the engine lays streams out: sample (frame, g) of stream s is output channel s * G + g."""
import numpy as np


def h32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16); x = (x * np.uint32(0x7feb352d)).astype(np.uint32)
    x ^= x >> np.uint32(15); x = (x * np.uint32(0x846ca68b)).astype(np.uint32)
    x ^= x >> np.uint32(16); return x
def dither(seed, c, t):                                   # t: int64 array of absolute frame times
    lo = (t & 0xffffffff).astype(np.uint32); hi = ((t >> 32) & 0xffffffff).astype(np.uint32)
    k0 = h32(np.array([(seed ^ (c * 0x9E3779B9)) & 0xffffffff], dtype=np.uint32))
    k = h32(lo ^ h32(hi ^ k0)); r1 = h32(k); r2 = h32(k ^ np.uint32(0x85EBCA6B))
    return ((r1 >> np.uint32(8)).astype(np.int64) - (r2 >> np.uint32(8)).astype(np.int64)).astype(np.float32) * np.float32(2.0**-24)
def quant(x, bits, d):                                    # x, d float32 -> int32
    S = np.float32(2.0**(bits-1)); x = np.where(np.isfinite(x), x, np.float32(0)).astype(np.float32)
    with np.errstate(over='ignore'): v = (x * S).astype(np.float32) + d
    return np.clip(np.rint(v), -S, S - 1).astype(np.int32)


# x -> (S16, S24) with dither off
EDGE_TABLE = [(0.0, 0, 0), (1.0, 32767, 8388607), (-1.0, -32768, -8388608), (0.5 / 32768, 0, 128), (1.5 / 32768, 2, 384),
              (-0.5 / 32768, 0, -128), (2.5 / 32768, 2, 640), (3e38, 32767, 8388607), (-3e38, -32768, -8388608),
              (float("nan"), 0, 0), (float("inf"), 0, 0), (0.99999, 32767, 8388524)]


def pack(planar, G, fmt, seed=None, t0=0):
    """planar float32 [nOut, frames] -> list of nOut / G streams shaped like Runtime.process_blocks_pcm returns them."""
    planar = np.asarray(planar, dtype=np.float32)
    n_out, frames = planar.shape
    t = np.int64(t0) + np.arange(frames, dtype=np.int64)
    out = []
    for s in range(n_out // G):
        rows = planar[s * G:(s + 1) * G]
        if fmt == "f32":
            out.append(np.ascontiguousarray(rows.T))
            continue
        bits = 16 if fmt == "s16" else 24
        q = np.stack([quant(rows[g], bits, dither(seed, s * G + g, t) if seed is not None else np.zeros(frames, np.float32))
                      for g in range(G)], axis=1)
        if fmt == "s16":
            out.append(q.astype(np.int16))
        else:
            u = q.astype(np.uint32)
            out.append(np.stack([(u >> np.uint32(8 * k)) & np.uint32(0xFF) for k in range(3)], axis=2).astype(np.uint8))
    return out


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def stats(planar):
    planar = np.asarray(planar, dtype=np.float32)
    fin = np.isfinite(planar)
    mag = np.where(fin, np.abs(planar), np.float32(0)).astype(np.float32)
    return {"peak": mag.max(axis=1) if planar.shape[1] else np.zeros(planar.shape[0], np.float32),
            "over": (fin & (mag > np.float32(1.0))).sum(axis=1).astype(np.uint64), "nonfinite": (~fin).sum(axis=1).astype(np.uint64)}
