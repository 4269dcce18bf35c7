"""The yardstick of PCM input: a numpy restatement of the decode written from the specification and NOT from
elementary_amd/csrc/pcm_unpack.h. An s16 code is worth ``code * 2**-15``, an s24 code (three little-endian bytes, two's complement)
``code * 2**-23``, an f32 sample its own bits; both products are exact in float32. ``decode`` turns streams in the engine's layout —
sample (frame, g) of stream s is input channel s * G + g — into planar float32 rows."""
import numpy as np


def s24_codes(stream):
    """uint8 [..., 3] -> int32 codes."""
    b = np.asarray(stream, dtype=np.uint8).astype(np.int64)
    v = b[..., 0] + 256 * b[..., 1] + 65536 * b[..., 2]
    return np.where(v >= 1 << 23, v - (1 << 24), v).astype(np.int32)


def s24_bytes(codes):
    """int32 codes -> uint8 [..., 3]."""
    v = np.asarray(codes, dtype=np.int64) % (1 << 24)
    return np.stack([v % 256, (v // 256) % 256, v // 65536], axis=-1).astype(np.uint8)


def decode_stream(stream, fmt):
    """One stream -> float32 [frames, G]."""
    if fmt == "s16":
        return (np.asarray(stream, dtype=np.int16).astype(np.float64) / 32768.0).astype(np.float32)
    if fmt == "s24":
        return (s24_codes(stream).astype(np.float64) / 8388608.0).astype(np.float32)
    return np.asarray(stream, dtype=np.float32)


def decode(streams, fmt):
    """A list of streams -> planar float32 [nStreams * G, frames]."""
    return np.ascontiguousarray(np.concatenate([decode_stream(s, fmt).T for s in streams], axis=0))


def random_streams(fmt, frames, G, n_streams, seed, amp=0.8):
    """Streams in the layout ``process_blocks_pcm_io`` takes, at about ``amp`` of full scale."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_streams):
        x = rng.uniform(-amp, amp, size=(frames, G))
        if fmt == "s16":
            out.append(np.rint(x * 32767).astype(np.int16))
        elif fmt == "s24":
            out.append(s24_bytes(np.rint(x * 8388607).astype(np.int32)))
        else:
            out.append(x.astype(np.float32))
    return out
