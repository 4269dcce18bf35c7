"""RIFF/WAVE files for PCM streams (``OfflineRenderer.write_wav``): the header written here, the bytes as the engine packed them.

``s16`` and ``s24`` are WAVE_FORMAT_PCM (tag 1), ``f32`` is WAVE_FORMAT_IEEE_FLOAT (tag 3, with the ``fact`` chunk that format asks
for). A ``WavWriter`` is opened before the length is known, takes the streams of one ``process_pcm`` call after another and patches
the two sizes of the header when it is closed.
"""
from __future__ import annotations

import struct

import numpy as np

_BYTES = {"s16": 2, "s24": 3, "f32": 4}


def header(fmt: str, channels: int, sample_rate: int, frames: int) -> bytes:
    """The bytes in front of the samples of a file of ``frames`` frames."""
    width = _BYTES[fmt]
    data = frames * channels * width
    tag = 3 if fmt == "f32" else 1
    fmt_chunk = struct.pack("<4sIHHIIHH", b"fmt ", 16, tag, channels, sample_rate, sample_rate * channels * width, channels * width, 8 * width)
    fact = struct.pack("<4sII", b"fact", 4, frames) if tag == 3 else b""
    pad = data & 1
    riff = 4 + len(fmt_chunk) + len(fact) + 8 + data + pad
    return struct.pack("<4sI4s", b"RIFF", riff, b"WAVE") + fmt_chunk + fact + struct.pack("<4sI", b"data", data)


class WavWriter:
    def __init__(self, path: str, fmt: str, channels: int, sample_rate: float):
        if fmt not in _BYTES:
            raise ValueError(f"unknown PCM format {fmt!r}: one of {sorted(_BYTES)}")
        self.fmt, self.channels, self.sample_rate, self.frames = fmt, int(channels), int(round(sample_rate)), 0
        self._f = open(path, "wb")
        self._f.write(header(fmt, self.channels, self.sample_rate, 0))

    def write(self, stream: np.ndarray) -> None:
        """One stream as ``process_pcm`` returns it: int16 / float32 ``[frames, G]`` or uint8 ``[frames, G, 3]``."""
        a = np.ascontiguousarray(stream)
        want = {"s16": np.int16, "s24": np.uint8, "f32": np.float32}[self.fmt]
        if a.dtype != want or a.ndim < 2 or a.shape[1] != self.channels or (self.fmt == "s24" and a.shape[2:] != (3,)):
            raise ValueError(f"a {self.fmt} stream of {self.channels} channels is expected, got {a.dtype} {a.shape}")
        if a.dtype.byteorder == ">":
            a = a.byteswap().newbyteorder()
        self._f.write(a.tobytes())
        self.frames += a.shape[0]

    def close(self) -> None:
        if self._f is None:
            return
        if (self.frames * self.channels * _BYTES[self.fmt]) & 1:
            self._f.write(b"\0")
        self._f.seek(0)
        self._f.write(header(self.fmt, self.channels, self.sample_rate, self.frames))
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
