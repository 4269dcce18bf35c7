"""RIFF/WAVE files for PCM streams (``OfflineRenderer.write_wav``): the header written here, the bytes as the engine packed them.

``s16`` and ``s24`` are WAVE_FORMAT_PCM (tag 1), ``f32`` is WAVE_FORMAT_IEEE_FLOAT (tag 3, with the ``fact`` chunk that format asks
for). A ``WavWriter`` is opened before the length is known, takes the streams of one ``process_pcm`` call after another and patches
the two sizes of the header when it is closed. A ``WavReader`` is the way back: it finds the ``fmt `` and ``data`` chunks of a file and hands out
the samples as they lie there, in the stream layout ``process_pcm_io`` takes — nothing is converted on the host.
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


_PCM_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")     # KSDATAFORMAT_SUBTYPE_*: the tag, then these 14 bytes


class WavReader:
    """A RIFF/WAVE file as PCM streams: ``fmt`` ('s16' / 's24' / 'f32'), ``channels``, ``sample_rate``, ``frames``; ``read(n)`` returns
    the next ``n`` frames (fewer at the end) as int16 / float32 ``[frames, channels]`` or uint8 ``[frames, channels, 3]``. Accepted:
    WAVE_FORMAT_PCM with 16 or 24 bits, WAVE_FORMAT_IEEE_FLOAT with 32 bits, and WAVE_FORMAT_EXTENSIBLE with those two subformats.
    Chunks other than ``fmt `` and ``data`` are skipped (with their pad byte). Anything else raises ``ValueError`` naming what was found."""

    def __init__(self, path: str):
        self._f = open(path, "rb")
        try:
            self._parse(path)
        except Exception:
            self._f.close()
            self._f = None
            raise

    def _parse(self, path):
        f = self._f
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError(f"{path}: not a RIFF/WAVE file (starts with {head[:12]!r})")
        fmt = None
        while True:
            ch = f.read(8)
            if len(ch) < 8:
                raise ValueError(f"{path}: no 'data' chunk" if fmt is not None else f"{path}: no 'fmt ' chunk")
            cid, size = struct.unpack("<4sI", ch)
            if cid == b"fmt ":
                body = f.read(size)
                if size < 16 or len(body) < size:
                    raise ValueError(f"{path}: a 'fmt ' chunk of {len(body)} bytes")
                tag, channels, rate, _, align, bits = struct.unpack("<HHIIHH", body[:16])
                if tag == 0xFFFE:
                    if size < 40 or body[26:40] != _PCM_GUID_TAIL:
                        raise ValueError(f"{path}: WAVE_FORMAT_EXTENSIBLE with subformat {body[24:40].hex() if size >= 40 else 'missing'}")
                    tag = struct.unpack("<H", body[24:26])[0]
                kind = {(1, 16): "s16", (1, 24): "s24", (3, 32): "f32"}.get((tag, bits))
                if kind is None or channels == 0 or align != channels * _BYTES[kind]:
                    raise ValueError(f"{path}: format tag {tag} with {bits} bits, {channels} channels, block align {align}: "
                                     "16- or 24-bit PCM (tag 1) or 32-bit float (tag 3) is read")
                fmt = (kind, channels, rate)
                if size & 1:
                    f.read(1)
            elif cid == b"data":
                if fmt is None:
                    raise ValueError(f"{path}: the 'data' chunk comes before 'fmt '")
                break
            else:
                f.seek(size + (size & 1), 1)
        self.fmt, self.channels, self.sample_rate = fmt
        width = self.channels * _BYTES[self.fmt]
        start = f.tell()
        f.seek(0, 2)
        have = f.tell() - start
        f.seek(start)
        if have < size:
            raise ValueError(f"{path}: truncated — the 'data' chunk announces {size} bytes, {have} are there")
        self.frames, self._left = size // width, size // width

    def read(self, frames: int) -> np.ndarray:
        n = max(0, min(int(frames), self._left))
        G, width = self.channels, _BYTES[self.fmt]
        raw = self._f.read(n * G * width)
        if len(raw) != n * G * width:
            raise ValueError(f"truncated: {len(raw)} of {n * G * width} bytes")
        self._left -= n
        if self.fmt == "s24":
            return np.frombuffer(raw, dtype=np.uint8).reshape(n, G, 3).copy()
        return np.frombuffer(raw, dtype="<i2" if self.fmt == "s16" else "<f4").reshape(n, G).astype(np.int16 if self.fmt == "s16" else np.float32, copy=True)

    def close(self) -> None:
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
