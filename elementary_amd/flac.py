"""``FlacWriter`` — the container around the FLAC frames the engine delivers (``Runtime.process_blocks_flac`` / ``flac_flush``, or the
host twin ``runtime.flac_encode``): the ``fLaC`` marker and a STREAMINFO block in front, the frames appended as they come, and at
``close`` the smallest / largest frame size and the total sample count patched into STREAMINFO.

The STREAMINFO MD5 comes from the engine too: with option ``flac_md5`` = 1 every stream's digest runs on the GPU next to the encoder
and ``Runtime.flac_read()['md5']`` holds it after the flush (``patch(md5=...)``); no unencoded sample reaches the host for it. Without
the option the field stays all zero — "not computed" in RFC 9639's words; decoders accept that and skip their check.

``FlacReader`` — the other direction: a FLAC file as an input of the offline render, indexed on the host and decoded on the GPU."""
from __future__ import annotations

import struct
from typing import Iterable, Optional


def streaminfo(flac_frame: int, bits: int, channels: int, sample_rate: int, total_samples: int = 0, min_frame: int = 0, max_frame: int = 0,
               md5: bytes = bytes(16)) -> bytes:
    """The 34 bytes of a STREAMINFO block for a fixed-block-size stream; ``md5``: the 16 bytes of the unencoded samples' digest (all
    zero: not computed)."""
    if len(md5) != 16:
        raise ValueError("an MD5 is 16 bytes")
    if not (1 <= channels <= 8) or not (4 <= bits <= 32) or not (0 < sample_rate < (1 << 20)) or not (0 <= total_samples < (1 << 36)):
        raise ValueError("STREAMINFO cannot hold these stream parameters")
    v = (int(sample_rate) << 44) | ((int(channels) - 1) << 41) | ((int(bits) - 1) << 36) | int(total_samples)
    return (struct.pack(">HH", int(flac_frame), int(flac_frame)) + int(min_frame).to_bytes(3, "big") + int(max_frame).to_bytes(3, "big")
            + v.to_bytes(8, "big") + bytes(md5))


class FlacReader:
    """One FLAC file as an input of the offline render (``in_fmt='flac'``): the metadata blocks are walked — STREAMINFO parsed, every
    other block skipped — and the frames behind them indexed (``elemhip_flac_index``: header CRC-8, consecutive frame numbers, fixed
    fields; the frames' CRC-16 is checked on the GPU). ``read(n)`` returns a ``FlacChunk``: a view of the frames that cover the next
    ``n`` samples, their slice of the table and the position — the compressed bytes are what crosses the host link, the samples are
    decoded on the GPU (``flac_decode.hip``). Fixed-block-size streams of 8 / 12 / 16 / 20 / 24 bits with blocks of up to 16384 samples.

    ``md5`` holds the 16 bytes STREAMINFO announces (all zero: none) and every chunk carries them. They are verified where the caller
    asks for it — ``verify_input=True`` of ``process_wav`` / ``process_pcm_io`` / ``process_flac`` / ``master_wav``, ``verify=True`` of
    ``update_virtual_file_system_files`` — against a digest the GPU computes over the decoded samples (option ``flac_in_md5``), which
    never reach the host. Every frame's CRC-16 is checked always. Unlike ``WavReader``,
    which streams, the whole (compressed) file is read into memory at construction: the index needs every frame header."""

    def __init__(self, path):
        import numpy as np
        from .runtime import flac_index
        with open(path, "rb") as f:
            raw = f.read()
        if raw[:4] != b"fLaC":
            raise ValueError("no fLaC marker")
        pos, last, info = 4, False, None
        while not last:
            if pos + 4 > len(raw):
                raise ValueError("the metadata blocks run past the file's end")
            last, kind = bool(raw[pos] & 0x80), raw[pos] & 0x7F
            size = int.from_bytes(raw[pos + 1:pos + 4], "big")
            if pos == 4:
                if kind != 0 or size != 34 or pos + 4 + size > len(raw):
                    raise ValueError("the first metadata block is not STREAMINFO")
                body = raw[pos + 4:pos + 4 + size]
                v = int.from_bytes(body[10:18], "big")
                info = {"min_block": struct.unpack(">H", body[0:2])[0], "max_block": struct.unpack(">H", body[2:4])[0],
                        "md5": bytes(body[18:34]), "rate": v >> 44, "channels": ((v >> 41) & 7) + 1, "bits": ((v >> 36) & 31) + 1, "total": v & ((1 << 36) - 1)}
            pos += 4 + size
        if info["min_block"] != info["max_block"]:
            raise ValueError("variable block size streams are not read")
        self.sample_rate, self.channels, self.bits, self.flac_frame = info["rate"], info["channels"], info["bits"], info["max_block"]
        self.fmt = "flac"
        self.md5 = info["md5"]
        self._data = np.frombuffer(raw, dtype=np.uint8)[pos:]
        self._off, self._first = flac_index(self._data, self.channels, self.bits, self.flac_frame)
        self.frames = int(self._first[-1])                  # samples per channel ("frames" as WavReader counts them)
        if info["total"] and info["total"] != self.frames:
            raise ValueError(f"STREAMINFO announces {info['total']} samples, the frames hold {self.frames}")
        self.flac_frames = len(self._off) - 1
        self._pos = 0

    def seek(self, position: int) -> None:
        self._pos = int(position)

    def read(self, n: int):
        """The next ``n`` samples as a ``FlacChunk`` (the part past the stream's end is silence); the cursor moves on by ``n``."""
        import numpy as np
        from .runtime import FlacChunk
        n, p0 = int(n), self._pos
        self._pos += n
        p1 = min(p0 + n, self.frames)
        if p0 >= p1:
            return self._announce(FlacChunk(self._data[:0], [0], [p0], self.channels, self.bits, self.frames, p0, n))
        j0 = int(np.searchsorted(self._first, p0, side="right")) - 1
        j1 = int(np.searchsorted(self._first, p1 - 1, side="right")) - 1
        base = int(self._off[j0])
        return self._announce(FlacChunk(self._data[base:int(self._off[j1 + 1])], self._off[j0:j1 + 2] - np.uint64(base), self._first[j0:j1 + 2],
                                        self.channels, self.bits, self.frames, p0, n))

    def _announce(self, chunk):
        chunk.md5 = self.md5            # what the file says its samples hash to (``verify_input``)
        return chunk

    def close(self) -> None:
        self._data = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class FlacWriter:
    """One FLAC file of one stream. ``write(data, frame_bytes)`` appends whole frames (``frame_bytes``: their byte lengths, for the
    STREAMINFO minimum / maximum; without it those fields stay 0, "unknown"); ``close(total_samples)`` patches the header."""

    def __init__(self, path, bits: int, channels: int, sample_rate: int, flac_frame: int = 4096):
        self.bits, self.channels, self.sample_rate, self.flac_frame = int(bits), int(channels), int(round(sample_rate)), int(flac_frame)
        self.frames = 0
        self.total_samples = 0
        self.min_frame = self.max_frame = 0
        self.md5 = bytes(16)
        self._sized = True
        self._f = open(path, "wb")
        self._f.write(b"fLaC" + bytes([0x80]) + (34).to_bytes(3, "big") + streaminfo(self.flac_frame, self.bits, self.channels, self.sample_rate))

    def write(self, data: bytes, frame_bytes: Optional[Iterable[int]] = None) -> None:
        if not data:
            return
        self._f.write(data)
        if frame_bytes is None:
            self._sized = False
            return
        sizes = [int(b) for b in frame_bytes]
        if sum(sizes) != len(data):
            raise ValueError("the frame lengths do not add up to the data")
        self.frames += len(sizes)
        self.min_frame = min(sizes + ([self.min_frame] if self.min_frame else []))
        self.max_frame = max(sizes + [self.max_frame])

    def patch(self, frames: int, min_frame: int, max_frame: int, total_samples: int, md5: Optional[bytes] = None) -> None:
        """The STREAMINFO figures from elsewhere (``Runtime.flac_read``) for frames that were written without their lengths; ``md5``:
        the stream's digest (``flac_read()['md5'][s]`` at ``md5_state`` 2, or a ``FlacMd5`` digest), which ``close`` writes."""
        self.frames, self.min_frame, self.max_frame, self.total_samples, self._sized = int(frames), int(min_frame), int(max_frame), int(total_samples), True
        if md5 is not None:
            if len(md5) != 16:
                raise ValueError("an MD5 is 16 bytes")
            self.md5 = bytes(md5)

    def close(self, total_samples: Optional[int] = None) -> None:
        if self._f is None:
            return
        total_samples = self.total_samples if total_samples is None else total_samples
        lo, hi = (self.min_frame, self.max_frame) if self._sized else (0, 0)
        self._f.seek(8)
        self._f.write(streaminfo(self.flac_frame, self.bits, self.channels, self.sample_rate, int(total_samples), lo, hi, self.md5))
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
