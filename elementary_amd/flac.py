"""``FlacWriter`` — the container around the FLAC frames the engine delivers (``Runtime.process_blocks_flac`` / ``flac_flush``, or the
host twin ``runtime.flac_encode``): the ``fLaC`` marker and a STREAMINFO block in front, the frames appended as they come, and at
``close`` the smallest / largest frame size and the total sample count patched into STREAMINFO.

The STREAMINFO MD5 stays all zero — "not computed" in RFC 9639's words: the unencoded samples never reach the host, and that is the
point of encoding on the GPU. Decoders accept it and skip their check."""
from __future__ import annotations

import struct
from typing import Iterable, Optional


def streaminfo(flac_frame: int, bits: int, channels: int, sample_rate: int, total_samples: int = 0, min_frame: int = 0, max_frame: int = 0) -> bytes:
    """The 34 bytes of a STREAMINFO block for a fixed-block-size stream."""
    if not (1 <= channels <= 8) or not (4 <= bits <= 32) or not (0 < sample_rate < (1 << 20)) or not (0 <= total_samples < (1 << 36)):
        raise ValueError("STREAMINFO cannot hold these stream parameters")
    v = (int(sample_rate) << 44) | ((int(channels) - 1) << 41) | ((int(bits) - 1) << 36) | int(total_samples)
    return (struct.pack(">HH", int(flac_frame), int(flac_frame)) + int(min_frame).to_bytes(3, "big") + int(max_frame).to_bytes(3, "big")
            + v.to_bytes(8, "big") + bytes(16))


class FlacWriter:
    """One FLAC file of one stream. ``write(data, frame_bytes)`` appends whole frames (``frame_bytes``: their byte lengths, for the
    STREAMINFO minimum / maximum; without it those fields stay 0, "unknown"); ``close(total_samples)`` patches the header."""

    def __init__(self, path, bits: int, channels: int, sample_rate: int, flac_frame: int = 4096):
        self.bits, self.channels, self.sample_rate, self.flac_frame = int(bits), int(channels), int(round(sample_rate)), int(flac_frame)
        self.frames = 0
        self.total_samples = 0
        self.min_frame = self.max_frame = 0
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

    def patch(self, frames: int, min_frame: int, max_frame: int, total_samples: int) -> None:
        """The STREAMINFO figures from elsewhere (``Runtime.flac_read``) for frames that were written without their lengths."""
        self.frames, self.min_frame, self.max_frame, self.total_samples, self._sized = int(frames), int(min_frame), int(max_frame), int(total_samples), True

    def close(self, total_samples: Optional[int] = None) -> None:
        if self._f is None:
            return
        total_samples = self.total_samples if total_samples is None else total_samples
        lo, hi = (self.min_frame, self.max_frame) if self._sized else (0, 0)
        self._f.seek(8)
        self._f.write(streaminfo(self.flac_frame, self.bits, self.channels, self.sample_rate, int(total_samples), lo, hi))
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
