"""elementary_amd/wav.py: the RIFF header is written by the module itself. S16 and S24 files read back with the standard library's
`wave` equal the streams; the IEEE-float header is checked field by field."""
import struct
import wave

import numpy as np

from elementary_amd.wav import WavWriter, header


def _streams(frames, ch):
    rng = np.random.default_rng(7)
    s16 = rng.integers(-32768, 32768, size=(frames, ch)).astype(np.int16)
    s24 = rng.integers(0, 256, size=(frames, ch, 3)).astype(np.uint8)
    f32 = rng.standard_normal((frames, ch)).astype(np.float32)
    return s16, s24, f32


def test_s16_and_s24_files_read_back_equal_the_streams(tmp_path):
    for frames, ch in ((1000, 2), (333, 3), (1, 1)):
        s16, s24, _ = _streams(frames, ch)
        for fmt, a, width in (("s16", s16, 2), ("s24", s24, 3)):
            p = str(tmp_path / f"{fmt}_{frames}_{ch}.wav")
            with WavWriter(p, fmt, ch, 44100.0) as w:      # in two pieces, as a streamed render arrives
                w.write(a[:frames // 2]); w.write(a[frames // 2:])
            with wave.open(p, "rb") as r:
                assert (r.getnchannels(), r.getsampwidth(), r.getframerate(), r.getnframes()) == (ch, width, 44100, frames)
                assert r.readframes(frames) == a.tobytes()
            size = len(open(p, "rb").read())
            assert size % 2 == 0 and struct.unpack("<I", open(p, "rb").read()[4:8])[0] == size - 8


def test_float_header_fields(tmp_path):
    _, _, f32 = _streams(321, 2)
    p = str(tmp_path / "f.wav")
    with WavWriter(p, "f32", 2, 48000.0) as w:
        w.write(f32)
    raw = open(p, "rb").read()
    riff, size, wav, fmt_id, fmt_len, tag, ch, rate, byte_rate, align, bits = struct.unpack("<4sI4s4sIHHIIHH", raw[:36])
    assert (riff, wav, fmt_id, fmt_len) == (b"RIFF", b"WAVE", b"fmt ", 16) and size == len(raw) - 8
    assert (tag, ch, rate, byte_rate, align, bits) == (3, 2, 48000, 48000 * 8, 8, 32)            # WAVE_FORMAT_IEEE_FLOAT
    fact, fact_len, fact_frames, data, data_len = struct.unpack("<4sII4sI", raw[36:56])
    assert (fact, fact_len, fact_frames, data, data_len) == (b"fact", 4, 321, b"data", 321 * 8)
    assert raw[56:] == f32.tobytes() and raw[:56] == header("f32", 2, 48000, 321)


def test_a_stream_of_the_wrong_kind_is_refused(tmp_path):
    import pytest
    with WavWriter(str(tmp_path / "x.wav"), "s16", 2, 48000.0) as w:
        with pytest.raises(ValueError):
            w.write(np.zeros((4, 3), np.int16))
        with pytest.raises(ValueError):
            w.write(np.zeros((4, 2), np.float32))
    with pytest.raises(ValueError):
        WavWriter(str(tmp_path / "y.wav"), "s32", 2, 48000.0)
