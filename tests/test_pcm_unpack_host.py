"""PCM input without a GPU: elementary_amd/csrc/pcm_unpack.h — the header the unpack kernel (pcm_unpack.hip) takes its arithmetic and
every index from — compiled for the host and driven by tests/native/pcm_unpack_host.cpp: the kernel's three stages emulated thread by
thread over block sizes 32, 341, 350 and 512, G = 1, 2, 3, 6 and 8, the three formats, sets of 1 and 3 blocks, whole and cut at 37
frames of the last block, into a poisoned destination, against the scalar loop; the same program once more under the address and
undefined-behaviour sanitizers; the decoded bits it prints against the numpy restatement (tests/pcm_unpack_reference.py), which was
not derived from the header; and the RIFF reader (elementary_amd/wav.py)."""
import json
import os
import shutil
import struct
import subprocess
import wave

import numpy as np
import pytest

import pcm_reference as ref
import pcm_unpack_reference as uref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elementary_amd", "csrc")


def _cxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++")):
        if c and os.path.exists(c):
            return c
    return None


def _build_and_run(workdir, name, extra):
    cxx = _cxx()
    assert cxx, "a C++17 compiler builds the host emulation"
    exe = os.path.join(str(workdir), name)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "pcm_unpack_host.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-3000:])
    return json.loads(res.stdout.strip().splitlines()[-1]), res.stderr


@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("pcm_in"), "pcm_unpack_host", [])[0]


def test_lane_schedule_writes_every_float_once_with_the_scalar_loops_bits(emulation):
    out = emulation
    print({k: v for k, v in out.items() if not isinstance(v, list)})
    # 4 sizes x 5 groups x 3 formats x 2 set lengths x (whole, cut), 6 sets with a block wholly behind the valid frames, 2 wide groups
    assert out["ok"] and out["failures"] == 0 and out["cases"] == 4 * 5 * 3 * 2 * 2 + 6 + 2, out["cases"]
    assert out["wide_loads"] > 0 and out["wide_stores"] > 0 and out["narrow_stores"] > 0 and out["wide_stores"] > 20 * out["narrow_stores"]
    assert out["zero_floats"] > 0                                   # (frames behind a cut were there to be zeroed)
    # stage B's transposed write of the skewed LDS rows and stage C's four dword reads per quad: no half-wave hits a bank twice
    assert out["half_wave_writes"] > 0 and out["write_conflicts"] == 0 and out["skew_conflicts"] == 0
    assert out["half_wave_reads"] > 0 and out["read_conflicts"] == 0


def test_every_s16_code_decodes_as_the_reference_says_and_packs_back(emulation):
    codes = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    got = np.array(emulation["s16"], dtype=np.uint32).view(np.float32)
    want = uref.decode_stream(codes[:, None], "s16")[:, 0]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[0] == np.float32(-1.0) and float(got[-1]) == 0.999969482421875
    assert np.array_equal(ref.pack(got[None, :], 1, "s16")[0][:, 0], codes)          # no dither: the codes come back
    assert np.array_equal(ref.quant(got, 16, np.zeros(len(got), np.float32)), codes.astype(np.int32))


def test_s24_extremes_and_strided_codes(emulation):
    codes = (-8388608 + 4097 * np.arange(4096, dtype=np.int64)).astype(np.int32)
    assert codes[0] == -8388608 and codes[-1] == 8388607
    got = np.array(emulation["s24"], dtype=np.uint32).view(np.float32)
    want = uref.decode_stream(uref.s24_bytes(codes)[:, None, :], "s24")[:, 0]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[0] == np.float32(-1.0) and float(got[-1]) == 0.99999988079071045
    packed = ref.pack(got[None, :], 1, "s24")[0]
    assert np.array_equal(uref.s24_codes(packed)[:, 0], codes) and ref.same_bytes(packed[:, 0, :], uref.s24_bytes(codes))


def test_f32_bit_patterns_pass_unchanged(emulation):
    pats = np.array(emulation["f32_in"], dtype=np.uint32)
    f = pats.view(np.float32)
    assert np.isnan(f).sum() >= 5 and np.isinf(f).sum() == 2 and 0x7FA5A5A5 in pats.tolist()         # NaN payloads, both infinities ...
    assert ((pats & 0x7F800000) == 0).sum() >= 4                                                    # ... zeros and denormals
    assert emulation["f32_out"] == emulation["f32_in"]
    assert np.array_equal(uref.decode([pats.view(np.float32).reshape(4, 4)], "f32").view(np.uint32), pats.reshape(4, 4).T)


def test_emulation_is_clean_under_asan_and_ubsan(tmp_path):
    out, err = _build_and_run(tmp_path, "pcm_unpack_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert out["ok"] and out["failures"] == 0, out["failures"]
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]


def test_the_kernel_takes_its_indices_from_the_headers():
    hip = open(os.path.join(CSRC, "pcm_unpack.hip")).read()
    for call in ("pp::tile_valid(", "pu::tile_span(", "pp::tile_frames(", "pp::stretch_begin(", "pp::image_head(", "pp::image_offset(",
                 "pp::piece_count(", "pu::decode_bits(", "pp::row_chunks(", "pp::quad_first(", "pp::quad_whole(", "pu::quad_slot(",
                 "pp::lds_image_offset(", "pp::lds_table_offset(", "pp::lds_bytes("):
        assert call in hip, call
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "pcm_unpack.h" in mk and "pcm_unpack.o" in mk and "pcm_unpack.resource.txt" in mk


# ---- WavReader -------------------------------------------------------------------------------------------------------------------
def _stream(fmt, frames, ch, seed=3):
    return uref.random_streams(fmt, frames, ch, 1, seed)[0]


@pytest.mark.parametrize("ch", [1, 2, 3, 6])
@pytest.mark.parametrize("fmt", ["s16", "s24", "f32"])
def test_reader_returns_what_the_writer_was_given(tmp_path, fmt, ch):
    from elementary_amd.wav import WavReader, WavWriter
    frames = 333
    a = _stream(fmt, frames, ch)
    if fmt == "f32":
        a.view(np.uint32)[5, 0] = 0x7FA5A5A5                         # (nothing is converted: a NaN's payload survives)
    p = str(tmp_path / "x.wav")
    with WavWriter(p, fmt, ch, 44100.0) as w:
        w.write(a)
    with WavReader(p) as r:
        assert (r.fmt, r.channels, r.sample_rate, r.frames) == (fmt, ch, 44100, frames)
        parts = [r.read(100), r.read(100), r.read(1000)]
        assert [len(x) for x in parts] == [100, 100, 133] and len(r.read(10)) == 0
    assert ref.same_bytes(np.concatenate(parts), a)


def test_reader_reads_files_of_the_wave_module(tmp_path):
    from elementary_amd.wav import WavReader
    for fmt, width in (("s16", 2), ("s24", 3)):
        a = _stream(fmt, 77, 2)
        p = str(tmp_path / f"{fmt}.wav")
        with wave.open(p, "wb") as w:
            w.setnchannels(2); w.setsampwidth(width); w.setframerate(48000)
            w.writeframes(a.tobytes())
        with WavReader(p) as r:
            assert (r.fmt, r.channels, r.sample_rate, r.frames) == (fmt, 2, 48000, 77)
            assert ref.same_bytes(r.read(77), a)


def _riff(chunks):
    body = b"WAVE" + b"".join(struct.pack("<4sI", cid, len(data) if size is None else size) + data + (b"\0" if len(data) & 1 else b"")
                              for cid, data, size in chunks)
    return struct.pack("<4sI", b"RIFF", len(body)) + body


def _fmt(tag, ch, rate, bits):
    return struct.pack("<HHIIHH", tag, ch, rate, rate * ch * bits // 8, ch * bits // 8, bits)


def test_reader_skips_unknown_chunks_and_honours_the_pad_byte(tmp_path):
    from elementary_amd.wav import WavReader
    a = _stream("s24", 5, 1)                                        # 15 bytes of data: odd, so a pad byte follows
    p = str(tmp_path / "l.wav")
    open(p, "wb").write(_riff([(b"fmt ", _fmt(1, 1, 44100, 24), None), (b"LIST", b"INFOabc", None), (b"data", a.tobytes(), None),
                               (b"junk", b"12", None)]))
    with WavReader(p) as r:                                          # (the odd LIST chunk is skipped with ITS pad byte)
        assert (r.fmt, r.channels, r.frames) == ("s24", 1, 5) and ref.same_bytes(r.read(9), a)


def test_reader_reads_an_extensible_header(tmp_path):
    from elementary_amd.wav import WavReader
    tail = bytes.fromhex("000000001000800000aa00389b71")
    for fmt, tag, bits in (("s24", 1, 24), ("f32", 3, 32)):
        a = _stream(fmt, 21, 6)
        ext = _fmt(0xFFFE, 6, 48000, bits) + struct.pack("<HHI", 22, bits, 0x3F) + struct.pack("<H", tag) + tail
        p = str(tmp_path / f"e_{fmt}.wav")
        open(p, "wb").write(_riff([(b"fmt ", ext, None), (b"data", a.tobytes(), None)]))
        with WavReader(p) as r:
            assert (r.fmt, r.channels, r.sample_rate, r.frames) == (fmt, 6, 48000, 21) and ref.same_bytes(r.read(21), a)
    bad = _fmt(0xFFFE, 2, 48000, 16) + struct.pack("<HHI", 22, 16, 3) + struct.pack("<H", 1) + bytes(14)
    open(str(tmp_path / "g.wav"), "wb").write(_riff([(b"fmt ", bad, None), (b"data", bytes(8), None)]))
    with pytest.raises(ValueError, match="subformat"):
        WavReader(str(tmp_path / "g.wav"))


def test_reader_names_what_it_cannot_read(tmp_path):
    from elementary_amd.wav import WavReader
    cases = {"eight.wav": (_riff([(b"fmt ", _fmt(1, 2, 44100, 8), None), (b"data", bytes(16), None)]), "8 bits"),
             "short.wav": (_riff([(b"fmt ", _fmt(1, 2, 44100, 16), None), (b"data", bytes(10), 400)]), "truncated"),
             "nodata.wav": (_riff([(b"fmt ", _fmt(1, 2, 44100, 16), None), (b"LIST", b"INFO", None)]), "no 'data' chunk"),
             "notwav.wav": (b"OggS" + bytes(40), "not a RIFF/WAVE")}
    for name, (raw, what) in cases.items():
        open(str(tmp_path / name), "wb").write(raw)
        with pytest.raises(ValueError, match=what):
            WavReader(str(tmp_path / name))


# ---- the entry point on a handle without a device ---------------------------------------------------------------------------------
def test_arguments_are_judged_before_the_device_is_asked_for():
    """8 and 103 come from the arguments alone; a well-formed call on a dry handle is 101."""
    from elementary_amd.runtime import ElemHipError, Runtime
    rt = Runtime(48000.0, 512, device=-1)
    s16 = np.zeros((512, 2), np.int16)

    def code(*a, **k):
        with pytest.raises(ElemHipError) as e:
            rt.process_blocks_pcm_io(*a, **k)
        return e.value.code

    assert code([s16], 4, 2) == 8 and code([s16], "s16", 2, in_channels_per_stream=0) == 8
    assert code([np.zeros((512, 17), np.int16)] * 2, "s16", 2) == 103
    assert code([s16], "s16", out_fmt="s16", num_streams=513, channels_per_stream=2) == 103
    assert code([s16], "s16", out_fmt=7, num_streams=1, channels_per_stream=2) == 8
    assert code([s16], "s16", 2) == 101 and code([s16], "s16", out_fmt="s24", num_streams=1, channels_per_stream=2) == 101
    with pytest.raises(ValueError):
        rt.process_blocks_pcm_io([np.zeros((512, 2), np.float32)], "s16", 2)          # (a stream of the wrong kind)
