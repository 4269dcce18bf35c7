"""FLAC delivery without a GPU.

1. tests/flac_reference.py, the pure-Python decoder written from RFC 9639, against itself: the CRC check values and a handful of frames
   assembled here from literal bit strings after the specification's layout — so that encoder and decoder cannot share a misreading.
2. elementary_amd/csrc/flac_encode.h compiled for the host and driven by tests/native/flac_encode_host.cpp: the kernels' lane schedule
   emulated lane by lane against encode_host(), byte for byte, and once more under the address and undefined-behaviour sanitizers.
3. elemhip_flac_encode (the scalar twin behind the C-ABI) through the decoder: lossless on every signal, with size conditions that
   follow from the format, not from a measurement.
4. FlacWriter: files that decode, STREAMINFO with the right figures and an all-zero MD5."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import flac_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elementary_amd", "csrc")


# ---- 1. the decoder against literal bit strings ---------------------------------------------------------------------------------------
def _frame(header_bits, body_bits):
    """header (without CRC-8) and subframes as '0'/'1' strings -> a frame: CRC-8, zero padding and CRC-16 added."""
    hb = header_bits.replace(" ", "")
    assert len(hb) % 8 == 0
    head = int(hb, 2).to_bytes(len(hb) // 8, "big")
    head += bytes([ref.crc8(head)])
    bb = body_bits.replace(" ", "")
    bb += "0" * (-len(bb) % 8)
    body = int(bb, 2).to_bytes(len(bb) // 8, "big") if bb else b""
    data = head + body
    return data + ref.crc16(data).to_bytes(2, "big")


def _s(v, n):
    return format(v & ((1 << n) - 1), "0%db" % n)


def _header(n, channels="0000", number="00000000"):
    # sync, reserved 0, fixed block size | block size: 8-bit explicit | 44.1 kHz | channels | 16 bits | reserved | number | n - 1
    return "11111111111110 0 0" + "0110" + "1001" + channels + "100" + "0" + number + _s(n - 1, 8)


def test_crc_check_values():
    assert ref.crc8(b"123456789") == 0xF4
    assert ref.crc16(b"123456789") == 0xFEE8


def test_decoder_reads_a_constant_subframe():
    f, end = ref.decode_frame(_frame(_header(4), "0 000000 0" + _s(-3, 16)))
    assert f["channels"] == [[-3, -3, -3, -3]] and f["subframes"][0]["kind"] == "CONSTANT" and f["blocksize"] == 4 and f["rate"] == 44100
    assert end == f["bytes"] == 4 + 1 + 1 + 1 + 3 + 2


def test_decoder_reads_a_verbatim_subframe():
    x = [1, -1, 32767, -32768]
    f, _ = ref.decode_frame(_frame(_header(4), "0 000001 0" + "".join(_s(v, 16) for v in x)))
    assert f["channels"] == [x] and f["subframes"][0]["kind"] == "VERBATIM"


def test_decoder_reads_a_fixed_order_2_subframe_with_two_rice_partitions():
    # warm-up 10, 12; residuals 1 | -1, 0, 2 -> zigzag 2 | 1, 0, 4; partition 0 with k = 0, partition 1 with k = 1
    body = ("0 001010 0" + _s(10, 16) + _s(12, 16) + "00" + "0001"
            + "0000" + "001"
            + "0001" + "1 1" + "1 0" + "001 0")
    f, _ = ref.decode_frame(_frame(_header(6), body))
    assert f["channels"] == [[10, 12, 15, 17, 19, 23]]
    sub = f["subframes"][0]
    assert (sub["kind"], sub["order"], sub["porder"], sub["params"]) == ("FIXED", 2, 1, [0, 1])


def test_decoder_reads_an_escaped_partition():
    body = "0 001000 0" + "00" + "0000" + "1111" + "00011" + "001" + "110" + "011" + "100"
    f, _ = ref.decode_frame(_frame(_header(4), body))
    assert f["channels"] == [[1, -2, 3, -4]] and f["subframes"][0]["params"] == [("escape", 3)]


def test_decoder_reads_a_left_side_frame():
    f, _ = ref.decode_frame(_frame(_header(2, channels="1000"), "0 000000 0" + _s(5, 16) + "0 000000 0" + _s(2, 17)))
    assert f["channels"] == [[5, 5], [3, 3]] and f["assignment"] == 8 and f["subframes"][1]["bps"] == 17


def test_decoder_reads_the_coded_frame_number():
    # 2048 = 0x800 -> 1110 0000 | 10 100000 | 10 000000
    f, _ = ref.decode_frame(_frame(_header(4, number="11100000" + "10100000" + "10000000"), "0 000000 0" + _s(0, 16)))
    assert f["number"] == 2048


def test_decoder_rejects_damage_trailing_and_missing_bits():
    good = _frame(_header(4), "0 000000 0" + _s(7, 16))
    ref.decode_frames(good)
    with pytest.raises(ref.FlacError):
        ref.decode_frames(good + b"\x00")                                  # trailing
    with pytest.raises(ref.FlacError):
        ref.decode_frames(good[:-1])                                       # missing
    with pytest.raises(ref.FlacError):
        ref.decode_frames(good[:7] + bytes([good[7] ^ 1]) + good[8:])      # a flipped payload bit: CRC-16
    with pytest.raises(ref.FlacError):
        ref.decode_frames(good[:2] + bytes([good[2] ^ 0x10]) + good[3:])   # a flipped header bit: CRC-8
    with pytest.raises(ref.FlacError):
        ref.decode_frame(_frame(_header(4), "0 000000 0" + _s(7, 15) + "1" + "1"))     # one bit too many, set in the padding


# ---- 2. the lane schedule against the scalar twin ---------------------------------------------------------------------------------------
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
                    os.path.join(ROOT, "tests", "native", "flac_encode_host.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-3000:])
    return json.loads(res.stdout.strip().splitlines()[-1]), res.stderr


@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("flac"), "flac_encode_host", [])[0]


def test_lane_schedule_gives_the_scalar_twins_bytes(emulation):
    out = emulation
    print(out)
    # frames 256 and 4096 x G 1, 2, 3, 8 x 16 and 24 bits x whole / 1 / 15 / 16 / 255 samples, every content kind (two per whole frame of
    # 4096); the seven frame numbers twice over; two odd frames whose outlier runs cross hundreds of words
    assert out["ok"] and out["failures"] == 0
    assert out["cases"] == 2 * 4 * 2 * 4 * 7 + 4 * 2 * (7 + 2) + 14 + 2, out["cases"]
    assert out["crc8"] == 0xF4 and out["crc16"] == 0xFEE8
    # every kind of subframe, every predictor order, escapes, deep partition orders, every stereo mode and long unary runs occurred
    assert out["constant"] > 0 and out["verbatim"] > 0 and all(n > 0 for n in out["fixed"]) and out["escapes"] > 0 and out["porder_max"] >= 4
    assert all(n > 0 for n in out["modes"]) and out["long_unary_lanes"] > 0
    assert out["wide_stores"] > 10 * out["narrow_stores"] > 0


def test_emulation_is_clean_under_asan_and_ubsan(tmp_path):
    out, err = _build_and_run(tmp_path, "flac_encode_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert out["ok"] and out["failures"] == 0, out["failures"]
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]


def test_the_kernels_take_their_arithmetic_from_the_header():
    hip = open(os.path.join(CSRC, "flac_encode.hip")).read()
    for call in ("fe::leaf(", "fe::tree_level(", "fe::decide(", "fe::lane_bits(", "fe::lane_emit(", "fe::choose_stereo(", "fe::stereo_candidate(",
                 "fe::header_put(", "fe::header_bytes(", "fe::frame_bytes(", "fe::frame_byte(", "fe::lane_crc(", "fe::candidate_sample(",
                 "pp::quantise(", "pp::dither(", "pp::stats_fold(", "pp::piece_whole("):
        assert call in hip, call
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "flac_encode.h" in mk and "flac_encode.o" in mk and "engine_flac.cpp" in mk


# ---- 3. the scalar twin through the decoder --------------------------------------------------------------------------------------------
def _signals(bits, n):
    lim = 1 << (bits - 1)
    i = np.arange(n)
    rng = np.random.default_rng(bits * 1000 + n)
    sine = np.rint(0.5 * lim * np.sin(2 * math.pi * 440.0 * i / 44100.0)).astype(np.int32)
    white = rng.integers(-lim, lim, size=n, dtype=np.int64).astype(np.int32)
    alt = np.where(i & 1, lim - 1, -lim).astype(np.int32)
    outlier = np.zeros(n, np.int32)
    outlier[n // 3] = lim - 1
    return {
        "silence": np.zeros((1, n), np.int32),
        "dc": np.full((1, n), -lim, np.int32),
        "ramp": ((i % 1000) - 500).astype(np.int32)[None, :],
        "sine": sine[None, :],
        "white": white[None, :],
        "alternating": alt[None, :],
        "alternating_stereo": np.stack([alt, -1 - alt]),          # L = +-full scale, R its mirror: the side channel needs all its 25 bits
        "equal": np.stack([sine, sine]),
        "opposite": np.stack([sine, -sine]),
        "outlier": outlier[None, :],
        "outlier_stereo": np.stack([outlier, white]),
    }


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("ff", [256, 4096])
def test_twin_is_lossless_and_no_longer_than_the_format_allows(bits, ff):
    from elementary_amd.runtime import flac_encode
    n = 2 * ff + 100                       # two whole frames and a short one
    for name, x in _signals(bits, n).items():
        data, lens = flac_encode(x, bits=bits, flac_frame=ff, sample_rate=44100)
        frames, chans = ref.decode_frames(data)
        G = x.shape[0]
        assert [f["bytes"] for f in frames] == lens.tolist() and sum(lens.tolist()) == len(data), name
        assert [f["blocksize"] for f in frames] == [ff, ff, 100] and [f["number"] for f in frames] == [0, 1, 2], name
        assert all(f["bps"] == bits and f["rate"] == 44100 for f in frames), name
        assert np.array_equal(np.array(chans, dtype=np.int64), x), name
        for f in frames:
            m, hb = f["blocksize"], f["header_bytes"]
            # no subframe is longer than its VERBATIM form, no stereo frame longer than its independent form
            assert f["bytes"] <= hb + (G * (8 + bits * m) + 7) // 8 + 2, (name, f["number"])
            assert all(sub["bits"] <= 8 + sub["bps"] * m for sub in f["subframes"]), name
            assert all(sub["wasted"] == 0 for sub in f["subframes"]), name
            if name in ("silence", "dc"):
                assert f["bytes"] == hb + (G * (8 + bits) + 7) // 8 + 2 and f["subframes"][0]["kind"] == "CONSTANT", name
            if name == "ramp":
                assert f["bytes"] <= G * (m // 8 + 32), (name, f["bytes"])
            if name == "equal":
                assert f["assignment"] in (8, 10) and f["subframes"][1]["kind"] == "CONSTANT", (name, f["assignment"])
        if name == "sine" and bits == 16:
            assert len(data) <= n * 2 // 2, len(data)            # an order-3 residual of a few LSB: about a quarter of s16
        if name == "alternating_stereo":
            assert max(abs(int(a) - int(b)) for a, b in zip(x[0], x[1])) == (1 << bits) - 1


def test_twin_cuts_and_numbers_frames_like_one_call():
    from elementary_amd.runtime import flac_encode
    x = _signals(16, 256 * 5 + 77)["outlier_stereo"]
    whole, lens = flac_encode(x, flac_frame=256)
    a, la = flac_encode(x[:, :512], flac_frame=256, flush=False)
    b, lb = flac_encode(x[:, 512:], flac_frame=256, first_frame_number=2)
    assert a + b == whole and la.tolist() + lb.tolist() == lens.tolist()
    head, _ = flac_encode(x[:, :300], flac_frame=256, flush=False)      # the remainder is left to the caller
    assert head == whole[:int(lens[0])]


@pytest.mark.parametrize("number", [0, 127, 128, 2047, 2048, 65536, 2 ** 31 - 1])
def test_twin_codes_frame_numbers_up_to_2_pow_31(number):
    from elementary_amd.runtime import flac_encode, ElemHipError
    x = _signals(16, 256)["sine"]
    data, _ = flac_encode(x, flac_frame=256, first_frame_number=number)
    f, _ = ref.decode_frame(data)
    assert f["number"] == number and np.array_equal(f["channels"][0], x[0])
    if number == 2 ** 31 - 1:
        with pytest.raises(ElemHipError):
            flac_encode(np.zeros((1, 512), np.int32), flac_frame=256, first_frame_number=number)


@pytest.mark.parametrize("rate,code_bytes", [(44100, 0), (96000, 0), (12345, 2), (352800, 2), (655350, 2), (384000, 2), (700001, 0)])
def test_twin_codes_sample_rates(rate, code_bytes):
    from elementary_amd.runtime import flac_encode
    x = np.zeros((1, 256), np.int32)
    data, _ = flac_encode(x, flac_frame=256, sample_rate=rate)
    f, _ = ref.decode_frame(data, 0, {"rate": rate, "bps": 16})
    assert f["rate"] == rate and f["header_bytes"] == 4 + 1 + code_bytes + 1


def test_twin_refuses_what_the_format_cannot_hold():
    from elementary_amd.runtime import flac_encode, ElemHipError
    for kw in ({"bits": 20}, {"flac_frame": 300}):
        with pytest.raises(ElemHipError) as e:
            flac_encode(np.zeros((1, 16), np.int32), **kw)
        assert e.value.code == 8
    with pytest.raises(ElemHipError) as e:
        flac_encode(np.zeros((9, 16), np.int32))
    assert e.value.code == 8
    with pytest.raises(ElemHipError) as e:
        flac_encode(np.full((1, 16), 32768, np.int32), bits=16)
    assert e.value.code == 6


# ---- 4. the container ------------------------------------------------------------------------------------------------------------------
def test_flac_writer_files_decode_with_the_right_streaminfo(tmp_path):
    from elementary_amd.flac import FlacWriter
    from elementary_amd.runtime import flac_encode
    n = 256 * 4 + 31
    sig = _signals(24, n)
    for s, x in enumerate((sig["sine"], sig["outlier_stereo"], np.concatenate([sig["equal"], sig["white"]]))):
        path = tmp_path / f"stream{s}.flac"
        data, lens = flac_encode(x, bits=24, flac_frame=256, sample_rate=48000)
        with FlacWriter(path, 24, x.shape[0], 48000, 256) as w:
            cut = int(lens[:2].sum())
            w.write(data[:cut], lens[:2])
            w.write(data[cut:], lens[2:])
            w.total_samples = n
        info, frames, chans = ref.decode_file(path.read_bytes())
        assert np.array_equal(np.array(chans, dtype=np.int64), x)
        assert info["md5"] == bytes(16) and info["total"] == n and info["channels"] == x.shape[0] and info["bps"] == 24 and info["rate"] == 48000
        assert (info["min_block"], info["max_block"]) == (256, 256)
        assert (info["min_frame"], info["max_frame"]) == (int(lens.min()), int(lens.max())) and len(frames) == 5
