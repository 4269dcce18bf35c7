"""FLAC input without a GPU.

1. tests/flac_reference.py against one LPC frame and one wasted-bits frame assembled here from literal bit strings after RFC 9639's
   layout — so that tests/flac_writer.py and the decoders cannot share a misreading.
2. The corpus (flac_writer.corpus()): the writer's frames, decoded by flac_reference, are the writer's samples.
3. elemhip_flac_index / elemhip_flac_decode (elementary_amd/csrc/flac_decode.h behind the C-ABI) on the corpus and on
   elemhip_flac_encode's output, against flac_reference: every table entry, every code.
4. tests/native/flac_decode_host.cpp: the kernels' lane functions lane by lane against decode_host() on the corpus, and once more under
   the address and undefined-behaviour sanitizers on the corpus and the corrupt corpus — every single-bit flip and every truncation of
   one 16-sample stereo frame, and a frame whose unary run continues past its end.
5. FlacReader on files of FlacWriter and of the test writer: chunks that cover exactly the frames asked for, metadata skipped.

Every comparison is exact."""
import os
import struct
import subprocess

import numpy as np
import pytest

import flac_reference as ref
import flac_writer as fw
from test_flac_host import _cxx, _frame, _header, _s

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elementary_amd", "csrc")


@pytest.fixture(scope="module")
def corpus():
    return fw.corpus()


# ---- 1. literal frames -------------------------------------------------------------------------------------------------------------------
def test_reference_reads_a_literal_lpc_frame():
    # order 1, precision 4, shift 1, coefficient 3: prediction (3 s[i-1]) >> 1. Warm-up 10; residuals 1, -1, 1 (zigzag 2, 1, 2) at k = 1
    body = ("0 100000 0" + _s(10, 16) + "0011" + "00001" + "0011"
            + "00" + "0000" + "0001" + "01 0" + "1 1" + "01 0")
    f, _ = ref.decode_frame(_frame(_header(4), body))
    assert f["channels"] == [[10, 16, 23, 35]]
    sub = f["subframes"][0]
    assert (sub["kind"], sub["order"], sub["params"]) == ("LPC", 1, [1])


def test_reference_reads_a_literal_wasted_bits_frame():
    # VERBATIM with two wasted bits (flag 1, then unary 1: "01"): 14-bit codes 1, -2, 3, 0 are the samples 4, -8, 12, 0
    body = "0 000001 1" + "01" + "".join(_s(v, 14) for v in (1, -2, 3, 0))
    f, _ = ref.decode_frame(_frame(_header(4), body))
    assert f["channels"] == [[4, -8, 12, 0]] and f["subframes"][0]["wasted"] == 2 and f["subframes"][0]["bps"] == 14


def test_writer_writes_the_literal_frames():
    lpc = fw.write_frame([[10, 16, 23, 35]], 16, 0, subs=[dict(kind="LPC", coefs=[3], precision=4, shift=1, porder=0, params=[1])], explicit_block=True)
    assert lpc == _frame(_header(4), "0 100000 0" + _s(10, 16) + "0011" + "00001" + "0011" + "00" + "0000" + "0001" + "01 0" + "1 1" + "01 0")
    wasted = fw.write_frame([[4, -8, 12, 0]], 16, 0, subs=[dict(kind="VERBATIM", wasted=2)], explicit_block=True)
    assert wasted == _frame(_header(4), "0 000001 1" + "01" + "".join(_s(v, 14) for v in (1, -2, 3, 0)))


# ---- 2. the corpus through the reference ----------------------------------------------------------------------------------------------------
def test_corpus_decodes_to_the_writers_samples(corpus):
    kinds, orders, wasted, escapes, assignments, sizes = set(), set(), set(), set(), set(), set()
    for name, data, chans, bps, bs in corpus:
        frames, got = ref.decode_frames(data)
        assert got == chans, name
        for f in frames:
            assignments.add(f["assignment"])
            sizes.add(f["blocksize"])
            for sub in f["subframes"]:
                kinds.add(sub["kind"])
                orders.add((sub["kind"], sub.get("order")))
                wasted.add(sub["wasted"])
                escapes.update(p[1] for p in sub.get("params", []) if isinstance(p, tuple))
    assert kinds == {"CONSTANT", "VERBATIM", "FIXED", "LPC"}
    assert {("FIXED", o) for o in range(5)} | {("LPC", o) for o in (1, 8, 12, 32)} <= orders
    assert {0, 1, 7} <= wasted and {0, 17} <= escapes and {8, 9, 10, 0, 1, 7} <= assignments
    assert {16, 192, 4096, 4608, 16384, 1, 17} <= sizes


# ---- 3. the C-ABI's index and scalar twin ---------------------------------------------------------------------------------------------------
def _check_against_reference(name, data, bps, bs):
    from elementary_amd.runtime import FlacChunk, flac_decode, flac_index
    frames, chans = ref.decode_frames(data)
    off, first = flac_index(data, len(chans), bps, bs)
    want_off = np.cumsum([0] + [f["bytes"] for f in frames])
    want_first = np.cumsum([0] + [f["blocksize"] for f in frames])
    assert np.array_equal(off, want_off.astype(np.uint64)) and np.array_equal(first, want_first.astype(np.uint64)), name
    total = int(want_first[-1])
    whole = FlacChunk(np.frombuffer(data, dtype=np.uint8), off, first, len(chans), bps, total, 0, total)
    assert np.array_equal(flac_decode(whole), np.array(chans, dtype=np.int32)), name
    # a range cut inside frames that runs past the end: the same codes, zeros behind
    p0 = total // 3
    part = flac_decode(whole.at(p0, total - p0 + 5))
    assert np.array_equal(part[:, :total - p0], np.array(chans, dtype=np.int32)[:, p0:]) and not part[:, total - p0:].any(), name


def test_index_and_twin_on_the_corpus(corpus):
    for name, data, chans, bps, bs in corpus:
        _check_against_reference(name, data, bps, bs)


@pytest.mark.parametrize("bits", [16, 24])
def test_index_and_twin_on_the_encoders_output(bits):
    from elementary_amd.runtime import flac_encode
    rng = np.random.RandomState(bits)
    t = np.arange(3 * 256 + 77)
    lim = (1 << (bits - 1)) - 1
    codes = np.stack([(0.5 * lim * np.sin(t * 0.02) + rng.randint(-40, 41, t.size)).astype(np.int32),
                      (0.4 * lim * np.sin(t * 0.021 + 1) + rng.randint(-40, 41, t.size)).astype(np.int32)])
    data, _ = flac_encode(codes, bits=bits, flac_frame=256)
    _check_against_reference("encoder", data, bits, 256)


def test_index_with_a_block_size_of_zero_takes_the_first_frames(corpus):
    from elementary_amd.runtime import flac_index
    name, data, chans, bps, bs = corpus[0]
    assert np.array_equal(flac_index(data, len(chans), bps, 0)[1], flac_index(data, len(chans), bps, bs)[1])


def test_index_refuses_what_the_decoder_does_not_read():
    from elementary_amd.runtime import ElemHipError, flac_index
    x = list(range(16))
    for data, bits in ((fw.write_frame([x], 16, 0, variable=True), 16),                       # variable block size
                       (fw.write_frame([x], 16, 0, bps_code=7), 32),                         # a 32-bit stream
                       (bytes(64), 16)):                                                      # no frame at all
        with pytest.raises(ElemHipError) as e:
            flac_index(data, 1, bits, 0)
        assert e.value.code == 106


# ---- 4. the lane functions against the scalar twin, and the sanitizers -----------------------------------------------------------------------
def good_frame():
    """One 16-sample stereo frame (mid/side, FIXED with an escape, LPC): what the corrupt corpus is made of. Returns it and its samples."""
    l, r = fw._noise(16, 16, 1), fw._noise(16, 16, 2)
    good = fw.write_frame([l, r], 16, 5, assignment="mid_side",
                          subs=[dict(kind="FIXED", order=2, porder=1, params=[9, ("escape", 17)]),
                                dict(kind="LPC", coefs=[5, -3], precision=6, shift=2, porder=0, params=[10], wasted=0)])
    assert ref.decode_frame(good)[0]["channels"] == [l, r]
    return good, [l, r]


def named_corrupt():
    """Frames with a valid CRC-16 that a decoder has to refuse for another reason (they are part of the corrupt corpus)."""
    good, (l, r) = good_frame()
    head = bytes([0xFF, 0xF8, 0x09, 0xA8, 0x06])          # block-size code 0 (reserved) under a valid CRC-8, mid/side, 16 bits, number 6
    code0 = head + bytes([ref.crc8(head)]) + good[7:-2]
    return {"block_code0": code0 + ref.crc16(code0).to_bytes(2, "big"),
            "reserved_type": fw.write_frame([l, r], 16, 6, subs=[dict(raw_type=2), dict(kind="VERBATIM")]),
            "variable": fw.write_frame([l, r], 16, 6, variable=True),
            "bps32": fw.write_frame([l, r], 16, 6, bps_code=7)}


def test_twin_names_the_reason_of_a_refused_frame():
    from elementary_amd.runtime import ElemHipError, FlacChunk, flac_decode, flac_index
    good, chans = good_frame()
    for name, reason in (("block_code0", 2), ("reserved_type", 2), ("variable", 6), ("bps32", 6)):
        frame = named_corrupt()[name]
        if name != "reserved_type":                 # (a header the index does not accept; the reserved subframe type lies behind a good one)
            with pytest.raises(ElemHipError) as e:
                flac_index(frame, 2, 16, 0)
            assert e.value.code == 106, name
        data = good + frame
        c = FlacChunk(np.frombuffer(data, dtype=np.uint8), [0, len(good), len(data)], [0, 16, 32], 2, 16, 32, 0, 32)
        with pytest.raises(ElemHipError) as e:
            flac_decode(c)
        assert (e.value.code, e.value.frame, e.value.reason) == (106, 1, reason), name
        assert np.array_equal(flac_decode(c.at(0, 16)), np.array(chans, dtype=np.int32))      # the frame in front still decodes


def _corrupt_corpus():
    good, _ = good_frame()
    cases = [good] + list(named_corrupt().values())
    for bit in range(len(good) * 8):
        bad = bytearray(good)
        bad[bit >> 3] ^= 0x80 >> (bit & 7)
        cases.append(bytes(bad))
    cases += [good[:k] for k in range(len(good))]
    # a frame whose unary run continues past its end: the residual's bits are all zero up to and through the CRC's place
    head = good[:7]
    runaway = head + bytes([0b00010000, 0b00000000, 0b00000000]) + bytes(12)      # FIXED 0, method 0, porder 0, k = 0, then zeros only
    cases.append(runaway + ref.crc16(runaway).to_bytes(2, "big"))
    return cases


def _corpus_file(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for data, channels, bps, bs, strict in cases:
            f.write(struct.pack("<IIIIQ", channels, bps, bs, 1 if strict else 0, len(data)) + data)


def _build(workdir, name, extra):
    cxx = _cxx()
    assert cxx, "a C++17 compiler builds the host emulation"
    exe = os.path.join(str(workdir), name)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", *extra, "-I", CSRC, os.path.join(ROOT, "tests", "native", "flac_decode_host.cpp"),
                    "-o", exe], check=True)
    return exe


def test_lane_functions_give_the_scalar_twins_codes(tmp_path, corpus):
    path = os.path.join(str(tmp_path), "corpus.bin")
    _corpus_file(path, [(data, len(chans), bps, bs, True) for _, data, chans, bps, bs in corpus])
    res = subprocess.run([_build(tmp_path, "flac_decode_host", []), path], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and ("%d cases, 0 failures" % len(corpus)) in res.stdout, (res.stdout[-3000:], res.stderr[-3000:])


def test_lane_functions_are_clean_under_asan_and_ubsan_on_corrupt_frames(tmp_path, corpus):
    corrupt = _corrupt_corpus()
    assert len(corrupt) > 500
    path = os.path.join(str(tmp_path), "corrupt.bin")
    _corpus_file(path, [(data, len(chans), bps, bs, True) for _, data, chans, bps, bs in corpus] + [(c, 2, 16, 16, False) for c in corrupt])
    exe = _build(tmp_path, "flac_decode_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    res = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "0 failures" in res.stdout, (res.stdout[-3000:], res.stderr[-3000:])
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-2000:]


def test_the_kernels_take_their_arithmetic_from_the_header():
    hip = open(os.path.join(CSRC, "flac_decode.hip")).read()
    for call in ("fd::parse_lane(", "fd::fixed_seed(", "fd::lpc_sample(", "fd::lane_crc(", "fd::stereo_pair(", "fd::in_range(", "fd::image_piece("):
        assert call in hip, call
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "flac_decode.h" in mk and "flac_decode.o" in mk and "engine_flac_in.cpp" in mk


# ---- 5. FlacReader ----------------------------------------------------------------------------------------------------------------------------
def test_flac_reader_chunks_cover_exactly_the_frames_asked_for(tmp_path):
    from elementary_amd.flac import FlacReader
    from elementary_amd.runtime import flac_decode
    bs = 64
    chans = [fw._noise(5 * bs + 17, 16, 1), fw._noise(5 * bs + 17, 16, 2)]
    frames = fw.write_stream(chans, 16, bs, assignment="left_side", subs=[dict(kind="FIXED", order=2, porder=0, params=[10], method=1)] * 2)
    path = os.path.join(str(tmp_path), "t.flac")
    with open(path, "wb") as f:      # a PADDING and a VORBIS_COMMENT block behind STREAMINFO: skipped
        f.write(fw.file_bytes(frames, 16, 2, bs, len(chans[0]), extra_blocks=[(1, bytes(40)), (4, b"\x00" * 8)]))
    r = FlacReader(path)
    assert (r.channels, r.bits, r.flac_frame, r.frames, r.flac_frames, r.sample_rate) == (2, 16, bs, 5 * bs + 17, 6, 44100)
    want = np.array(chans, dtype=np.int32)
    sizes = [len(ref.decode_frame(frames, 0)[0]["channels"][0])]
    a = r.read(bs + 10)              # samples [0, 74): frames 0 and 1
    assert (a.frames, a.position, a.count, int(a.first_samples[0]), int(a.first_samples[-1])) == (2, 0, bs + 10, 0, 2 * bs) and sizes == [bs]
    assert np.array_equal(flac_decode(a), want[:, :bs + 10])
    b = r.read(2 * bs - 10)          # samples [74, 192): frames 1 and 2, ending on a frame's last sample
    assert (b.frames, b.position, int(b.first_samples[0]), int(b.first_samples[-1]), int(b.offsets[0])) == (2, bs + 10, bs, 3 * bs, 0)
    assert np.array_equal(flac_decode(b), want[:, bs + 10:3 * bs])
    c = r.read(10 * bs)              # the rest and past the end: frames 3, 4 and the short one; silence behind
    assert (c.frames, int(c.first_samples[-1])) == (3, 5 * bs + 17)
    got = flac_decode(c)
    assert np.array_equal(got[:, :2 * bs + 17], want[:, 3 * bs:]) and not got[:, 2 * bs + 17:].any()
    d = r.read(5)                    # nothing left
    assert d.frames == 0 and not flac_decode(d).any()


def test_flac_reader_reads_flac_writers_files(tmp_path):
    from elementary_amd.flac import FlacReader, FlacWriter
    from elementary_amd.runtime import flac_decode, flac_encode
    rng = np.random.RandomState(3)
    codes = rng.randint(-3000, 3000, (2, 2 * 256 + 50)).astype(np.int32)
    data, lens = flac_encode(codes, bits=24, flac_frame=256, sample_rate=48000)
    path = os.path.join(str(tmp_path), "w.flac")
    with FlacWriter(path, 24, 2, 48000, flac_frame=256) as w:
        w.write(data, lens)
        w.total_samples = codes.shape[1]
    r = FlacReader(path)
    assert (r.channels, r.bits, r.sample_rate, r.frames, r.flac_frames) == (2, 24, 48000, codes.shape[1], 3)
    assert np.array_equal(flac_decode(r.read(codes.shape[1])), codes)


def test_flac_reader_refuses_other_files(tmp_path):
    from elementary_amd.flac import FlacReader
    p = os.path.join(str(tmp_path), "x.flac")
    with open(p, "wb") as f:
        f.write(b"RIFF" + bytes(40))
    with pytest.raises(ValueError):
        FlacReader(p)
