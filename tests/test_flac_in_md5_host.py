"""The STREAMINFO MD5 of FLAC inputs and resources without a GPU (option "flac_in_md5"; elementary_amd/csrc/flac_in_md5.h).

1. FlacInMd5 — elemhip_flac_in_md5_update, which walks the kernel's schedule of chunks serially — against hashlib.md5 over the same
   codes packed by numpy as libFLAC hashes them: (bits + 7) // 8 bytes per sample, 12- and 20-bit codes sign-extended into their top
   byte; every padding residue, the empty message, both ends of the range and -1.
2. Updates in uneven pieces.
3. Refusals, and the delivery twin's own, which stay.
4. The option and the slots on a dry handle; a FLAC resource's digest through the dry loader.

The oracle is exact, so nothing here has a tolerance."""
import hashlib

import numpy as np
import pytest

EMPTY = bytes.fromhex("d41d8cd98f00b204e9800998ecf8427e")
BITS = (8, 12, 16, 20, 24)
GROUPS = (1, 2, 3, 8)


def sample_bytes(bits):
    return (bits + 7) // 8


def packed(codes, bits):
    """int [G, n] -> the bytes STREAMINFO's MD5 is defined over: sample by sample, channel by channel, the low B bytes, little-endian."""
    a = np.ascontiguousarray(np.asarray(codes, dtype=np.int32).T).astype("<i4")
    return np.ascontiguousarray(a.view(np.uint8).reshape(a.shape[0], a.shape[1], 4)[:, :, :sample_bytes(bits)]).tobytes()


def codes_of(G, n, bits, seed=1):
    rng = np.random.default_rng(seed * 1000003 + 97 * G + bits + 7 * n)
    x = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=(G, n), dtype=np.int64).astype(np.int32)
    if n >= 3:
        x[0, 0], x[-1, -1], x[0, 1] = -(1 << (bits - 1)), (1 << (bits - 1)) - 1, -1          # both ends of the range, and -1
    return x


def digest(codes, bits):
    from elementary_amd.runtime import FlacInMd5
    return FlacInMd5().update(codes, bits).digest()


def counts_for(G, bits):
    """Sample counts that leave 0, 1, 55, 56 and 63 bytes behind the last whole block (those G * B can reach), and ones that cross a
    chunk of 64 blocks and two."""
    B = sample_bytes(bits)
    want, counts = {0, 1, 55, 56, 63}, []
    for n in range(1, 400):
        r = (n * G * B) % 64
        if r in want:
            want.discard(r)
            counts.append(n)
    return counts + [4096 // (G * B) + 3, 2 * 4096 // (G * B) + 11]


# ---- 1. against hashlib ------------------------------------------------------------------------------------------------------------------
def test_the_oracle_sign_extends_short_codes():
    assert packed([[-1]], 12) == b"\xff\xff" and packed([[-2048]], 12) == b"\x00\xf8" and packed([[-1]], 20) == b"\xff\xff\xff"
    assert packed([[-(1 << 19)]], 20) == b"\x00\x00\xf8" and packed([[-128, 127]], 8) == b"\x80\x7f"


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("G", GROUPS)
def test_twin_equals_hashlib(G, bits):
    seen = set()
    for n in counts_for(G, bits):
        x = codes_of(G, n, bits)
        seen.add((n * G * sample_bytes(bits)) % 64)
        assert digest(x, bits) == hashlib.md5(packed(x, bits)).digest(), (G, bits, n)
    if G == 1 and sample_bytes(bits) == 1:
        assert {0, 1, 55, 56, 63} <= seen          # (a mono 8-bit stream reaches every residue)


@pytest.mark.parametrize("bits", BITS)
def test_the_empty_message_and_the_range_ends(bits):
    from elementary_amd.runtime import FlacInMd5
    assert FlacInMd5().digest() == EMPTY == hashlib.md5(b"").digest()
    assert FlacInMd5().update(np.zeros((2, 0), dtype=np.int32), bits).digest() == EMPTY
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    x = np.array([[lo, hi, -1, 0, 1]], dtype=np.int32)
    want = packed(x, bits)
    if bits in (12, 20):
        B = sample_bytes(bits)
        assert want[B - 1] & 0xF8 == 0xF8 and want[3 * B - 1] == 0xFF          # the sign fills the top byte
    assert digest(x, bits) == hashlib.md5(want).digest()


# ---- 2. pieces ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,bits", [(1, 8), (2, 12), (3, 20), (8, 16), (2, 24)])
def test_uneven_pieces_give_the_one_piece_digest(G, bits):
    from elementary_amd.runtime import FlacInMd5
    n = 5 * 256 + 101
    x = codes_of(G, n, bits, seed=2)
    h, at = FlacInMd5(), 0
    for m in (1, 37, 350, 0, n):
        m = min(m, n - at)
        h.update(x[:, at:at + m], bits)
        at += m
        assert h.digest() == hashlib.md5(packed(x[:, :at], bits)).digest()        # (a digest in between leaves the record as it was)
    assert at == n and h.digest() == digest(x, bits)


def test_the_delivery_twin_gives_the_same_digest_where_both_apply():
    from elementary_amd.runtime import FlacMd5
    for bits in (16, 24):
        x = codes_of(2, 777, bits, seed=3)
        assert FlacMd5().update(x, bits).digest() == digest(x, bits)


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments():
    from elementary_amd.runtime import ElemHipError, FlacInMd5, FlacMd5
    for codes, bits in ((np.zeros((1, 4), dtype=np.int32), 32), (np.zeros((0, 4), dtype=np.int32), 16), (np.zeros((9, 4), dtype=np.int32), 16)):
        with pytest.raises(ElemHipError) as e:
            FlacInMd5().update(codes, bits)
        assert e.value.code == 8
    # the delivery side stays as it is: 16 and 24 bits only
    for bits in (8, 12, 20):
        with pytest.raises(ElemHipError):
            FlacMd5().update(np.zeros((1, 4), dtype=np.int32), bits)


# ---- 4. a dry handle ----------------------------------------------------------------------------------------------------------------------
def test_option_values_and_slots_on_a_dry_handle():
    from elementary_amd.runtime import ElemHipError, Runtime
    dry = Runtime(44100.0, 64, device=-1)
    for good in (1, 0, 1.0):
        dry.set_option("flac_in_md5", good)
    for bad in (2, 0.5, -1):
        with pytest.raises(ElemHipError) as e:
            dry.set_option("flac_in_md5", bad)
        assert e.value.code == 6
    assert dry.flac_in_md5() == {"state": [], "md5": [], "hashed": []}
    dry.flac_in_md5_reset()
    assert dry.flac_in_md5() == {"state": [], "md5": [], "hashed": []}


def test_verdicts():
    from elementary_amd.runtime import flac_md5_verdict
    d = hashlib.md5(b"x").digest()
    assert flac_md5_verdict(2, d, d) == "ok" and flac_md5_verdict(2, d, bytes(16)) == "absent" and flac_md5_verdict(1, bytes(16), d) == "incomplete"
    assert flac_md5_verdict(3, bytes(16), d) == "incomplete" and flac_md5_verdict(2, d, d[::-1]) == "mismatch"


@pytest.mark.parametrize("bits", [12, 24])
def test_a_resource_digest_through_the_dry_loader(tmp_path, bits):
    """The scalar path of a handle without a device hashes a FLAC resource under the device path's rule: the whole stream leaves the
    file's digest, a part of it leaves "incomplete", and without the option nothing is hashed."""
    import flac_writer as fw
    from elementary_amd.flac import FlacReader
    from elementary_amd.runtime import Runtime
    chans = [fw._noise(3 * 64 + 17, bits, 5 + c, amp=0.9) for c in range(2)]
    path = tmp_path / "r.flac"
    path.write_bytes(fw.file_bytes(fw.write_stream(chans, bits, 64), bits, 2, 64, len(chans[0])))
    want = hashlib.md5(packed(chans, bits)).digest()
    rd = FlacReader(str(path))
    dry = Runtime(44100.0, 64, device=-1)
    assert dry.add_shared_resource_pcm("off", rd.read(rd.frames))
    assert dry.shared_resource_md5("off") == {"state": 0, "md5": bytes(16)}
    dry.set_option("flac_in_md5", 1)
    rd.seek(0)
    assert dry.add_shared_resource_pcm("whole", rd.read(rd.frames))
    assert dry.shared_resource_md5("whole") == {"state": 2, "md5": want}
    rd.seek(0)
    assert dry.add_shared_resource_pcm("part", rd.read(100))
    assert dry.shared_resource_md5("part") == {"state": 1, "md5": bytes(16)}
    assert np.array_equal(dry.shared_resource_read("whole"), dry.shared_resource_read("off"))


# ---- 5. the kernel's schedule, lane by lane, compiled for the host ---------------------------------------------------------------------------
def _build_and_run(workdir, name, extra):
    import json
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++")) if c and os.path.exists(c)), None)
    assert cxx, "a C++17 compiler builds the host emulation"
    exe = os.path.join(str(workdir), name)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", *extra, "-I", os.path.join(root, "elementary_amd", "csrc"),
                    os.path.join(root, "tests", "native", "flac_in_md5_host.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-3000:])
    return json.loads(res.stdout.strip().splitlines()[-1]), res.stderr


def _check_emulation(out):
    # 5 sample sizes x 4 channel counts x 2 frame sizes x 4 set lengths; sets that cut frames decode the boundary frame twice
    assert out["ok"] and out["failures"] == 0 and out["cases"] == 5 * 4 * 2 * 4 == out["gaps"], out
    assert out["decoded_twice"] > out["cases"]


def test_lane_walk_of_the_jobs_equals_the_twin_and_rfc1321(tmp_path):
    _check_emulation(_build_and_run(tmp_path, "flac_in_md5_host", [])[0])


def test_lane_walk_under_the_sanitizers(tmp_path):
    out, err = _build_and_run(tmp_path, "flac_in_md5_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]
    _check_emulation(out)
