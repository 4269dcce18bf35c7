"""PCM delivery without a GPU: elementary_amd/csrc/pcm_pack.h — the header the pack kernel (pcm_pack.hip) takes its arithmetic and every
index from — compiled for the host and driven by tests/native/pcm_pack_host.cpp: the kernel's three stages emulated thread by thread
over block sizes 32, 341, 350 and 512, G = 1, 2, 3, 6 and 8, the three formats, sets of 1 and 3 blocks, whole and cut at 37 frames of
the last block, against a plain scalar loop; the same program once more under the address and undefined-behaviour sanitizers; and
the codes it prints for an edge vector and for 4096 dithered samples around t = 2^32 against the numpy restatement
(tests/pcm_reference.py), which was not derived from the header."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import pcm_reference as ref

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
                    os.path.join(ROOT, "tests", "native", "pcm_pack_host.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-3000:])
    return json.loads(res.stdout.strip().splitlines()[-1]), res.stderr


@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("pcm"), "pcm_pack_host", [])[0]


def test_lane_schedule_writes_every_byte_once_with_the_scalar_loops_bits(emulation):
    out = emulation
    print({k: v for k, v in out.items() if not isinstance(v, list)})
    assert out["ok"] and out["failures"] == 0 and out["cases"] == 4 * 5 * 3 * 2 * 2 + 2, out["cases"]
    # whole 16-byte pieces leave as 16-byte stores; the narrow ones are the pieces tiles share (odd block sizes, 3-byte samples)
    assert out["wide_stores"] > 0 and out["narrow_stores"] > 0 and out["wide_stores"] > 20 * out["narrow_stores"], out["wide_stores"]
    assert out["wide_loads"] > 0 and out["narrow_loads"] > 0
    # the transposed read of the skewed LDS rows: no half-wave hits a bank twice, for the groups run and for every group up to 32
    assert out["half_wave_reads"] > 0 and out["bank_conflicts"] == 0 and out["skew_conflicts"] == 0


def test_edge_vector_meets_the_table_and_the_reference(emulation):
    x = np.array([row[0] for row in ref.EDGE_TABLE], dtype=np.float32)
    zero = np.zeros(len(x), np.float32)
    for bits, key, col in ((16, "edge_s16", 1), (24, "edge_s24", 2)):
        want = [row[col] for row in ref.EDGE_TABLE]
        assert ref.quant(x, bits, zero).tolist() == want          # the restatement meets the table ...
        assert emulation[key] == want                              # ... and so does the header


def test_dithered_samples_across_2_pow_32_equal_the_reference(emulation):
    i = np.arange(4096, dtype=np.int64)
    x = (((37 * i) % 201 - 100).astype(np.float32) / np.float32(128.0)).astype(np.float32)
    d = ref.dither(12345, 3, (np.int64(1) << np.int64(32)) - 2048 + i)
    assert float(np.abs(d).max()) < 1.0 and abs(float(d.var()) - 1.0 / 6.0) < 0.02            # TPDF, 2 LSB peak to peak
    for bits in (16, 24):
        got = np.array(emulation[f"dither_s{bits}"], dtype=np.int32)
        assert np.array_equal(got, ref.quant(x, bits, d)), int((got != ref.quant(x, bits, d)).sum())
        assert not np.array_equal(got, ref.quant(x, bits, np.zeros(4096, np.float32)))         # (the dither is on)


def test_emulation_is_clean_under_asan_and_ubsan(tmp_path):
    out, err = _build_and_run(tmp_path, "pcm_pack_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert out["ok"] and out["failures"] == 0, out["failures"]
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]


def test_the_kernel_takes_its_indices_from_the_header():
    hip = open(os.path.join(CSRC, "pcm_pack.hip")).read()
    for call in ("pp::tile_valid(", "pp::tile_frames(", "pp::row_chunks(", "pp::quad_first(", "pp::quad_whole(", "pp::stats_fold(", "pp::dither_lo(",
                 "pp::encode(", "pp::stretch_begin(", "pp::image_head(", "pp::image_offset(", "pp::piece_count(", "pp::piece_whole(", "pp::store_unit(",
                 "pp::lds_image_offset(", "pp::row_bases("):
        assert call in hip, call
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "pcm_pack.h" in mk and "pcm_pack.o" in mk
