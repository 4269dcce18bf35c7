"""The lane schedule of the quad-skewed recurrence loop without a GPU: elementary_amd/csrc/chain_skew.h, the header the specialised
kernels' loop takes every index from (island_ops.inc chain_loop_q), compiled for the host and run by tests/native/chain_skew_host.cpp
— 64 emulated lanes, blocks of 64, 128, 192 and 512 frames, tasks of 1, 3 and 16 members, a one-pole with random input against the
plain serial loop (no contraction). The same program once more under the address and undefined-behaviour sanitizers."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++")):
        if c and os.path.exists(c):
            return c
    return None


def _build_and_run(workdir, name, extra):
    cxx = _cxx()
    assert cxx, "a C++17 compiler builds the host emulation"
    exe = os.path.join(str(workdir), name)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "elementary_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "chain_skew_host.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(res.stdout.strip())
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-3000:])
    return json.loads(res.stdout.strip().splitlines()[-1]), res.stderr


def test_skewed_loop_matches_the_serial_loop_bit_for_bit(tmp_path):
    """Every frame written exactly once with the serial loop's bits, every lane of a member left with the serial final state, no load
    offset outside [0, 4n - 16], a task of 17 members refused: for n in {64, 128, 192, 512} x count in {1, 3, 16}."""
    out, _ = _build_and_run(tmp_path, "chain_skew_host", [])
    assert out["ok"] and out["failures"] == 0 and out["cases"] == 12, out
    assert out["clamped_loads"] > 0 and out["stores"] > 0, out       # the head and tail clamps were exercised


def test_skewed_loop_emulation_is_clean_under_asan_and_ubsan(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined: an index of the schedule that left a buffer would stop it."""
    out, err = _build_and_run(tmp_path, "chain_skew_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert out["ok"] and out["failures"] == 0, out
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]


def test_the_kernel_text_takes_its_indices_from_the_header():
    """One copy of the formulas: the run-time compiled text carries chain_skew.h, and the loop calls it for the lane mapping, the
    predicates and the offsets."""
    csrc = os.path.join(ROOT, "elementary_amd", "csrc")
    ops = open(os.path.join(csrc, "island_ops.inc")).read()
    spec = open(os.path.join(csrc, "island_spec.inc")).read()
    for call in ("chain_skew::lane_skew(", "chain_skew::store_bias(", "chain_skew::load_bias(", "chain_skew::load_offset(", "chain_skew::store_mask(",
                 "chain_skew::head_active(", "chain_skew::tail_active(", "chain_skew::kLoadImmBias"):
        assert call in ops, call
    assert "chain_skew::lane_member(" in spec and "chain_skew::applies(" in spec
    assert "chain_skew.h" in open(os.path.join(csrc, "Makefile")).read()
