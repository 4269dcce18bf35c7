"""The store windows of the quad-skewed recurrence loop without a GPU: elementary_amd/csrc/chain_skew.h states which group of a span
closes a window and which stores it carries, island_ops.inc chain_loop_q issues them under one EXEC switch, and
tests/native/chain_window_host.cpp emulates the loop with the header's functions — 64 lanes, blocks of 64, 128, 192 and 512 frames,
tasks of 1, 3 and 16 members, spans of 2, 4 and 8 groups and every window size that fits them, against the unwindowed schedule and
the plain serial loop. The same program once more under the address and undefined-behaviour sanitizers."""
import json
import os
import shutil
import subprocess

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
                    os.path.join(ROOT, "tests", "native", "chain_window_host.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(res.stdout.strip())
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-3000:])
    return json.loads(res.stdout.strip().splitlines()[-1]), res.stderr


# blocks of 64 and 192 frames hold spans of 2 and 4 groups (2 + 3 window sizes), 128 and 512 also spans of 8 (+ 4): 28 per member count
CASES = 3 * 28


def test_windowed_stores_are_the_unwindowed_schedule_s_bytes(tmp_path):
    """Every frame stored exactly once with the bytes and at the offset of the unwindowed schedule (and of the serial loop), no window
    stored before its last group's steps, none across two spans, none left open at the end of a block."""
    out, _ = _build_and_run(tmp_path, "chain_window_host", [])
    assert out["ok"] and out["failures"] == 0 and out["cases"] == CASES, out
    assert out["switches"] < out["stores"], out          # windows wider than one group were exercised


def test_window_emulation_is_clean_under_asan_and_ubsan(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined: a store offset that left the block buffer would stop it."""
    out, err = _build_and_run(tmp_path, "chain_window_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert out["ok"] and out["failures"] == 0 and out["cases"] == CASES, out
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]


def test_the_loop_takes_its_windows_from_the_header():
    ops = open(os.path.join(ROOT, "elementary_amd", "csrc", "island_ops.inc")).read()
    for call in ("chain_skew::window(", "chain_skew::window_fits(", "chain_skew::window_closes(", "chain_skew::window_first("):
        assert call in ops, call
