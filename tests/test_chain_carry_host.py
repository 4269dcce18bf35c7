"""The quad-skewed recurrence loop without its tail, without a GPU: tests/native/chain_carry_host.cpp emulates 64 lanes with the index
arithmetic of elementary_amd/csrc/chain_skew.h — no loads and no steps behind the last group, every lane takes the carried
registers of the first lane of its quad — for every task size 1 .. 16 at blocks of 64, 128, 192 and 512 frames, three blocks in a
row, against the plain serial loop. The same program once more under the address and undefined-behaviour sanitizers."""
import json
import os
import subprocess

from test_chain_skew_host import ROOT, _cxx


def _build_and_run(workdir, name, extra):
    cxx = _cxx()
    assert cxx, "a C++17 compiler builds the host emulation"
    exe = os.path.join(str(workdir), name)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "elementary_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "chain_carry_host.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(res.stdout.strip())
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-3000:])
    return json.loads(res.stdout.strip().splitlines()[-1]), res.stderr


def test_broadcast_leaves_every_lane_with_the_serial_final_state(tmp_path):
    """Frames written once with the serial loop's bits, load offsets inside [0, 4n - 16] and none behind the last group, every lane at
    the serial final state after the broadcast, mirror lanes unchanged by it: 4 block sizes x 16 task sizes x 3 blocks."""
    out, _ = _build_and_run(tmp_path, "chain_carry_host", [])
    assert out["ok"] and out["failures"] == 0 and out["cases"] == 64, out
    assert out["clamped_loads"] > 0 and out["stores"] > 0, out        # the head's clamp was exercised
    assert out["short_lanes"] > 0 and out["mirror_lanes"] > 0, out    # lanes that needed the broadcast, and lanes it must not change


def test_broadcast_emulation_is_clean_under_asan_and_ubsan(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined: an index of the schedule that left a buffer would stop it."""
    out, err = _build_and_run(tmp_path, "chain_carry_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert out["ok"] and out["failures"] == 0, out
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]


def test_the_kernel_broadcasts_what_the_header_names():
    """The loop takes the DPP control of its broadcast from the header and runs no tail."""
    ops = open(os.path.join(ROOT, "elementary_amd", "csrc", "island_ops.inc")).read()
    loop = ops[ops.index("void chain_loop_q("):ops.index("void chain_loop_d(")]
    assert "chain_skew::kStateQuadPerm" in ops and "step.each(" in loop
    assert "kTailSteps" not in loop and "load_edge(n /" not in loop
