"""Instruction census of the quad-skewed recurrence loops of the C2 voice kernel, on the CPU: tools/chain_loop_census.py builds the
voice shape on a dry engine, the run-time compiler cross-compiles it for gfx950, and the tool counts the instruction classes of a
steady 16-frame group in the disassembly. A lone recurrence wave pays per instruction issued (DESIGN_LOG §3.4), so the count is the
loop's cost model: the chain's own 32 VALU, four loads per streamed operand, ONE wait, ONE store, and the EXEC switch around the
stores shared by the W groups of a window — no register copies, no wait per 16-byte piece.

Figures when this test was written (profiles/r09/chain_loop_census.txt), W = 4 in both loops:
  pole loop   39.00 per group = 32 VALU + 4 loads + 1 wait + 1 store + 1.00 scalar; bound 39. Parent: 44.9 over the block, 47 inside a span.
  phase loop  34.00 per group = 32 VALU + 1 store + 1.00 scalar; bound 34. Parent: 38.0 (37 inside a span).
The phase loop has no streamed operand; as a loop around its 64-frame spans it counted 35.00, one scalar instruction per group for
its counter and back edge, which the bound 32 + 1 + 4 / W has no room for. Its step is two VALU ops per frame (ChainStep::kShort), and
such a loop is written out span by span as the streamed one is: 2.7 KB of code."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import chain_loop_census as census  # noqa: E402


@pytest.fixture(scope="module")
def voice_loops():
    if not census.llvm_tool("llvm-objdump") or not census.llvm_tool("llvm-readelf"):
        pytest.skip("llvm-objdump / llvm-readelf disassemble the code object")
    if not os.path.exists(os.path.join(ROOT, "elementary_amd", "elemhip_jitc")) or not shutil.which("hipcc"):
        pytest.skip("the run-time compiler's helper cross-compiles the shape")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "chain_loop_census.py"), "c2", "--json"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    rep = json.loads(res.stdout.strip().splitlines()[-1])
    voice = [s for s in rep["shapes"] if any(lp["kind"] == "quad" and lp["streams"] == 1 for lp in s["loops"])]
    assert len(voice) == 1, rep
    for lp in voice[0]["loops"]:
        print(lp)
    return voice[0]


def test_the_voice_kernel_keeps_out_of_scratch(voice_loops):
    assert voice_loops["scratch"] == 0 and voice_loops["vgprs"] <= 256, voice_loops


def test_pole_loop_census(voice_loops):
    """One streamed operand: 32 chain VALU + 4 loads + 1 wait + 1 store + 4 / W for the EXEC switch, and no register copy."""
    pole = [lp for lp in voice_loops["loops"] if lp["kind"] == "quad" and lp["streams"] == 1]
    assert len(pole) == 1 and pole[0]["runs"] >= 2, voice_loops["loops"]
    lp, w = pole[0], pole[0]["window"]
    print(f"pole loop, window {w}: {lp['total_per_group']:.2f} instructions per group {lp['per_group']}")
    assert lp["per_group"]["move"] == 0, lp
    assert lp["per_group"]["wait"] <= 1, lp
    assert lp["total_per_group"] <= 32 + 4 + 1 + 1 + 4 / w, lp


def test_phase_loop_census(voice_loops):
    """No streamed operand: 32 chain VALU + 1 store + 4 / W."""
    plain = [lp for lp in voice_loops["loops"] if lp["kind"] == "quad" and lp["streams"] == 0]
    assert plain, voice_loops["loops"]
    lp = min(plain, key=lambda q: q["per_group"]["valu"])         # the merged phase task: two VALU per frame
    w = lp["window"]
    print(f"phase loop, window {w}: {lp['total_per_group']:.2f} instructions per group {lp['per_group']}")
    assert 31.5 <= lp["per_group"]["valu"] <= 32.5, lp
    assert lp["per_group"]["move"] == 0 and lp["per_group"]["wait"] == 0, lp
    assert lp["total_per_group"] <= 32 + 1 + 4 / w, lp
