"""Instruction census of the recurrence loops of a specialised island kernel, without a GPU: builds a benchmark graph's plan on a dry
engine (the run-time compiler cross-compiles its shapes for gfx950 into a kernel cache of this run's own), disassembles every code
object with llvm-objdump and prints, per recurrence loop, the instruction mix of a steady 16-frame group: chain VALU, loads, waits,
register moves, scalar instructions, stores.

A recurrence store stands inside an EXEC switch (island_ops.inc: chain_store_window, chain_store_group): scalar move from EXEC, scalar
move to EXEC, the stores, scalar move back. The stores of one switch are a cluster; their immediates tell the loop: 64 bytes apart (or
a single store) is the quad-skewed loop with a window of that many groups, 16 bytes apart the four pieces of one group of the generic
loop. A run is what stands between two consecutive clusters, the closing cluster included, whatever it is: a loop's back edge and its
counter are part of it. Consecutive runs of one kind and window, with the same number of VALU instructions per group give
or take two (or 6 %; the generic loop's groups are software-pipelined across its clusters and are not told apart this way), form a loop; a run with anything else in it (LDS traffic of the task dispatch, a barrier) ends the loop and
falls out, and so does the head before a loop's first cluster. The steady runs of a loop are
those with the full number of loads (the last span of a streamed loop issues none). It counts instruction classes by mnemonic and
nothing else.

Usage: python tools/chain_loop_census.py [c2|c4] [--json]"""
import os as _os, sys as _sys; _R = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))); _sys.path[:0] = [_R, _os.path.join(_R, 'tests')]
import collections
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM_BIN = ("/opt/rocm/lib/llvm/bin", "/opt/rocm/llvm/bin")
CLASSES = ("valu", "load", "wait", "move", "scalar", "store", "other")


def llvm_tool(name):
    for d in LLVM_BIN:
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


def classify(mnemonic):
    m = mnemonic
    if m.startswith("s_waitcnt"):
        return "wait"
    if m.startswith("s_"):
        return "scalar"
    if m.startswith(("buffer_store", "global_store", "flat_store", "scratch_store", "ds_write")):
        return "store"
    if m.startswith(("buffer_load", "global_load", "flat_load", "scratch_load", "ds_read")):
        return "load"
    if m.startswith(("v_mov_b32", "v_mov_b64", "v_accvgpr")) and "dpp" not in m:
        return "move"
    if m.startswith("v_"):
        return "valu"
    return "other"


_INSN = re.compile(r"^\s+([a-z_0-9]+)\s*(.*?)\s*//")


def instructions(disassembly):
    """[(mnemonic, operands)] of a code object's disassembly, in text order."""
    out = []
    for line in disassembly.splitlines():
        m = _INSN.match(line)
        if m:
            out.append((m.group(1), m.group(2)))
    return out


def _offset(ops):
    m = re.search(r"offset:(\d+)", ops)
    return int(m.group(1)) if m else 0


def clusters(ins):
    """The EXEC-switched store clusters: (index of the move from EXEC, index behind the move back, [store immediates])."""
    found, i = [], 0
    while i + 3 < len(ins):
        m0, o0 = ins[i]
        m1, o1 = ins[i + 1]
        if m0 == "s_mov_b64" and o0.endswith(", exec") and m1 == "s_mov_b64" and o1.startswith("exec,"):
            j, offs = i + 2, []
            while j < len(ins) and classify(ins[j][0]) == "store":
                offs.append(_offset(ins[j][1])); j += 1
            if offs and j < len(ins) and ins[j][0] == "s_mov_b64" and ins[j][1].startswith("exec,"):
                j += 1
                if j < len(ins) and ins[j][0] == "s_nop":
                    j += 1
                found.append((i, j, offs))
                i = j
                continue
        i += 1
    return found


def census(disassembly):
    """The recurrence loops of one code object: a list of dicts (kind, window, steady runs, per-group class means)."""
    ins = instructions(disassembly)
    cl = clusters(ins)
    loops, cur = [], None                   # a loop: consecutive runs of one kind and window with nothing but the loop's classes in them
    for (_a0, b0, _o0), (_a1, b1, offs) in zip(cl, cl[1:]):
        strides = {y - x for x, y in zip(offs, offs[1:])}
        if len(offs) == 1 or strides == {64}:
            key = ("quad", len(offs))
        elif strides == {16} and len(offs) == 4:
            key = ("generic", 1)
        else:
            key = None
        counts = collections.Counter(classify(m) for m, _ in ins[b0:b1])
        if key is None or counts["other"]:
            cur = None
            continue
        valu = counts["valu"] / key[1]       # per group; the scheduler moves a step or two across a cluster, another task's loop differs by more
        if cur is None or cur[0] != key or (key[0] == "quad" and abs(valu - cur[2]) > max(2.0, 0.06 * cur[2])):
            cur = (key, [], valu)
            loops.append(cur)
        cur[1].append(counts)
    out = []
    for (kind, groups), rs, _valu in loops:
        most = max(r["load"] for r in rs)
        steady = [r for r in rs if r["load"] == most]     # (the last span of a streamed loop issues no loads: fewer instructions, not more)
        if len(rs) < 2:
            continue
        per = {c: sum(r[c] for r in steady) / (len(steady) * groups) for c in CLASSES if c != "other"}
        out.append({"kind": kind, "window": groups if kind == "quad" else None, "runs": len(steady), "edge_runs": len(rs) - len(steady),
                    "streams": most / (4.0 * groups), "per_group": per, "total_per_group": sum(per.values())})
    return out


def resources(path):
    """VGPRs, scratch bytes per lane and .text bytes of a code object."""
    notes = subprocess.run([llvm_tool("llvm-readelf"), "--notes", path], capture_output=True, text=True, check=True).stdout
    sections = subprocess.run([llvm_tool("llvm-readelf"), "-S", path], capture_output=True, text=True, check=True).stdout
    vg = re.search(r"\.vgpr_count:\s*(\d+)", notes)
    sc = re.search(r"\.private_segment_fixed_size:\s*(\d+)", notes)
    tx = re.search(r"\.text\s+PROGBITS\s+[0-9a-f]+\s+[0-9a-f]+\s+([0-9a-f]+)", sections)
    return {"vgprs": int(vg.group(1)) if vg else None, "scratch": int(sc.group(1)) if sc else None, "text_bytes": int(tx.group(1), 16) if tx else None}


def disassemble(path):
    return subprocess.run([llvm_tool("llvm-objdump"), "-d", "--mcpu=gfx950", path], capture_output=True, text=True, check=True).stdout


def build_shapes(which, cache_dir):
    """Render the graph on a dry engine with the kernel cache at cache_dir; returns the code objects it left there."""
    os.environ["ELEMHIP_KCACHE"] = cache_dir          # read when the library's run-time compiler starts: set before it is loaded
    import torch  # noqa: F401  (first, as every process that loads the engine does)
    from elementary_amd import graphs
    from elementary_amd.runtime import Runtime
    if which == "c2":
        sr, roots = graphs.C2_SAMPLE_RATE, graphs.c2_graph(voices=8)
    elif which == "c4":
        sr, roots = graphs.C4_SAMPLE_RATE, [graphs.c4_instance(k) for k in range(128)]
    else:
        raise SystemExit(f"unknown graph {which!r}: c2 or c4")
    rt = Runtime(sr, 512, device=-1)
    rt.set_option("specialize", 2)
    assert rt.render(*roots)["result"] == 0
    st = rt.stats()
    for k in range(st["spec_shapes"]):
        info = rt.spec_info(k)
        assert info["state"] == 1, info["log"][:2000]
    return sorted(glob.glob(os.path.join(cache_dir, "*.hsaco")))


def report(which, cache_dir):
    shapes = []
    for path in build_shapes(which, cache_dir):
        shapes.append({"code_object": os.path.basename(path), **resources(path), "loops": census(disassemble(path))})
    return {"graph": which, "shapes": shapes}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    which = args[0] if args else "c2"
    with tempfile.TemporaryDirectory(prefix="elemhip_census_") as tmp:
        os.chmod(tmp, 0o700)
        rep = report(which, tmp)
    if "--json" in sys.argv:
        print(json.dumps(rep))
        return
    for s in rep["shapes"]:
        print(f"{which} {s['code_object']}: {s['vgprs']} VGPRs, scratch {s['scratch']} bytes/lane, .text {s['text_bytes']} bytes")
        for lp in s["loops"]:
            per = lp["per_group"]
            what = f"quad-skewed, window {lp['window']}" if lp["kind"] == "quad" else "generic (four stores per group)"
            print(f"  {what}, {lp['streams']:g} streamed operand(s), {lp['runs']} steady runs: {lp['total_per_group']:.2f} instructions per 16-frame group = "
                  + ", ".join(f"{per[c]:.2f} {c}" for c in CLASSES if c != "other"))


if __name__ == "__main__":
    main()
