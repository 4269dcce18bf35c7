"""Breakpoint automation, timed: a C4-style render (128 instances of the C4 chain, instance k scaled by engine input k mod K) whose K
control channels are automation lanes (elemhip_automation_set: a dozen breakpoints each, expanded on the GPU) against the same render on
the same build fed the dense float32 control signals as K planar inputs through elemhip_process_blocks_host. One process, one engine
per leg, the same frames and sample times in every round (the outputs are compared once: the same bits); 3 warm-up calls, then 12 timed
rounds in which the legs ALTERNATE, so drift of the shared host falls on both alike; a host clock around calls that end in a device
synchronise. Reported per K: both legs' median, min and max in ms and the lanes' median as a ratio to the dense leg's. `--out FILE`
also writes the report there; `--lanes-only` renders a few lane-fed calls and nothing else, for a kernel trace of its own."""
import sys, time; sys.path.insert(0, '.')
import numpy as np
from elementary_amd import el, graphs
from elementary_amd.runtime import Runtime, automation_host, automation_launches

lanes_only = "--lanes-only" in sys.argv
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
WARM, ROUNDS, BS, INST, BATCH, SETS = 3, 12, 512, 128, 1024, 2
FRAMES = SETS * BATCH * BS
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def lane(c):
    """Twelve breakpoints over the call: ramps and steps between 0.2 and 1."""
    rng = np.random.default_rng(100 + c)
    at = np.sort(rng.choice(FRAMES, size=12, replace=False))
    return [(int(f), float(0.2 + 0.8 * rng.random()), int(k % 3 != 2)) for k, f in enumerate(at)]


def workload(K):
    roots = [el.mul(graphs.c4_instance(k), el.in_({"channel": k % K})) for k in range(INST)]
    lanes = {c: lane(c) for c in range(K)}

    def engine(with_lanes):
        rt = Runtime(graphs.C4_SAMPLE_RATE, BS, device=0); rt.set_option("specialize", 2); rt.set_option("batch_blocks", BATCH)
        assert rt.render(*roots)["result"] == 0
        rt.process_blocks_host(np.zeros((K, 64 * BS), dtype=np.float32), INST, 64 * BS, sample_time=-64 * BS)      # root fades settle
        for c, p in (lanes if with_lanes else {}).items():
            rt.automation(c, p)
        return rt

    a = engine(True)
    if lanes_only:
        for _ in range(3):
            a.process_blocks_host(None, INST, FRAMES, sample_time=0)
        return
    d = engine(False)
    dense = np.stack([automation_host(lanes[c], 0, FRAMES) for c in range(K)])
    out = {k: np.empty((INST, FRAMES), dtype=np.float32) for k in ("lanes", "dense")}
    calls = {"dense": lambda: d.process_blocks_host(dense, INST, FRAMES, out=out["dense"], sample_time=0),
             "lanes": lambda: a.process_blocks_host(None, INST, FRAMES, out=out["lanes"], sample_time=0)}
    # (the C4 chains carry state, so the legs are compared call by call: both engines have rendered the same history)
    n0 = automation_launches()
    for _ in range(WARM):
        for fn in calls.values():
            fn()
        assert np.array_equal(out["lanes"].view(np.uint32), out["dense"].view(np.uint32)), "the lane leg and the dense leg differ"
    ts = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, fn in calls.items():
            t0 = time.perf_counter(); fn(); ts[k].append(time.perf_counter() - t0)
    assert np.array_equal(out["lanes"].view(np.uint32), out["dense"].view(np.uint32)), "the lane leg and the dense leg differ"
    base = float(np.median(ts["dense"]))
    say(f"K = {K}: {INST} C4 instances x input k mod {K}, {FRAMES} frames per call ({SETS} sets of {BATCH} blocks of {BS}), {WARM} warm-up calls, "
        f"{ROUNDS} timed rounds, legs alternating; {automation_launches() - n0} automation launches")
    mb = {"dense": 4.0 * K * FRAMES / 1e6, "lanes": 0.0}
    for k, v in ts.items():
        med = float(np.median(v))
        say(f"  {k + ' input':12s} {mb[k]:8.1f} MB of control in per call   median {1e3 * med:8.3f} ms   min {1e3 * min(v):8.3f}   max {1e3 * max(v):8.3f}"
            f"   median / dense {med / base:5.3f}")
    a.close(); d.close()


for K in ((8,) if lanes_only else (1, 8, 32)):
    workload(K)
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
