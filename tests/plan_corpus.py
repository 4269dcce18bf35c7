"""A fixed corpus of graphs, planned on dry handles, and the `program_digest` of each plan (Engine::describePlan: a hash
over island headers, program blobs, level / convolve / root / tap tables and specialised-kernel texts).

`digests()` returns {name: digest}; tests/golden/plan_digests.json holds the recorded ones and
test_host_logic.py::test_planner_output_is_pinned compares the two, so a refactor of the planner is held to "not one bit of
any plan moves". A change that alters plans ON PURPOSE re-records the file with

    python tests/plan_corpus.py

and the diff of the JSON shows which graphs moved. That is the intended use.

The corpus is what the planner tests of test_host_logic.py already build. Not in it: a graph with a call-out node type (no
Python test outside the GPU suite registers one; the facade test drives a native host program).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE, os.path.join(ROOT, "benchmarks")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = os.path.join(HERE, "golden", "plan_digests.json")


def _dry(sr, bs=512, **opts):
    from elementary_amd.runtime import Runtime
    rt = Runtime(sr, bs, device=-1)
    for k, v in opts.items():
        rt.set_option(k, v)
    return rt


def _digest(rt):
    return rt.describe_plan()["program_digest"]


def _render(rt, *roots):
    assert rt.render(*roots)["result"] == 0
    return _digest(rt)


def digests():
    import numpy as np
    import bench_configs as B
    from cases import NODE_CASES, node_case_resources
    from elementary_amd import el, graphs
    out = {}

    # every node case: in a handle of its own, and all of them in ONE handle in sorted order (twins across cases; the comparing
    # cache mode and the specialised texts, as test_relocated_programs_in_verify_mode builds them)
    one = _dry(44100.0, specialize=2, plan_cache=2)
    for name, data in node_case_resources().items():
        assert one.add_shared_resource(name, data)
    for name in sorted(NODE_CASES):
        rt = _dry(44100.0)
        for rname, data in node_case_resources().items():
            assert rt.add_shared_resource(rname, data)
        out["node/" + name] = _render(rt, *NODE_CASES[name][0]())
        out["node_one_handle/" + name] = _render(one, *NODE_CASES[name][0]())

    # C2: 16 and 48 voices one after the other in a handle, 256 voices, 300 voices lane-packed
    rt = _dry(graphs.C2_SAMPLE_RATE, specialize=2, plan_cache=2)
    for v in (16, 48):
        out["c2/%d" % v] = _render(rt, *graphs.c2_graph(voices=v))
    out["c2/256"] = _render(_dry(graphs.C2_SAMPLE_RATE), *graphs.c2_graph())
    out["c2/300_cu150"] = _render(_dry(graphs.C2_SAMPLE_RATE, specialize=2, plan_cache=2, cu_count=150), *graphs.c2_graph(voices=300))
    for key, val in (("merge_phases", 0), ("fuse_svf_coef", 0), ("fuse_svf_coef", 1), ("mixer_split", 1), ("mixer_split", 4),
                     ("pipeline_copies", 1), ("pipeline_copies", 6)):
        out["c2/16_%s_%d" % (key, val)] = _render(_dry(graphs.C2_SAMPLE_RATE, **{key: val}), *graphs.c2_graph(voices=16))

    # C4 render jobs: packed across roots, and with defaults
    out["c4/96_pack_roots_cu32"] = _render(_dry(graphs.C4_SAMPLE_RATE, specialize=2, plan_cache=2, pack_roots=1, cu_count=32),
                                           *[graphs.c4_instance(k) for k in range(96)])
    out["c4/128"] = _render(_dry(graphs.C4_SAMPLE_RATE), *[graphs.c4_instance(k) for k in range(128)])

    # C1, and C3 with its impulse responses as shared resources
    out["c1"] = _render(_dry(graphs.C1_SAMPLE_RATE), *graphs.c1_graph())
    rt = _dry(graphs.C3_SAMPLE_RATE)
    for ch in range(graphs.C3_CHANNELS):
        assert rt.add_shared_resource("ir%d" % ch, graphs.c3_impulse_response(ch))
    out["c3"] = _render(rt, *graphs.c3_graph())

    # the C5 mutation stream (one voice of 128 replaced per batch), once per cache mode
    texts, _, _ = B._c5_batches(128, 24)
    for mode in (0, 1, 2):
        rt = _dry(graphs.C2_SAMPLE_RATE, plan_cache=mode, specialize=2)
        for i, t in enumerate(texts):
            assert rt.apply_instructions_json(t) == 0
            if i % 16 == 15:
                rt.gc()
        out["c5/plan_cache_%d" % mode] = _digest(rt)

    # a tap loop, and the block sizes above one LDS slot
    def loop():
        return el.tapOut({"name": "fb"}, el.add(el.in_({"channel": 0}), el.mul(0.5, el.tapIn({"name": "fb"}))))
    for bs in (512, 1024, 2048, 32768, 700, 1000, 1023, 514, 521, 1031):
        rt = _dry(48000.0, bs)
        out["bs%d/cycle" % bs] = _render(rt, el.mul(0.5, el.cycle(220.0)))
        out["bs%d/tap_loop" % bs] = _render(rt, loop())
        out["bs%d/cycle_again" % bs] = _render(rt, el.mul(0.25, el.cycle(330.0)))

    # deep and wide
    x = el.in_({"channel": 0})
    for k in range(300):
        x = el.pole(0.5, el.mul(0.5, x))
    out["deep_300"] = _render(_dry(44100.0), x)
    out["wide_500"] = _render(_dry(44100.0), el.add(*[el.cycle(100.0 + k) for k in range(500)]))

    # a multi-output node: one plan entry per channel
    rt = _dry(44100.0)
    assert rt.add_shared_resource("/v/stereo", np.asarray([[27, 27, 27], [15, 15, 15]], np.float32))
    out["mc_table"] = _render(rt, el.add(*el.mc.table({"path": "/v/stereo", "channels": 3}, 0)))
    return out


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(path, "w") as f:
        json.dump(digests(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)
