"""The C++ restatement (oracle/elem_oracle.cpp) against the unmodified reference engine
(oracle/_ref) on every node case and on the BASELINE graphs: same compiler, same libm, no FMA
contraction on either side, so the two must agree BIT FOR BIT. Where oracle/_ref is not built (it
needs the reference checkout at build time), the restatement is held against the reference engine's
outputs recorded as SHA-256 digests of their bits (tests/golden/reference_digests.json, written by
tests/golden/make_ref_digests.py): the same bit-for-bit comparison."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle
from cases import NODE_CASES, REF_ONLY, node_case_resources, sampleseq_scenario
from edge_cases import EDGE_REF_ONLY, NODE_EDGE_CASES, clock_starts, edge_inputs, edge_resources, edge_roots
from elementary_amd import graphs
from helpers import render_one, render_pair

pytestmark = pytest.mark.skipif(not oracle.have_port(), reason="needs the port (oracle/libelemoracle.so)")
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_digests.json")


def port(sr, bs):
    return oracle.PortRuntime(sr, bs)


def ref(sr, bs):
    return oracle.RefRuntime(sr, bs)


def _numbers_as_floats(x):
    """1 and 1.0 compare equal in Python but print differently in JSON: digest what `==` compares."""
    if isinstance(x, dict):
        return {k: _numbers_as_floats(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_numbers_as_floats(v) for v in x]
    if isinstance(x, int) and not isinstance(x, bool):
        return float(x)
    return x


def digest(x) -> str:
    """SHA-256 of a result's bits: dtype, shape and bytes of an array; the JSON text of anything else."""
    h = hashlib.sha256()
    if isinstance(x, np.ndarray):
        h.update(f"{x.dtype.str}{x.shape}".encode())
        h.update(np.ascontiguousarray(x).tobytes())
    else:
        h.update(json.dumps(_numbers_as_floats(x), sort_keys=True).encode())
    return h.hexdigest()


def _render(makes, roots_fn, **kw):
    """One engine: its output. Two engines (restatement, reference): both outputs, rendered side by side by render_pair, which
    also holds the two render results' instruction batches equal."""
    return render_one(makes[0], roots_fn, **kw) if len(makes) == 1 else render_pair(*makes, roots_fn, **kw)


def _gc(make):
    """gc.test.js:5-43 pattern: nodes of a replaced graph are pruned only after the next rebuild."""
    from elementary_amd import el
    rt = make(44100.0, 512)
    rt.render(el.mul(2, 3))
    for _ in range(4):
        rt.process(None, 1, 512)
    first = rt.gc()
    rt.render(el.mul(3, 4))
    for _ in range(10):
        rt.process(None, 1, 512)
    second = rt.gc()
    rt.render(el.mul(4, 5))
    for _ in range(10):
        rt.process(None, 1, 512)
    third = rt.gc()
    return [sorted(first), sorted(second), sorted(third)]


def _events(make):
    from elementary_amd import el
    from helpers import lcg_noise
    rt = make(44100.0, 128)
    x = el.in_({"channel": 0})
    assert rt.render(el.meter({"name": "in"}, x), el.snapshot({"name": "snap"}, el.train(500.0), el.mul(2, x)),
                     el.meter({}, el.cycle(100.0)),
                     el.scope({"name": "sc", "size": 256, "channels": 2}, x, el.mul(0.5, x), el.mul(0.25, x)))["result"] == 0
    log = []
    for k in range(12):
        rt.process(lcg_noise(128, 5 + k, 0.5)[None, :], 4, 128)
        if k % 3 != 1:                      # skipped relays: only the newest readout survives
            log.append(rt.process_queued_events())
    return log


def _edge(make, name, block=512, blocks=6):
    """One engine over an edge-corpus case (tests/edge_cases.py): 6 blocks of 512 at 44.1 kHz from sample_time 0 — clock_far_out
    from each of its start times, one after the other. Returns [starts * blocks, roots, block]."""
    outs = []
    for start in (clock_starts(block) if name == "clock_far_out" else [0]):
        rt = make(44100.0, block)
        for rname, data in edge_resources().items():
            assert rt.add_shared_resource(rname, data)
        roots = edge_roots(name, block)
        assert rt.render(*roots)["result"] == 0
        outs += [rt.process(edge_inputs(k, block), len(roots), block, sample_time=start + k * block) for k in range(blocks)]
    return np.stack(outs)


EDGE_SCENARIOS = ["edge/" + n for n in sorted(set(NODE_EDGE_CASES) - EDGE_REF_ONLY)]
SCENARIOS = (["node/" + n for n in sorted(set(NODE_CASES) - REF_ONLY)] + ["c1", "c2x64", "c4x6", "gc", "sampleseq32", "sampleseq512", "events"]
             + EDGE_SCENARIOS)


def run_scenario(key, *makes):
    """The result of scenario `key` on each engine of `makes` (one or two); one engine: the result itself, two: a pair."""
    if key.startswith("node/"):
        fn, n_in = NODE_CASES[key[5:]]
        return _render(makes, fn, sample_rate=44100.0, blocks=14, n_in=n_in, resources=node_case_resources())
    if key == "c1":
        return _render(makes, graphs.c1_graph, sample_rate=graphs.C1_SAMPLE_RATE, blocks=100)
    if key == "c2x64":
        return _render(makes, lambda: graphs.c2_graph(64), sample_rate=graphs.C2_SAMPLE_RATE, blocks=60)
    if key == "c4x6":
        return _render(makes, lambda: [graphs.c4_instance(k) for k in range(6)], sample_rate=graphs.C4_SAMPLE_RATE, blocks=60)
    if key.startswith("edge/"):
        res = [_edge(mk, key[5:]) for mk in makes]
        return res[0] if len(res) == 1 else tuple(res)
    one = {"gc": _gc, "sampleseq32": sampleseq_scenario, "sampleseq512": lambda mk: sampleseq_scenario(mk, block=512),
           "events": _events}[key]
    res = [one(mk) for mk in makes]
    return res[0] if len(res) == 1 else tuple(res)


def against_reference(key):
    """The restatement's result for `key`, checked bit for bit against the reference engine: live where oracle/_ref is built,
    otherwise against the recorded digest of the reference's result."""
    if oracle.have_ref():
        got, want = run_scenario(key, port, ref)
        if isinstance(got, np.ndarray) and key.startswith("edge/"):      # NaN != NaN: compare the bits, NaN payloads included
            assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
                f"{key}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} samples differ in their bits"
        elif isinstance(got, np.ndarray):
            assert np.array_equal(got, want), f"{key}: max abs diff {np.abs(got - want).max():.3e}"
        else:
            assert got == want, key
    else:
        got = run_scenario(key, port)
        with open(DIGESTS) as f:
            assert digest(got) == json.load(f)[key], f"{key}: the restatement's bits differ from the reference engine's recorded output"
    return got


@pytest.mark.parametrize("name", sorted(set(NODE_CASES) - REF_ONLY))
def test_node_case_bit_exact(name):
    against_reference("node/" + name)


@pytest.mark.parametrize("name", sorted(set(NODE_EDGE_CASES) - EDGE_REF_ONLY))
def test_edge_case_bit_exact(name):
    """The restatement is the GPU suite's checker wherever oracle/_ref is missing: pinned on the edge corpus too, NaN payloads
    included (clamps, domain edges, non-finite samples through every recurrence, the clock beyond 2^32)."""
    got = against_reference("edge/" + name)
    if name in ("math_domain", "nan_ordering", "nonfinite_into_state"):
        assert np.isnan(got).any() and np.isinf(got).any()


def test_c1_and_c2_bit_exact():
    against_reference("c1")
    against_reference("c2x64")


def test_c4_instances_bit_exact():
    against_reference("c4x6")


def test_gc_matches_reference():
    """gc.test.js:5-43 pattern: nodes of a replaced graph are pruned only after the next rebuild."""
    got = against_reference("gc")
    assert got[0] == [] and len(got[2]) > 0


def test_sampleseq_scenario_bit_exact():
    """builtins/SampleSeq.h: restatement vs the reference engine over the sampleseq.test.js script."""
    got = against_reference("sampleseq32")
    assert np.abs(got).max() > 0.5
    against_reference("sampleseq512")


def test_event_relay_matches_reference():
    """Runtime::processQueuedEvents: same (type, payload) sequence from the restatement and the reference."""
    log = against_reference("events")
    assert sum(len(e) for e in log) > 16
