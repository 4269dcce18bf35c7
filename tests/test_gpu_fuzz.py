"""Randomised graphs (seeded): planner clustering / staging / pipelining edge cases that the hand-written
cases do not reach. Every graph is rendered three ways — reference CPU engine, HIP process(), HIP
process_blocks() (multi-block pipelined launches) — and must agree (1e-6 abs, x max|ref| when > 1)."""
import random

import numpy as np
import pytest

from elementary_amd import el
from helpers import lcg_noise

pytestmark = pytest.mark.gpu
TOL = 1e-6


def random_graph(seed, n_nodes=28, n_roots=3):
    """Nodes are drawn from two pools. `exact` holds signals every IEEE engine computes bit-identically (no libm
    transcendental, no double-precision filter upstream); only those may drive inputs that integrate or threshold
    their argument (oscillator frequencies, comparisons, triggers) — a 1-ulp libm difference there grows without
    bound and says nothing about the engine. Everything else reads from `anyp`."""
    rnd = random.Random(seed)
    X = [el.in_({"channel": 0}), el.in_({"channel": 1})]
    exact = list(X) + [el.const({"value": rnd.uniform(-1, 1)}) for _ in range(3)]
    anyp = list(exact)

    def ex():
        return rnd.choice(exact)

    def pick():
        return rnd.choice(anyp)

    def clip(x):                         # exact limiter
        return el.max(-1.0, el.min(1.0, x))

    E, A = True, False                   # result is exact iff the maker says so (its inputs then all came from `exact`)
    makers = [
        (E, lambda: el.add(ex(), ex())), (E, lambda: el.mul(ex(), ex())), (E, lambda: el.sub(ex(), ex())),
        (A, lambda: el.add(pick(), pick(), pick(), pick())), (A, lambda: el.mul(pick(), pick())),
        (E, lambda: el.min(ex(), ex())), (A, lambda: el.max(pick(), pick())),
        (A, lambda: el.tanh(pick())), (A, lambda: el.sin(el.mul(3.0, pick()))), (E, lambda: el.abs(ex())), (E, lambda: el.sqrt(el.abs(ex()))),
        (E, lambda: el.le(ex(), ex())), (E, lambda: el.geq(ex(), 0.1)),
        (E, lambda: el.phasor(rnd.uniform(1, 2000))), (E, lambda: el.phasor(el.add(300.0, el.mul(200.0, clip(ex()))))),
        (A, lambda: el.blepsaw(rnd.uniform(50, 3000))), (A, lambda: el.blepsquare(el.add(500.0, el.mul(300.0, clip(ex()))))),
        (E, lambda: el.pole(rnd.uniform(0.5, 0.999), clip(ex()))), (A, lambda: el.pole(el.mul(0.9, el.abs(clip(ex()))), pick())),
        (A, lambda: el.env(el.tau2pole(0.001), el.tau2pole(0.02), pick())),
        (A, lambda: el.lowpass(el.add(900.0, el.mul(700.0, clip(pick()))), rnd.uniform(0.5, 4.0), clip(pick()))),
        (A, lambda: el.highpass(rnd.uniform(100, 5000), 1.0, clip(pick()))),
        (A, lambda: el.mm1p({"mode": "lowpass"}, el.prewarp(rnd.uniform(100, 4000)), clip(pick()))),
        (A, lambda: el.biquad(0.2, 0.3, 0.2, -0.5, 0.2, clip(pick()))),
        (E, lambda: el.z(ex())), (E, lambda: el.sdelay({"size": rnd.randint(1, 900)}, ex())),
        (A, lambda: el.delay({"size": rnd.choice([16, 400, 3000])}, rnd.uniform(1, 300), rnd.uniform(-0.5, 0.5), clip(pick()))),
        (A, lambda: el.latch(el.train(rnd.uniform(5, 300)), pick())), (E, lambda: el.counter(el.train(rnd.uniform(5, 100)))),
        (A, lambda: el.accum(el.abs(clip(pick())), el.train(rnd.uniform(5, 50)))),
        (E, lambda: el.seq({"seq": [rnd.uniform(-1, 1) for _ in range(rnd.randint(1, 6))], "hold": rnd.random() < 0.5},
                           el.train(rnd.uniform(20, 400)), el.train(rnd.uniform(1, 20)))),
        (E, lambda: el.seq2({"seq": [rnd.uniform(-1, 1) for _ in range(rnd.randint(1, 6))]}, el.train(rnd.uniform(20, 400)), 0)),
        (E, lambda: el.rand({"seed": rnd.randint(1, 1 << 30)})), (E, lambda: el.mul(1e-5, el.time())), (E, lambda: el.metro({"interval": rnd.uniform(1, 20)})),
        (A, lambda: el.maxhold({"hold": rnd.uniform(0.5, 5.0)}, el.abs(pick()), el.train(rnd.uniform(2, 40)))),
        (E, lambda: el.sparseq2({"interpolate": rnd.randint(0, 1), "seq": [{"time": 512.0 * k, "value": rnd.uniform(-1, 1)} for k in range(1, 9)]}, el.time())),
    ]
    for _ in range(n_nodes):
        is_exact, mk = rnd.choice(makers)
        node = mk()
        anyp.append(node)
        if is_exact:
            exact.append(node)
    return [el.tanh(el.add(*rnd.sample(anyp[5:], 4))) for _ in range(n_roots)]


@pytest.mark.parametrize("seed", range(48))
def test_random_graph(gpu_required, seed):
    import torch
    import oracle
    from elementary_amd.runtime import Runtime
    nb, n_out = 22, min(3, 1 + seed % 5)
    x = np.stack([np.stack([lcg_noise(512, 11 + 7 * k + c, 0.5) for c in range(2)]) for k in range(nb)])   # [nb, 2, 512]
    chk = oracle.RefRuntime(48000.0, 512) if oracle.have_ref() else oracle.PortRuntime(48000.0, 512)
    a, b = Runtime(48000.0, 512), Runtime(48000.0, 512)
    b.set_option("batch_blocks", 5 + seed % 7)
    for rt in (chk, a, b):
        assert rt.render(*random_graph(seed, n_nodes=24 + 22 * (seed % 4), n_roots=1 + seed % 5)[:n_out])["result"] == 0
    ref = np.stack([chk.process(x[k], n_out, 512) for k in range(nb)])
    got = np.stack([a.process(x[k], n_out, 512) for k in range(nb)])
    xin = torch.from_numpy(x).cuda()
    out = torch.zeros((nb, n_out, 512), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    b.process_blocks(nb, n_out, out_ptr=out.data_ptr(), in_ptr=xin.data_ptr(), num_inputs=2)
    batched = out.cpu().numpy()
    assert np.isfinite(ref).all()
    scale = max(1.0, float(np.abs(ref).max()))
    assert float(np.abs(got - ref).max()) <= TOL * scale, f"seed {seed}: process() max err {np.abs(got - ref).max():.3e}"
    assert np.array_equal(batched, got), f"seed {seed}: process_blocks differs from process by {np.abs(batched - got).max():.3e}"
    assert b.stats()["batch_launches"] > 0


def wild_graph(seed, n_nodes=40, n_roots=3):
    """random_graph's discipline (`exact` / `anyp`) with parameters drawn ACROSS every clamp instead of inside it: filter cutoffs
    in [-500, 40 000] Hz (the SVF clamps to [20, sr/2.0001], prewarp + mm1p to g in [0, 0.9999]), Q in [-1, 60] (clamp [0.25, 20]),
    delay lengths in [-50, 2 size] (clamp [0, size]; constants and exact signals), feedback in [-3, 3] (clamp +-1), phasor and
    oscillator frequencies in [-3000, 60 000] Hz, table indices in [-2, 3] (clamp [0, 1]). Whatever can grow without bound (an
    oscillator at a negative frequency) enters the pools through the exact limiter; an index or a length is always a finite
    value: a constant, or an affine map of a limited signal."""
    rnd = random.Random(7000 + seed)
    X = [el.in_({"channel": 0}), el.in_({"channel": 1})]
    exact = list(X) + [el.const({"value": rnd.uniform(-1, 1)}) for _ in range(3)]
    anyp = list(exact)

    def ex():
        return rnd.choice(exact)

    def pick():
        return rnd.choice(anyp)

    def clip(x):                         # exact limiter (a NaN comes out as 1: std::min(1, NaN) == 1)
        return el.max(-1.0, el.min(1.0, x))

    def span(lo, hi, src):               # a constant in [lo, hi], or a signal sweeping a random part of it
        if rnd.random() < 0.5:
            return rnd.uniform(lo, hi)
        a, b = sorted(rnd.uniform(lo, hi) for _ in range(2))
        return el.add(0.5 * (a + b), el.mul(0.5 * (b - a), clip(src())))

    def svf():
        f = rnd.choice([el.lowpass, el.highpass, el.bandpass, el.notch, el.allpass])
        return f(span(-500.0, 40000.0, pick), span(-1.0, 60.0, pick), clip(pick()))

    def shelf():
        f = rnd.choice([el.lowshelf, el.highshelf, el.peak])
        return f(span(-500.0, 40000.0, pick), span(-1.0, 60.0, pick), span(-40.0, 40.0, pick), clip(pick()))

    def mm1p():
        g = el.prewarp(span(-500.0, 40000.0, pick)) if rnd.random() < 0.6 else span(-0.5, 3.0, pick)
        return el.mm1p({"mode": rnd.choice(["lowpass", "highpass", "allpass"])}, g, clip(pick()))

    def delay():
        size = rnd.choice([16, 400, 600, 3000])
        return el.delay({"size": size}, span(-50.0, 2.0 * size, ex), span(-3.0, 3.0, pick), clip(pick()))

    def table():
        return el.table({"path": rnd.choice(["/t/ramp", "/t/five", "/t/one"])}, span(-2.0, 3.0, pick))

    E, A = True, False
    makers = [
        (E, lambda: el.add(ex(), ex())), (E, lambda: el.mul(ex(), ex())), (E, lambda: el.sub(ex(), ex())),
        (A, lambda: el.add(pick(), pick(), pick())), (A, lambda: el.mul(pick(), pick())),
        (E, lambda: el.min(ex(), ex())), (A, lambda: el.max(pick(), pick())), (A, lambda: el.tanh(pick())),
        (E, lambda: el.le(ex(), ex())), (E, lambda: el.abs(ex())),
        (E, lambda: el.phasor(span(-3000.0, 60000.0, ex))), (E, lambda: el.phasor(span(-3000.0, 60000.0, ex))),
        (E, lambda: el.syncphasor(span(-3000.0, 60000.0, ex), el.train(rnd.uniform(5, 300)))),
        (A, lambda: clip(el.blepsaw(span(-3000.0, 60000.0, ex)))), (A, lambda: clip(el.blepsquare(span(-3000.0, 60000.0, ex)))),
        (A, lambda: clip(el.bleptriangle(span(-3000.0, 60000.0, ex)))),
        (A, svf), (A, svf), (A, svf), (A, shelf), (A, shelf), (A, mm1p), (A, mm1p), (A, delay), (A, delay), (A, delay), (A, table), (A, table),
        (E, lambda: el.pole(rnd.uniform(0.5, 0.999), clip(ex()))), (E, lambda: el.z(ex())),
        (E, lambda: el.counter(el.train(rnd.uniform(5, 100)))), (A, lambda: el.latch(el.train(rnd.uniform(5, 300)), pick())),
    ]
    for _ in range(n_nodes):
        is_exact, mk = rnd.choice(makers)
        node = mk()
        anyp.append(node)
        if is_exact:
            exact.append(node)
    return [el.tanh(el.add(*rnd.sample(anyp[5:], 4))) for _ in range(n_roots)]


# seeds on which the reference engine's output is finite (chosen on the CPU from 0, 1, 2, ...: a seed on which it is not is
# replaced by the next one, never skipped; the first 24 all are)
WILD_SEEDS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]


@pytest.mark.parametrize("seed", WILD_SEEDS)
def test_wild_graph(gpu_required, seed):
    """wild_graph three ways, as test_random_graph: reference engine, HIP process(), HIP process_blocks(); the same tolerance
    (1e-6 abs, x max|ref| when > 1) and the two HIP paths equal bit for bit. 8 blocks behind the two of the root fade-in, which
    process_blocks gets in a call of their own (it renders launch sets only once the fades have settled)."""
    import torch
    import oracle
    from cases import node_case_resources
    from elementary_amd.runtime import Runtime
    nb, fade, n_out = 10, 2, 3
    x = np.stack([np.stack([lcg_noise(512, 11 + 7 * k + c, 0.5) for c in range(2)]) for k in range(nb)])   # [nb, 2, 512]
    chk = oracle.RefRuntime(48000.0, 512) if oracle.have_ref() else oracle.PortRuntime(48000.0, 512)
    a, b = Runtime(48000.0, 512), Runtime(48000.0, 512)
    b.set_option("batch_blocks", 3 + seed % 4)
    for rt in (chk, a, b):
        for rname, data in node_case_resources().items():
            assert rt.add_shared_resource(rname, data)
        assert rt.render(*wild_graph(seed))["result"] == 0
    ref = np.stack([chk.process(x[k], n_out, 512) for k in range(nb)])
    got = np.stack([a.process(x[k], n_out, 512) for k in range(nb)])
    xin = torch.from_numpy(x).cuda()
    out = torch.zeros((nb, n_out, 512), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    b.process_blocks(fade, n_out, out_ptr=out.data_ptr(), in_ptr=xin.data_ptr(), num_inputs=2)
    b.process_blocks(nb - fade, n_out, out_ptr=out[fade:].data_ptr(), in_ptr=xin[fade:].data_ptr(), num_inputs=2)
    batched = out.cpu().numpy()
    assert np.isfinite(ref).all()
    scale = max(1.0, float(np.abs(ref).max()))
    assert np.isfinite(got).all()
    assert float(np.abs(got - ref).max()) <= TOL * scale, f"seed {seed}: process() max err {np.abs(got - ref).max():.3e}"
    assert np.array_equal(batched, got), f"seed {seed}: process_blocks differs from process by {np.abs(batched - got).max():.3e}"
    assert b.stats()["batch_launches"] > 0


def amplifying_graph(seed):
    """The family `random_graph` leaves out on purpose: a libm transcendental or a double-precision filter result in front of
    something that integrates or thresholds it. A 1-ulp difference between device libm and glibc is then amplified — by
    the integration time for an oscillator frequency, to a full-scale step where a comparison flips — in ANY pair of IEEE
    engines, so the 1e-6 bar cannot hold sample for sample; what can be measured is how rare and how large the effect is."""
    rnd = random.Random(1000 + seed)
    x0, x1 = el.in_({"channel": 0}), el.in_({"channel": 1})
    soft = el.tanh(el.mul(2.0, x0))                                                    # transcendental
    filt = el.lowpass(el.add(900.0, el.mul(500.0, x1)), rnd.uniform(0.7, 3.0), x0)     # double-precision filter
    makers = [
        lambda: el.phasor(el.add(300.0, el.mul(250.0, soft))),                         # frequency integrates into the phase
        lambda: el.blepsaw(el.add(400.0, el.mul(300.0, el.sin(el.mul(3.0, x1))))),
        lambda: el.le(filt, rnd.uniform(-0.05, 0.05)),                                 # a threshold on a filter output
        lambda: el.latch(el.le(el.sin(el.mul(40.0, x0)), 0.0), x1),                    # trigger from a transcendental
        lambda: el.accum(el.abs(soft), el.train(rnd.uniform(20, 60))),                 # running sum of a transcendental
        lambda: el.pole(0.995, soft),                                                  # leaky integrator, gain 200
        lambda: el.counter(el.geq(filt, 0.0)),
        lambda: el.maxhold({"hold": 2.0}, el.abs(filt), el.train(10.0)),
    ]
    picks = [mk() for mk in rnd.sample(makers, 4)]
    return [el.mul(0.25, el.add(*picks))]


@pytest.mark.parametrize("seed", range(6))
def test_transcendental_into_integrators_and_comparators(gpu_required, seed):
    """Measured, not just documented (tests/test_gpu_fuzz.py:17-21). Stated bar for this family: at least
    99.5 % of the samples within 1e-5 of the reference engine and a median error <= 1e-6 — a flipped comparison or a latched
    neighbour value is a rare O(1) event, drift of an integrated frequency stays below 1e-5 over the 22 blocks."""
    import oracle
    from elementary_amd.runtime import Runtime
    nb = 22
    x = np.stack([np.stack([lcg_noise(512, 311 + 7 * k + c, 0.5) for c in range(2)]) for k in range(nb)])
    chk = oracle.RefRuntime(48000.0, 512) if oracle.have_ref() else oracle.PortRuntime(48000.0, 512)
    a = Runtime(48000.0, 512)
    for rt in (chk, a):
        assert rt.render(*amplifying_graph(seed))["result"] == 0
    ref = np.stack([chk.process(x[k], 1, 512) for k in range(nb)])
    got = np.stack([a.process(x[k], 1, 512) for k in range(nb)])
    err = np.abs(got - ref).ravel()
    scale = max(1.0, float(np.abs(ref).max()))
    within = float((err <= 1e-5 * scale).mean())
    assert np.isfinite(got).all()
    assert within >= 0.995 and float(np.median(err)) <= 1e-6 * scale, f"seed {seed}: {100 * within:.2f} % within 1e-5, median {np.median(err):.2e}, max {err.max():.2e}"
