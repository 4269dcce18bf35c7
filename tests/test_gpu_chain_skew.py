"""The quad-skewed recurrence loop of the specialised kernels (elementary_amd/csrc/chain_skew.h, island_ops.inc chain_loop_q): a task of
up to 16 float recurrences gives every member four lanes that run its chain 0, 4, 8 and 12 frames apart and share one 16-byte store
per group; group 0 of a block and the 12 steps behind the last group are predicated per lane. Small graphs whose recurrence tasks take
that loop (and the shapes that must NOT take it: 17 members, the wide biquad), at block sizes 64 .. 512, 1 .. 6 blocks in flight and
launch sets of 1, 2, 7, 13 and 20 blocks.

Every case: the launch-set output is bit-identical to the same engine rendering block by block through `process`; once the root
fade has settled a graph of plain float arithmetic is bit-identical to the reference engine as well (the C2 voice, with its libm
oscillators, within the suite's 1e-6 bar); 7 + 13 blocks in two calls equal 20 in one — the state a launch set writes back to the
node records is the serial loop's, whichever lane of a quad wrote it."""
import numpy as np
import pytest

from elementary_amd import el, graphs
from helpers import lcg_noise

pytestmark = pytest.mark.gpu
TOL = 1e-6
SETTLED = 3            # blocks after which the root gain is exactly 1 (test_gpu_spec.py: the merged phase task test)


def _x(ch=0):
    return el.in_({"channel": ch})


def _poles(count):
    # `count` independent one-poles of one stage, each on its own stream, summed into one root: one island, one task
    return [el.add(*[el.pole(0.5 + 0.025 * k, el.mul(0.05 * (k + 1), _x())) for k in range(count)])]


def _gate(ch, level):
    return el.le(_x(ch), level)


def _biquad_signals():
    w = el.add(1.0, el.mul(0.1, _x(1)))
    return [el.biquad(el.mul(0.2, w), el.mul(0.3, w), el.mul(0.2, w), el.mul(-0.5, w), el.mul(0.2, w), _x())]


# name -> (roots, exact): exact = nothing but float +, -, *, compare between the inputs and the root
GRAPHS = {
    "pole": (lambda: [el.pole(0.97, _x())], True),
    "c2_voice": (lambda: [graphs.c2_voice(3)], False),
    "poles16": (lambda: _poles(16), True),
    "poles17": (lambda: _poles(17), True),
    "env": (lambda: [el.env(0.9, 0.995, _x())], True),
    "phasor_signal": (lambda: [el.phasor(el.add(440.0, el.mul(200.0, _x())))], True),
    "sphasor": (lambda: [el.syncphasor(el.add(300.0, el.mul(100.0, _x())), _gate(1, 0.0))], True),
    "counter": (lambda: [el.counter(_gate(0, 0.2))], True),
    "accum": (lambda: [el.accum(_x(), _gate(1, -0.4))], True),
    "latch": (lambda: [el.latch(_gate(1, 0.0), _x())], True),
    "maxhold": (lambda: [el.maxhold({"hold": 10.0}, _x(), _gate(1, -0.45))], True),
    "biquad_const": (lambda: [el.biquad(0.2, 0.3, 0.2, -0.5, 0.2, _x())], True),
    "biquad_signal": (_biquad_signals, True),
}
SR = 48000.0
CALLS_A = (7, 13, 1, 2)       # launch sets of 7, 13, 1 and 2 blocks
CALLS_B = (20, 3)             # ... and 20 in one call: blocks 0 .. 19 are CALLS_A's 7 + 13
NB = sum(CALLS_A)


def _checker(bs):
    import oracle
    return oracle.RefRuntime(SR, bs) if oracle.have_ref() else oracle.PortRuntime(SR, bs)


def _engine(bs, roots, copies):
    from elementary_amd.runtime import Runtime
    rt = Runtime(SR, bs, device=0)
    rt.set_option("specialize", 2)
    rt.set_option("batch_blocks", 20)
    if copies is not None:
        rt.set_option("pipeline_copies", copies)
    assert rt.render(*roots)["result"] == 0
    return rt


def _in_sets(rt, calls, x, bs):
    import torch
    outs, at = [], 0
    for nb in calls:
        out = torch.zeros((nb, 1, bs), dtype=torch.float32, device="cuda")
        xin = torch.from_numpy(np.ascontiguousarray(x[at:at + nb])).cuda()
        torch.cuda.synchronize()
        rt.process_blocks(nb, 1, out_ptr=out.data_ptr(), in_ptr=xin.data_ptr(), num_inputs=2)
        outs.append(out.cpu().numpy())
        at += nb
    return np.concatenate(outs)


def _check(name, bs, copies):
    mk, exact = GRAPHS[name]
    assert sum(CALLS_B) == NB
    x = np.stack([np.stack([lcg_noise(bs, 3 + 2 * k + ch, 0.5) for ch in range(2)]) for k in range(NB)]).astype(np.float32)
    a, b, s = _engine(bs, mk(), copies), _engine(bs, mk(), copies), _engine(bs, mk(), copies)
    got_a, got_b = _in_sets(a, CALLS_A, x, bs), _in_sets(b, CALLS_B, x, bs)
    by_block = np.stack([s.process(x[k], 1, bs) for k in range(NB)])
    for rt in (a, b, s):
        st = rt.stats()
        assert st["spec_launches"] > 0, st
        assert all(rt.spec_info(q)["state"] == 1 for q in range(st["spec_shapes"])), st
    c = _checker(bs)
    assert c.render(*mk())["result"] == 0
    ref = np.stack([c.process(x[k], 1, bs) for k in range(NB)])
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got_a - ref).max())
    print(f"{name} bs {bs} copies {copies}: max |sets - reference| {err:.3e} (scale {scale:.3g}), "
          f"sets == block by block: {np.array_equal(got_a, by_block)}, 7 + 13 == 20: {np.array_equal(got_a, got_b)}, "
          f"bit-equal to the reference after the fade: {np.array_equal(got_a[SETTLED:], ref[SETTLED:])}")
    assert np.isfinite(got_a).all()
    assert np.array_equal(got_a, by_block), f"{name}: launch sets vs block by block {np.abs(got_a - by_block).max():.3e}"
    assert np.array_equal(got_a, got_b), f"{name}: 7 + 13 blocks vs 20 in one call {np.abs(got_a - got_b).max():.3e}"
    assert err <= TOL * scale, f"{name}: vs the reference {err:.3e}"
    if exact:
        assert np.array_equal(got_a[SETTLED:], ref[SETTLED:]), f"{name}: not bit-identical to the reference, {np.abs(got_a - ref)[SETTLED:].max():.3e}"


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_recurrence_graphs_at_block_512(gpu_required, name):
    _check(name, 512, None)


@pytest.mark.parametrize("bs", [64, 128, 192])
@pytest.mark.parametrize("name", ["pole", "c2_voice", "poles16", "sphasor"])
def test_other_block_sizes(gpu_required, name, bs):
    """64 and 192: one and three spans of the depth-4 loops; 128: a single span of the depth-8 loop (head and last span in one)."""
    _check(name, bs, None)


@pytest.mark.parametrize("copies", [1, 3, 6])
@pytest.mark.parametrize("name", ["c2_voice", "poles16"])
def test_blocks_in_flight(gpu_required, name, copies):
    _check(name, 512, copies)
