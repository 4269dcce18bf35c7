"""The end of a block in the quad-skewed recurrence loop (elementary_amd/csrc/chain_skew.h, island_ops.inc chain_loop_q): behind the
last group the three lagging lanes of a quad take the member's state registers from the lane of skew 0 (one DPP quad permute per
register) instead of stepping their last 4, 8 or 12 frames themselves. Every lane of the wave then writes the node record, so a
wrong register in any lane shows at the next launch boundary, and a wrong one in lane 0 inside the launch set.

Every case asserts, with the graph makers and the checker of test_gpu_chain_skew.py: the launch-set output is bit-identical to the
same engine rendering block by block through `process`; 7 + 13 blocks in two calls equal 20 in one (the record written back at a
launch boundary and read again); the output is within 1e-6 of the reference and, for the graphs of plain float arithmetic,
bit-equal to it once the root fade has settled.

Shapes: block sizes 64 (one span: the head and the broadcast in the same span), 128, 192 and 512; one member, 16 members (every lane
a member lane), 3 members (mirror lanes beside the quads), two carried registers (sphasor), three (maxhold, one of them an integer),
the counter, the C2 voice; 1, 3 and 6 blocks in flight; launch sets of one block; a constant changed between two launch sets."""
import numpy as np
import pytest

from elementary_amd import el
from helpers import lcg_noise
import test_gpu_chain_skew as skew
from test_gpu_chain_skew import SETTLED, TOL, _checker, _engine, _in_sets, _poles, _x

pytestmark = pytest.mark.gpu

POLES3 = (lambda: _poles(3), True)       # three quads and 52 mirror lanes
NAMES = ["pole", "poles16", "poles3", "sphasor", "counter", "maxhold", "c2_voice"]


@pytest.mark.parametrize("bs", [64, 128, 192, 512])
@pytest.mark.parametrize("name", NAMES)
def test_state_after_the_quad_broadcast(gpu_required, monkeypatch, name, bs):
    monkeypatch.setitem(skew.GRAPHS, "poles3", POLES3)
    skew._check(name, bs, None)


@pytest.mark.parametrize("copies", [1, 3, 6])
@pytest.mark.parametrize("name", ["poles16", "c2_voice"])
def test_blocks_in_flight(gpu_required, name, copies):
    skew._check(name, 64, copies)


def _noise(nb, bs):
    return np.stack([np.stack([lcg_noise(bs, 3 + 2 * k + ch, 0.5) for ch in range(2)]) for k in range(nb)]).astype(np.float32)


@pytest.mark.parametrize("name", ["pole", "poles3", "maxhold"])
def test_launch_sets_of_one_block(gpu_required, monkeypatch, name):
    """Twelve launch sets of one block each: the record is read, the block rendered and the record written in every launch."""
    monkeypatch.setitem(skew.GRAPHS, "poles3", POLES3)
    bs, nb = 64, 12
    mk, exact = skew.GRAPHS[name]
    x = _noise(nb, bs)
    a, s = _engine(bs, mk(), None), _engine(bs, mk(), None)
    got = _in_sets(a, (1,) * nb, x, bs)
    by_block = np.stack([s.process(x[k], 1, bs) for k in range(nb)])
    st = a.stats()
    assert st["spec_launches"] > 0 and all(a.spec_info(q)["state"] == 1 for q in range(st["spec_shapes"])), st
    c = _checker(bs)
    assert c.render(*mk())["result"] == 0
    ref = np.stack([c.process(x[k], 1, bs) for k in range(nb)])
    err = float(np.abs(got - ref).max())
    print(f"{name}: one-block sets, max |sets - reference| {err:.3e}, == block by block: {np.array_equal(got, by_block)}")
    assert np.array_equal(got, by_block)
    assert err <= TOL * max(1.0, float(np.abs(ref).max()))
    assert exact and np.array_equal(got[SETTLED:], ref[SETTLED:])


@pytest.mark.parametrize("bs", [64, 512])
def test_a_constant_changed_between_two_launch_sets(gpu_required, bs):
    """The pole's coefficient is a keyed const: 7 blocks with p = 0.97, the property set to 0.5, 13 more blocks. The second set starts
    from the first set's final state and uses the new coefficient, as block-by-block rendering and the reference do."""
    def roots(p):
        return [el.pole(el.const({"key": "p", "value": p}), _x())]

    nb1, nb2 = 7, 13
    x = _noise(nb1 + nb2, bs)
    a, s, c = _engine(bs, roots(0.97), None), _engine(bs, roots(0.97), None), _checker(bs)
    assert c.render(*roots(0.97))["result"] == 0
    got1 = _in_sets(a, (nb1,), x[:nb1], bs)
    by1 = np.stack([s.process(x[k], 1, bs) for k in range(nb1)])
    ref1 = np.stack([c.process(x[k], 1, bs) for k in range(nb1)])
    for rt in (a, s, c):
        assert rt.render(*roots(0.5))["result"] == 0
    got2 = _in_sets(a, (nb2,), x[nb1:], bs)
    by2 = np.stack([s.process(x[k], 1, bs) for k in range(nb1, nb1 + nb2)])
    ref2 = np.stack([c.process(x[k], 1, bs) for k in range(nb1, nb1 + nb2)])
    got, by_block, ref = np.concatenate([got1, got2]), np.concatenate([by1, by2]), np.concatenate([ref1, ref2])
    st = a.stats()
    assert st["spec_launches"] > 0 and all(a.spec_info(q)["state"] == 1 for q in range(st["spec_shapes"])), st
    # the new coefficient is in use: an engine that kept 0.97 would go on as the unchanged graph does
    keep = _engine(bs, roots(0.97), None)
    stale = _in_sets(keep, (nb1, nb2), x, bs)
    err = float(np.abs(got - ref).max())
    print(f"bs {bs}: max |sets - reference| {err:.3e}, == block by block: {np.array_equal(got, by_block)}, "
          f"second set differs from p = 0.97 by {np.abs(got[nb1:] - stale[nb1:]).max():.3e}")
    assert np.array_equal(stale[:nb1], got1) and not np.array_equal(stale[nb1:], got2)
    assert np.array_equal(got, by_block)
    assert err <= TOL * max(1.0, float(np.abs(ref).max()))
    assert np.array_equal(got[SETTLED:], ref[SETTLED:])
