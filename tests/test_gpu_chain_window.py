"""The store windows of the quad-skewed recurrence loop (elementary_amd/csrc/chain_skew.h, island_ops.inc chain_loop_q): a lane keeps
its 16-byte piece of W consecutive groups and stores the W of them under one EXEC switch; a window never leaves its span, and the
last one of a block closes before the state hand-over. Built on test_gpu_chain_skew's check and graphs, at the block sizes where the
window meets an edge of the schedule: 64 frames (one span of the depth-4 loops: head, window and state hand-over in one span), 128
(one span of the depth-8 loop: two windows), 192 and 512.

Every case asserts what test_gpu_chain_skew._check asserts: launch sets bit-identical to the same engine rendering block by block,
7 + 13 blocks in two calls equal to 20 in one, within 1e-6 of the reference engine, and bit-equal to it after the root fade for the
graphs of plain float arithmetic."""
import numpy as np
import pytest

from elementary_amd import el
from helpers import lcg_noise
import test_gpu_chain_skew as skew

pytestmark = pytest.mark.gpu

# graphs this file adds to the ones it borrows, for the time of its own tests
EXTRA = {
    "poles3": (lambda: skew._poles(3), True),                 # three members: lanes 12 .. 63 mirror the last one and do not store
    "phasor_const": (lambda: [el.mul(el.phasor(440.0), el.add(1.0, skew._x()))], True),   # a recurrence without a streamed operand
}
NAMES = ["pole", "poles3", "poles16", "sphasor", "maxhold", "phasor_const", "c2_voice"]


@pytest.fixture(autouse=True)
def _extra_graphs(monkeypatch):
    for name, graph in EXTRA.items():
        monkeypatch.setitem(skew.GRAPHS, name, graph)


@pytest.mark.parametrize("bs", [64, 128, 192, 512])
@pytest.mark.parametrize("name", NAMES)
def test_windowed_stores_at_every_span_shape(gpu_required, name, bs):
    skew._check(name, bs, None)


@pytest.mark.parametrize("copies", [1, 3, 6])
@pytest.mark.parametrize("name", ["c2_voice", "poles16"])
def test_blocks_in_flight_at_block_64(gpu_required, name, copies):
    """One span per block: the window that closes a block is the one the next block's first loads and the deferred publish follow."""
    skew._check(name, 64, copies)


@pytest.mark.parametrize("name", ["c2_voice", "poles16"])
def test_twelve_launch_sets_of_one_block(gpu_required, name):
    """A launch set of a single block twelve times over: every set starts with a head and ends with a closing window and a state
    hand-over, and nothing else."""
    bs, nb = 64, 12
    mk, exact = skew.GRAPHS[name]
    x = np.stack([np.stack([lcg_noise(bs, 5 + 2 * k + ch, 0.5) for ch in range(2)]) for k in range(nb)]).astype(np.float32)
    a, b, s = skew._engine(bs, mk(), None), skew._engine(bs, mk(), None), skew._engine(bs, mk(), None)
    ones, one_set = skew._in_sets(a, (1,) * nb, x, bs), skew._in_sets(b, (nb,), x, bs)
    by_block = np.stack([s.process(x[k], 1, bs) for k in range(nb)])
    for rt in (a, b, s):
        assert rt.stats()["spec_launches"] > 0, rt.stats()
    c = skew._checker(bs)
    assert c.render(*mk())["result"] == 0
    ref = np.stack([c.process(x[k], 1, bs) for k in range(nb)])
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(ones - ref).max())
    print(f"{name}: twelve sets of one block, max |sets - reference| {err:.3e} (scale {scale:.3g})")
    assert np.isfinite(ones).all()
    assert np.array_equal(ones, by_block), f"{name}: sets of one block vs block by block {np.abs(ones - by_block).max():.3e}"
    assert np.array_equal(ones, one_set), f"{name}: twelve sets of one block vs one set of twelve {np.abs(ones - one_set).max():.3e}"
    assert err <= skew.TOL * scale, f"{name}: vs the reference {err:.3e}"
    if exact:
        assert np.array_equal(ones[skew.SETTLED:], ref[skew.SETTLED:]), f"{name}: not bit-identical to the reference"
