"""Option "capture_history_blocks" on the GPU: `capture` and `mc.capture` nodes with a device ring that keeps a whole relay window of
takes and a per-block log, and a blockwise relay that replays from it what a relay after every block would have drained and
emitted (elementary_amd/csrc/capture_replay.h) — launch sets of full size with such a listener attached.

The reference is what test_gpu_events.py uses: the reference engine behind OfflineRenderer, relayed after every block, the takes'
samples within that file's TOL. Gates are `ge(in 1, 0.5)` over a 0/1 pattern written here, so every edge is exact.
"""
import numpy as np
import pytest

import test_gpu_events as ge
from elementary_amd import el
from elementary_amd.offline import OfflineRenderer
from helpers import lcg_noise_fast

pytestmark = pytest.mark.gpu
TOL = ge.TOL
KINDS = ("capture", "mc.capture", "meter")


def _square(frames, high, low, start=0):
    """0/1 pattern: `high` frames on, `low` frames off, from frame `start` (off before it)."""
    g = np.zeros(frames, np.float32)
    k = np.arange(frames - start)
    g[start:] = ((k % (high + low)) < high).astype(np.float32)
    return g


def _collect(factory, calls, n_out, bs, **kw):
    """`calls`: [(roots function, gate pattern, ...)] — a render and a process per entry; input 0 is noise, inputs 1, 2 the gate
    patterns (2: zeros where a call brings one). `kw`: keywords of OfflineRenderer.initialize (none: it is called without).
    -> (events, output, renderer)"""
    core = OfflineRenderer(factory)
    core.initialize(num_input_channels=3, num_output_channels=n_out, sample_rate=48000.0, block_size=bs, **kw)
    log = []
    for kind in KINDS:
        core.on(kind, lambda p, kind=kind: log.append((kind, p)))
    outs = []
    for k, (roots_fn, *gates) in enumerate(calls):
        frames = len(gates[0])
        core.render(*roots_fn())
        out = [np.zeros(frames, np.float32) for _ in range(n_out)]
        core.process([lcg_noise_fast(frames, 11 + k, 0.5), gates[0], gates[1] if len(gates) > 1 else np.zeros(frames, np.float32)], out)
        outs.append(np.stack(out))
    return log, np.concatenate(outs, axis=1), core


def _gate(channel=1):
    return el.ge(el.in_({"channel": channel}), 0.5)


def _mono(gain=0.5):
    def roots():
        x = el.in_({"channel": 0})
        return [el.capture({"name": "c"}, _gate(), x), el.meter({"name": "m"}, el.mul(gain, x))]
    return roots


def _against_reference(calls, n_out, bs, window, host_blocks, engine_blocks=None):
    a, ya, core = _collect(ge._hip, calls, n_out, bs, capture_history_blocks=window)
    b, yb, _ = _collect(ge._ref, calls, n_out, bs)
    ge._same_events(a, b)
    assert float(np.abs(ya - yb).max()) <= TOL
    assert core.runtime.event_window_blocks() == window
    st = core.runtime.stats()
    # single-block calls would leave no launch set behind (the first blocks, while the roots fade in, go block by block)
    assert st["blocks_rendered"] == (engine_blocks or host_blocks) and st["batch_launches"] >= 1, st
    return [p for k, p in b if k != "meter"], a


def test_takes_across_block_boundaries(gpu_required):
    """Block 128, 96 blocks in one window of 96; the gate is high for 160 frames and low for 160: every take straddles a block
    boundary and the flush of the 128-frame scratch, and a meter beside the node reports every block — the reference's events in
    the reference's order."""
    takes, a = _against_reference([(_mono(), _square(96 * 128, 160, 160))], 2, 128, 96, 96)
    assert len(takes) == 38 and all(len(p["data"]) == 160 for p in takes)
    assert [k for k, _ in a].count("meter") == 96 and a[0][0] == "meter" and a[-1][0] == "meter"


def test_several_falls_in_one_block(gpu_required):
    """Block 512, 32 blocks; a gate of period 24 falls 21 times per block, a noisy gate (`ge(noise, 0.2)`) and a 37 Hz `train` beside
    it: one event per node and block in which its gate fell, carrying everything flushed in that block."""
    def roots():
        x = el.in_({"channel": 0})
        return [el.capture({"name": "fast"}, _gate(), x), el.capture({"name": "noisy"}, el.ge(x, 0.2), el.mul(2.0, x)),
                el.add(el.capture({"name": "train"}, el.train(37.0), x), el.meter({"name": "m"}, x))]
    takes, _ = _against_reference([(roots, _square(32 * 512, 12, 12))], 3, 512, 32, 32)
    assert [p["source"] for p in takes].count("fast") == 32 and [p["source"] for p in takes].count("noisy") == 32
    assert 10 <= [p["source"] for p in takes].count("train") <= 13
    assert all(len(p["data"]) in (252, 264) for p in takes if p["source"] == "fast")      # 21 or 22 runs of 12 frames


def test_a_take_longer_than_the_reference_ring(gpu_required):
    """Block 512, 160 blocks in one window; the gate is high from frame 100 to frame 81 000: one take of 80 900 frames, more than the
    65 536 a device copy of the reference's ring holds — one event, every frame."""
    g = np.zeros(160 * 512, np.float32)
    g[100:81000] = 1.0
    takes, _ = _against_reference([(_mono(), g)], 2, 512, 160, 160)
    assert len(takes) == 1 and len(takes[0]["data"]) == 80900


def test_sliced_host_block(gpu_required):
    """A host block of 1024 frames is two engine blocks; the gate falls at frame 300 of every host block (first slice) and rises again
    at frame 700 (second slice): the event of a host block carries what was flushed up to its end, as the reference's does."""
    pattern = np.tile(np.concatenate([np.ones(300), np.zeros(400), np.ones(324)]).astype(np.float32), 24)
    takes, _ = _against_reference([(_mono(), pattern)], 2, 1024, 24, 24, engine_blocks=48)
    assert len(takes) == 24 and len(takes[0]["data"]) == 300 + 256 and len(takes[1]["data"]) == 624


def test_a_take_across_two_process_calls_and_a_rerender(gpu_required):
    """Two calls of 32 blocks of 512 in windows of 32, a re-render in between that keeps the capture node (the meter gets a new
    input): a take that begins at frame 9000 of the first call ends at frame 5000 of the second."""
    first, second = _square(32 * 512, 700, 900), _square(32 * 512, 800, 600, start=5000)
    first[9000:] = 1.0
    second[:5000] = 1.0
    second[5000:5600] = 0.0
    takes, _ = _against_reference([(_mono(), first), (_mono(0.25), second)], 2, 512, 32, 64)
    assert (32 * 512 - 9000) + 5000 in [len(p["data"]) for p in takes] and len(takes) == 15


def test_mc_capture_with_a_commit_in_between(gpu_required):
    """`mc.capture` of two channels gated by the first test's pattern beside one of one channel gated by the second test's, block
    128, two calls of 96 blocks in windows of 96 with a commit in between (the reference makes the nodes' rings anew when the new
    sequence is pushed): whatever the reference emits."""
    def roots(gain):
        def fn():
            x = el.in_({"channel": 0})
            slow = el.mc.capture({"name": "two", "channels": 2}, _gate(), x, el.mul(0.5, x))
            fast = el.mc.capture({"name": "one", "channels": 1}, _gate(2), el.mul(2.0, x))
            return list(slow) + list(fast) + [el.meter({"name": "m"}, el.mul(gain, x))]
        return fn
    g, g2 = _square(96 * 128, 160, 160), _square(96 * 128, 12, 12)
    takes, _ = _against_reference([(roots(0.5), g, g2), (roots(0.25), g, g2)], 4, 128, 96, 192)
    two = [p for p in takes if p["source"] == "two"]
    assert len(two) >= 70 and all(len(p["data"]) == 2 for p in two) and len([p for p in takes if p["source"] == "one"]) >= 150


def test_option_off_is_the_engine_never_told(gpu_required):
    """`capture_history_blocks = 0`, no keyword at all, and `event_history_blocks = 64` alone: the same events, output bytes and window."""
    calls = [(_mono(), _square(40 * 512, 700, 900))]
    a, ya, ca = _collect(ge._hip, calls, 2, 512, capture_history_blocks=0)
    b, yb, cb = _collect(ge._hip, calls, 2, 512)
    c, yc, cc = _collect(ge._hip, calls, 2, 512, event_history_blocks=64)
    assert a == b == c and len([1 for k, _ in a if k == "capture"]) >= 10
    assert ya.tobytes() == yb.tobytes() == yc.tobytes()
    assert ca.runtime.event_window_blocks() == cb.runtime.event_window_blocks() == cc.runtime.event_window_blocks() == 1


def test_plain_relay_on_a_history_node(gpu_required):
    """A live Runtime renders single blocks and relays (not blockwise) after every third: with the larger ring the plain relay fetches
    what the reference's positions name from behind the absolute count — the events of the same run without the option."""
    from elementary_amd.runtime import Runtime
    bs, blocks = 128, 60
    x = np.stack([lcg_noise_fast(blocks * bs, 3, 0.5), _square(blocks * bs, 160, 160)])     # (the graph reads inputs 0 and 1)
    logs = []
    for option in (64, None):
        rt = Runtime(48000.0, bs, device=0)
        if option is not None:
            rt.set_option("capture_history_blocks", option)
        assert rt.render(*_mono()())["result"] == 0
        log = []
        for k in range(blocks):
            rt.process(x[:, k * bs:(k + 1) * bs], 2, bs)
            if k % 3 == 2:
                log += list(rt.process_queued_events())
        assert rt.event_window_blocks() == (option or 1)
        logs.append(log)
    assert logs[0] == logs[1]
    takes = [p for k, p in logs[0] if k == "capture"]
    assert len(takes) >= 15 and sum(len(p["data"]) for p in takes) >= 22 * 160
