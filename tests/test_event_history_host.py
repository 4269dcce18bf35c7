"""Option "event_history_blocks" without a GPU: the relay's replay of the reference's analyzer ring (elementary_amd/csrc/
event_replay.h, compiled for the host) against a direct model of that ring and against the fft recordings, and the relay window
a dry engine handle reports with the option on and off."""
import tempfile

import pytest

import event_history_cases as eh
import fft_cases as fc

BLOCKS = 200
# (block, size, comparison): sizes above and below the block, both comparisons, a size the ring can never hold, a block that is
# no power of two. (512, 256, *) overrun from about block 32 on: every block brings 512 frames and a relay takes 256.
CASES = [(128, 256, eh.MORE_THAN), (512, 256, eh.MORE_THAN), (512, 256, eh.AT_LEAST), (512, 4096, eh.AT_LEAST),
         (512, 8192, eh.AT_LEAST), (700, 512, eh.MORE_THAN)]


@pytest.fixture(scope="module")
def replay():
    with tempfile.TemporaryDirectory() as d:
        r = eh.Replay(d)
        yield r
        r.close()


def _in_windows(replay, block, size, cmp, blocks, window):
    """The run as windows of `window` blocks, the end positions of each carried into the next: [(block, first frame)], end."""
    pos, out, at = (0, 0), [], 0
    while at < blocks:
        n = min(window, blocks - at)
        ev, pos = replay.window(pos, block, size, cmp, n)
        out += [(at + b, first) for b, first in ev]
        at += n
    return out, pos


@pytest.mark.parametrize("block,size,cmp", CASES)
def test_replay_equals_a_direct_model_of_the_ring(replay, block, size, cmp):
    """200 blocks, a read attempt after each: the header's (block, first frame) list and end positions are the model's, whether
    the run is replayed as one window, as windows of 7 blocks or block by block."""
    want, want_end = eh.model_events(block, size, cmp, BLOCKS)
    for window in (1, 7, BLOCKS):
        got, end = _in_windows(replay, block, size, cmp, BLOCKS, window)
        assert got == want, (window, got[:5], want[:5])
        assert end == want_end, (window, end, want_end)
    if size == 8192:
        assert want == []                                  # the ring holds 8191 frames at most
    elif size < block:
        # the overrun regime (from about block 30 on): an event per block, each starting 8191 frames before its block's end
        assert len(want) == BLOCKS
        late = [(b, first) for b, first in want if b >= 40]
        assert late and all(first == (b + 1) * block - 8191 for b, first in late), late[:3]
        assert any(want[i + 1][1] != want[i][1] + size for i in range(len(want) - 1))      # frames were skipped
    else:
        assert len(want) > 10 and all(want[i + 1][1] == want[i][1] + size for i in range(len(want) - 1))   # nothing skipped


@pytest.mark.parametrize("name", sorted(fc.manifest()["scenarios"]))
def test_replay_reproduces_the_recorded_fft_events(replay, name):
    """Every recorded scenario from (0, 0): the replay names the block and the first input frame of every recorded fft event. A
    scenario relayed after every third block reads once per three blocks (a write of three blocks' frames where nothing overruns);
    one that changes `size` is two windows, the second from the first's end positions; two fft nodes are two rings."""
    man = fc.manifest()
    sc = man["scenarios"][name]
    every, bs = int(sc["relay_every"]), int(sc["block"])
    for k, node in enumerate(sc["ffts"]):
        source = node["props"].get("name")
        want = [(e["block"], e["frame"], e["size"]) for e in fc.fft_events(sc) if e["source"] == source]
        cuts = sorted({ch["after_block"] + 1 for ch in sc["changes"] if ch["id"] == node["id"] and ch["key"] == "size"}) + [sc["blocks"]]
        size, pos, at, got = node["props"].get("size", 1024), (0, 0), 0, []
        for cut in cuts:
            assert (cut - at) % every == 0
            ev, pos = replay.window(pos, bs * every, size, eh.AT_LEAST, (cut - at) // every)
            got += [(at + (b + 1) * every - 1, first, size) for b, first in ev]
            for ch in sc["changes"]:
                if ch["id"] == node["id"] and ch["key"] == "size" and ch["after_block"] + 1 == cut:
                    size = ch["value"]
            at = cut
        assert got == want, (name, k, got[:4], want[:4])
        assert pos[0] == sc["blocks"] * bs


def _window(bs, option, roots):
    from elementary_amd.runtime import Runtime
    rt = Runtime(48000.0, bs, device=-1)
    if option is not None:
        rt.set_option("event_history_blocks", option)
    assert rt.render(*roots())["result"] == 0
    return rt.event_window_blocks()


def test_window_of_a_dry_handle_with_and_without_history():
    """A scope or fft made under the option serves a window of that many blocks whatever its `size`; without it the 8192-frame
    rule holds: floor((8191 - 256) / 128) = 61 blocks, one block when `size` is below the block. A capture node keeps its one."""
    from elementary_amd import el
    x = lambda: el.in_({"channel": 0})
    scope = lambda: [el.scope({"name": "sc", "size": 256}, x())]
    fft = lambda: [el.fft({"name": "f", "size": 256}, x())]
    capture = lambda: [el.capture({"name": "c"}, el.train(2.0), x())]
    assert _window(128, 256, scope) == 256 and _window(512, 256, scope) == 256
    assert _window(128, 0, scope) == 61 and _window(512, 0, scope) == 1
    assert _window(128, None, scope) == 61 and _window(512, None, scope) == 1
    assert _window(512, 256, fft) == 256 and _window(512, 0, fft) == 1
    assert _window(128, 96, fft) == 96 and _window(128, 0, fft) == (8192 - 256) // 128
    assert _window(512, 256, capture) == 1 and _window(512, 0, capture) == 1
    assert _window(512, 256, lambda: scope() + capture()) == 1
    # clamped like the other options; the readout logs bound it in host blocks of several slices
    assert _window(512, 5000, scope) == 1024 and _window(512, -3, scope) == 1
    assert _window(1024, 1024, scope) == 512
    # the option reaches nodes made AFTER it: a node that exists keeps its 8192-frame ring
    from elementary_amd.runtime import Runtime
    rt = Runtime(48000.0, 128, device=-1)
    assert rt.render(*scope())["result"] == 0
    rt.set_option("event_history_blocks", 256)
    assert rt.render(*scope())["result"] == 0 and rt.event_window_blocks() == 61
    assert rt.render(el.scope({"name": "other", "size": 512}, x()))["result"] == 0 and rt.event_window_blocks() == 256


def test_plan_digests_do_not_move_with_the_option_on():
    """The ring's mask lives in the node's record, not in the program: every node case of the plan corpus plans to the recorded
    digest with the option on, and a scope / fft graph plans to the same digest with and without it."""
    import plan_corpus
    from cases import NODE_CASES, node_case_resources
    from elementary_amd import el
    want = plan_corpus.recorded()
    for name in sorted(NODE_CASES):
        rt = plan_corpus._dry(44100.0, event_history_blocks=1024)
        for rname, data in node_case_resources().items():
            assert rt.add_shared_resource(rname, data)
        assert plan_corpus._render(rt, *NODE_CASES[name][0]()) == want["node/" + name], name

    def analyzers():
        x = el.in_({"channel": 0})
        return [el.scope({"name": "sc", "size": 256, "channels": 2}, x, el.mul(0.5, x)), el.fft({"name": "f", "size": 512}, x), el.meter({"name": "m"}, x)]
    for spec in (0, 2):
        on = plan_corpus._render(plan_corpus._dry(48000.0, specialize=spec, event_history_blocks=1024), *analyzers())
        off = plan_corpus._render(plan_corpus._dry(48000.0, specialize=spec), *analyzers())
        assert on == off, spec
