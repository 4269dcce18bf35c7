"""Option "capture_history_blocks" without a GPU: the relay's replay of a capture node's per-block log (elementary_amd/csrc/
capture_replay.h, compiled for the host) against a direct model of the reference's CaptureNode under a relay after every block,
the relay window a dry engine handle reports with the option on and off, and the plan digests with the option on."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import event_history_cases as eh


def model(gate, block):
    """builtins/Capture.h:21-95 driven as the offline renderer drives it (index.ts:112-120): `block` samples, then processEvents.
    Recorded samples are numbered in the order they are recorded, so the scratch holds [flushed, flushed + scratch), the ring what
    was flushed and not drained, the relay buffer [first, drained). -> takes [(block, first frame, length)], and per block what the
    kernels log: (frames handed to the ring by its end, the gate fell in it)."""
    prev, scratch, flushed, drained, first, takes, log = 0.0, 0, 0, 0, 0, [], []
    for b in range(len(gate) // block):
        ready = False
        for g in gate[b * block:(b + 1) * block]:
            falling = (g - prev) < -0.5
            prev = g
            if falling or scratch >= 128:                  # :43-52
                flushed, scratch = flushed + scratch, 0
                ready = ready or falling
            if g:                                          # :55-57
                scratch += 1
        drained = flushed                                  # :62-72 (a block never overruns the ring of bitceil(sr) frames)
        log.append((flushed, ready))
        if ready:                                          # :74-94
            takes.append((b, first, drained - first))
            first = drained
    return takes, log


def gate_runs(frames, mean_run, seed):
    """A 0/1 gate of `frames` samples made of runs with random lengths around `mean_run`."""
    rng = np.random.default_rng(seed)
    out, level = [], 0.0
    while sum(len(r) for r in out) < frames:
        out.append(np.full(int(rng.integers(1, 2 * mean_run)), level))
        level = 1.0 - level
    return np.concatenate(out)[:frames]


class Replay:
    """tests/native/capture_replay_host.cpp, built into `workdir` and kept running: `window(...)` replays one relay window."""

    def __init__(self, workdir):
        compiler = eh.cxx()
        assert compiler, "a C++17 compiler builds the replay driver"
        exe = os.path.join(workdir, "capture_replay_host")
        subprocess.run([compiler, "-std=c++17", "-O1", "-I", os.path.join(eh.ROOT, "elementary_amd", "csrc"),
                        os.path.join(eh.ROOT, "tests", "native", "capture_replay_host.cpp"), "-o", exe], check=True)
        self.p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)

    def window(self, relayed, pending, per_host, entries):
        """entries: [(block counter, F mod 2^32, E)] per engine block -> ([(host block of the window, take end)], frames relayed)"""
        self.p.stdin.write(f"{relayed} {int(pending)} {per_host} {len(entries)} " + " ".join(f"{b} {f} {int(e)}" for b, f, e in entries) + "\n")
        self.p.stdin.flush()
        out = []
        while True:
            t = self.p.stdout.readline().split()
            assert t, "the replay driver ended early"
            if t[0] == "end":
                return out, int(t[1])
            out.append((int(t[1]), int(t[2])))

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=10)


@pytest.fixture(scope="module")
def replay():
    with tempfile.TemporaryDirectory() as d:
        r = Replay(d)
        yield r
        r.close()


def _in_windows(replay, log, window, per_host=1, offset=0):
    """The logged run as windows of `window` HOST blocks, the relayed count carried from one into the next; the device counts frames
    mod 2^32 from `offset`. -> takes [(host block, first frame, length)]"""
    relayed, last, takes, at = offset, offset, [], 0
    entries = [(k, (offset + f) & 0xFFFFFFFF, e) for k, (f, e) in enumerate(log)]
    while at < len(entries):
        chunk = entries[at:at + window * per_host]
        got, relayed = replay.window(relayed, False, per_host, chunk)
        for b, end in got:
            takes.append((at // per_host + b, last - offset, end - last))
            last = end
        at += len(chunk)
    assert relayed - offset == log[-1][0]
    return takes


# (block, mean run of the gate): no fall in most blocks, about one, several — at both block sizes
GATES = [(64, 700), (64, 40), (64, 5), (512, 6000), (512, 300), (512, 24)]


@pytest.mark.parametrize("block,mean_run", GATES)
def test_replay_equals_a_model_of_the_reference_node(replay, block, mean_run):
    """192 blocks of a random 0/1 gate: the takes the header names from the per-block log are the model's, one for one — block,
    first frame and length — whether the run is replayed block by block, in windows of 7 or of 96 blocks (takes span windows), and
    with the device's frame counter wrapping 2^32 on the way."""
    gate = gate_runs(192 * block, mean_run, 1000 + block + mean_run)
    if mean_run > block:
        gate[96 * block - 300:96 * block + 300] = 1.0          # high across the boundary of the two windows of 96
    want, log = model(gate, block)
    falls = [sum(1 for i in range(b * block, (b + 1) * block) if i and gate[i] < gate[i - 1]) for b in range(192)]
    assert len(want) >= 3
    if mean_run * 4 < block:
        assert min(falls[1:]) >= 2 and len(want) >= 191      # several falling edges in every block: one event per block
    elif mean_run > block:
        assert len(want) < 96 and falls.count(0) > 96        # most blocks see none
        # a take that spans two windows of 96 blocks: handed to the ring in the first, its event in the second
        assert any(b >= 96 and first < log[95][0] for b, first, n in want)
        assert any(n > 128 for _, _, n in want)              # (longer than the scratch: flushed in pieces)
    else:
        assert 0 < falls.count(0) < 150 and max(falls) >= 2  # none, one and several
    for window in (1, 7, 96):
        assert _in_windows(replay, log, window) == want, window
    assert _in_windows(replay, log, 7, offset=2 ** 32 - want[1][1] - 5) == want


@pytest.mark.parametrize("mean_run", [2000, 300, 24])
def test_replay_of_a_sliced_host_block(replay, mean_run):
    """A host block of 1024 frames renders as two engine blocks of 512 with a log entry each; the reference's node sees one block:
    F of a host block is its last slice's, E the OR of its slices' — the model at 1024 frames, the log from the model at 512."""
    gate = gate_runs(96 * 1024, mean_run, 77 + mean_run)
    want, _ = model(gate, 1024)
    _, log = model(gate, 512)
    for window in (1, 7, 96):
        assert _in_windows(replay, log, window, per_host=2) == want, window
    if mean_run > 100:
        assert any(log[2 * h][1] and not log[2 * h + 1][1] for h in range(96))  # a fall in the first slice alone still counts


def test_replay_corner_cases(replay):
    """A ready flag carried into the window goes out with its first block; a counter logged before a plain relay drained past it
    brings nothing; no blocks, no takes."""
    assert replay.window(100, True, 1, [(0, 140, 0), (1, 300, 0)]) == ([(0, 140)], 300)
    assert replay.window(100, False, 1, [(0, 140, 0), (1, 300, 1), (2, 300, 1)]) == ([(1, 300), (2, 300)], 300)
    assert replay.window(500, False, 1, [(0, 140, 1), (1, 620, 0)]) == ([(0, 500)], 620)
    assert replay.window(7, True, 1, []) == ([], 7)


def _window(bs, options, roots):
    from elementary_amd.runtime import Runtime
    rt = Runtime(48000.0, bs, device=-1)
    for k, v in options.items():
        rt.set_option(k, v)
    assert rt.render(*roots())["result"] == 0
    return rt.event_window_blocks()


def test_window_of_a_dry_handle_with_and_without_capture_history():
    """A capture node made under "capture_history_blocks" serves a window of that many blocks, alone or beside a scope made under
    "event_history_blocks"; without it — unset, 0, or "event_history_blocks" alone — the window stays one block."""
    from elementary_amd import el
    from elementary_amd.runtime import Runtime
    x = lambda: el.in_({"channel": 0})
    capture = lambda: [el.capture({"name": "c"}, el.train(2.0), x())]
    mc = lambda: el.mc.capture({"name": "m", "channels": 2}, el.train(2.0), x(), el.mul(0.5, x()))
    both = lambda: [el.scope({"name": "sc", "size": 256}, x())] + capture()
    assert _window(512, {"capture_history_blocks": 256}, capture) == 256
    assert _window(512, {"capture_history_blocks": 256}, mc) == 256
    assert _window(512, {"capture_history_blocks": 256, "event_history_blocks": 256}, both) == 256
    assert _window(512, {"capture_history_blocks": 256, "event_history_blocks": 64}, both) == 64
    assert _window(512, {"capture_history_blocks": 256}, both) == 1             # (the scope of 256 frames at block 512 wants its own option)
    assert _window(512, {"capture_history_blocks": 0}, capture) == 1 and _window(512, {}, capture) == 1
    assert _window(512, {"event_history_blocks": 256}, capture) == 1
    assert _window(512, {"event_history_blocks": 256}, both) == 1
    # clamped like the other option; the per-block logs bound it in host blocks of several slices
    assert _window(512, {"capture_history_blocks": 5000}, capture) == 1024 and _window(512, {"capture_history_blocks": -3}, capture) == 1
    assert _window(1024, {"capture_history_blocks": 1024}, capture) == 512
    # the option reaches nodes made AFTER it: a node that exists keeps its ring and its window of one
    rt = Runtime(48000.0, 512, device=-1)
    assert rt.render(*capture())["result"] == 0
    rt.set_option("capture_history_blocks", 256)
    assert rt.render(*capture())["result"] == 0 and rt.event_window_blocks() == 1
    assert rt.render(el.capture({"name": "other"}, el.train(3.0), x()))["result"] == 0 and rt.event_window_blocks() == 256


def test_plan_digests_do_not_move_with_the_capture_option_on():
    """The ring's masks and the log's live in the node's record, not in the program: the corpus cases that hold capture nodes plan
    to the recorded digests with the option on, and a capture graph plans to the same digest with and without it."""
    import plan_corpus
    from cases import NODE_CASES, node_case_resources
    from elementary_amd import el
    want = plan_corpus.recorded()
    for name in ("capture", "mc_capture"):
        rt = plan_corpus._dry(44100.0, capture_history_blocks=1024)
        for rname, data in node_case_resources().items():
            assert rt.add_shared_resource(rname, data)
        assert plan_corpus._render(rt, *NODE_CASES[name][0]()) == want["node/" + name], name

    def captures():
        x = el.in_({"channel": 0})
        g = el.ge(el.in_({"channel": 1}), 0.5)
        return [el.capture({"name": "c"}, g, x), el.meter({"name": "m"}, x)] + el.mc.capture({"name": "mc", "channels": 2}, g, x, el.mul(0.5, x))
    for spec in (0, 2):
        on = plan_corpus._render(plan_corpus._dry(48000.0, specialize=spec, capture_history_blocks=1024), *captures())
        off = plan_corpus._render(plan_corpus._dry(48000.0, specialize=spec), *captures())
        assert on == off, spec
