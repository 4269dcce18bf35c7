"""The event relay's host-block arithmetic without a GPU: elementary_amd/csrc/event_fold.h, compiled for the host (tests/native/
event_fold_host.cpp, built the way event_history_cases.py builds the replay driver), against a few lines of Python that restate
each rule — the host block of an engine block, the meter and snapshot folds, the scope's run coalescing, the capture ring's fill."""
import bisect
import os
import struct
import subprocess
import tempfile

import pytest

import event_history_cases as eh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSLICED3 = (False, 3, [])
# host block 1024 over engine block 512: two host blocks of two slices, then one the window's end cut after its first slice
SLICED = (True, 5, [2, 4, 5])
GAP = 4096


def f2u(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def u2f(u):
    return struct.unpack("<f", struct.pack("<I", u))[0]


class Fold:
    def __init__(self, workdir):
        compiler = eh.cxx()
        assert compiler, "a C++17 compiler builds the fold driver"
        exe = os.path.join(workdir, "event_fold_host")
        subprocess.run([compiler, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "elementary_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "event_fold_host.cpp"), "-o", exe], check=True)
        self.p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)

    def ask(self, *words, until_end=False):
        self.p.stdin.write(" ".join(str(int(w)) if not isinstance(w, str) else w for w in words) + "\n")
        self.p.stdin.flush()
        out = []
        while True:
            t = self.p.stdout.readline().split()
            assert t, "the fold driver ended early"
            out.append(t)
            if not until_end or t[0] == "end":
                return out

    @staticmethod
    def win(w):
        sliced, blocks, ends = w
        return [int(sliced), blocks, len(ends)] + list(ends)

    def block_of(self, w, from_end):
        return int(self.ask("block", *self.win(w), from_end)[0][0])

    def meter(self, w, entries, blockwise):
        flat = [f2u(x) for e in entries for x in e]
        out = self.ask("meter", *self.win(w), int(blockwise), len(entries), *flat, until_end=True)
        return [(int(t[1]), u2f(int(t[2])), u2f(int(t[3]))) for t in out[:-1]]

    def snapshot(self, w, blk, entries):
        flat = [x for (at, value, pushes) in entries for x in (at, f2u(value), pushes)]
        out = self.ask("snap", *self.win(w), blk, len(entries), *flat, until_end=True)
        return [(int(t[1]), u2f(int(t[2]))) for t in out[:-1]]

    def scope(self, size, emits):
        out = self.ask("scope", size, len(emits), *[x for e in emits for x in e], until_end=True)
        runs = [tuple(int(x) for x in t[1:]) for t in out if t[0] == "r"]
        ems = [tuple(int(x) for x in t[1:]) for t in out if t[0] == "e"]
        return runs, ems, int(out[-1][1])

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=10)


@pytest.fixture(scope="module")
def fold():
    with tempfile.TemporaryDirectory() as d:
        f = Fold(d)
        yield f
        f.close()


# ---- the rules, restated ----
def model_block(w, from_end):
    sliced, blocks, ends = w
    last = blocks - 1 if blocks else 0
    s = 0 if from_end > last else last - from_end
    return bisect.bisect_right(ends, s) if sliced else s      # host blocks that ended at or before slice s


def model_wraps(pushes):
    return pushes != 0 and pushes % 32 == 0


def model_meter(w, entries, blockwise):
    groups = []
    for k, (mn, mx) in enumerate(entries):
        b = model_block(w, len(entries) - 1 - k)
        if groups and groups[-1][0] == b:
            groups[-1] = (b, min(groups[-1][1], mn), max(groups[-1][2], mx))
        else:
            groups.append((b, mn, mx))
    if blockwise:
        return groups
    return [] if not groups or model_wraps(len(groups)) else [groups[-1]]


def model_snapshot(w, blk, entries):
    per_block = {}
    for at, value, pushes in entries:
        b = model_block(w, (blk - 1 - at) & 0xFFFFFFFF)
        newest, total = per_block.get(b, (None, 0))
        per_block[b] = (value, total + pushes)
    return [(b, v) for b, (v, total) in sorted(per_block.items()) if not model_wraps(total)]


def model_runs(size, emits):
    runs, out = [], []
    for block, first in emits:
        if not runs or first < runs[-1][0] or first > runs[-1][0] + runs[-1][1] + GAP:
            runs.append([first, 0])
        runs[-1][1] = max(runs[-1][1], first + size - runs[-1][0])
        out.append((block, first, len(runs) - 1))
    return runs, out


# ---- host block of an engine block ----
def test_host_block_unsliced_window_of_three(fold):
    for from_end, want in ((0, 2), (1, 1), (2, 0)):
        assert fold.block_of(UNSLICED3, from_end) == want == model_block(UNSLICED3, from_end)


def test_host_block_sliced_with_a_cut_last_block(fold):
    got = [fold.block_of(SLICED, k) for k in range(6)]
    assert got == [model_block(SLICED, k) for k in range(6)]
    assert got == [2, 1, 1, 0, 0, 0]          # slices 4 | 3 2 | 1 0, and one past the window's start


def test_host_block_beyond_the_window_clamps_to_slice_zero(fold):
    for w in (UNSLICED3, SLICED):
        for from_end in (7, 1000, 2 ** 40):
            assert fold.block_of(w, from_end) == 0 == model_block(w, from_end)


# ---- meter ----
def test_meter_six_entries_over_the_sliced_window(fold):
    entries = [(-0.5, 0.25), (-0.125, 0.5), (-0.75, 0.125), (-1.0, 1.0), (-2.0, 0.5), (-0.25, 3.0)]
    want = model_meter(SLICED, entries, True)
    assert fold.meter(SLICED, entries, True) == want
    assert want == [(0, -0.75, 0.5), (1, -2.0, 1.0), (2, -0.25, 3.0)]       # three groups, min / max folded per group
    assert fold.meter(SLICED, entries, False) == [want[-1]] == model_meter(SLICED, entries, False)


@pytest.mark.parametrize("groups", [32, 33])
def test_meter_plain_relay_and_the_32_push_rule(fold, groups):
    w = (False, groups, [])
    entries = [(-float(k + 1), float(k + 1)) for k in range(groups)]
    got = fold.meter(w, entries, False)
    assert got == model_meter(w, entries, False)
    assert got == ([] if groups == 32 else [(32, -33.0, 33.0)])             # 32 groups: nothing; 33: the newest alone


def test_meter_blockwise_emits_all_groups(fold):
    w = (False, 32, [])
    entries = [(-float(k + 1), float(k + 1)) for k in range(32)]
    got = fold.meter(w, entries, True)
    assert got == model_meter(w, entries, True) == [(k, -float(k + 1), float(k + 1)) for k in range(32)]


# ---- snapshot ----
def test_snapshot_fold_per_host_block(fold):
    # the node's block counter stands at 105 after the window's five slices 100 .. 104: host blocks {100, 101} {102, 103} {104}
    blk = 105
    entries = [(100, 1.5, 3), (101, 2.5, 4),      # one host block, two latches: the newest value, 7 pushes
               (102, 3.5, 20), (103, 4.5, 12),    # 32 pushes in one host block: the reference's queue reads as empty
               (104, 5.5, 31)]                    # its neighbour with 31 is kept
    got = fold.snapshot(SLICED, blk, entries)
    assert got == model_snapshot(SLICED, blk, entries)
    assert got == [(0, 2.5), (2, 5.5)]
    # unsliced, the same entries are a block each: nothing sums to 32, every latch is relayed
    w = (False, 5, [])
    assert fold.snapshot(w, blk, entries) == model_snapshot(w, blk, entries) == [(k, 1.5 + k) for k in range(5)]
    one = [(102, 3.5, 32), (103, 4.5, 31)]
    assert fold.snapshot(w, blk, one) == model_snapshot(w, blk, one) == [(3, 4.5)]


# ---- scope runs ----
SIZE = 256
SCOPE_CASES = {
    "contiguous": [(0, 0), (1, 256), (2, 512)],
    "gap_of_4096_is_fetched_along": [(0, 0), (1, 256), (2, 512 + GAP)],
    "gap_of_4097_starts_a_run": [(0, 0), (1, 256), (2, 512 + GAP + 1)],
    "an_earlier_frame_starts_a_run": [(0, 9000), (1, 9256), (2, 8000), (3, 8256)],
}


@pytest.mark.parametrize("name", sorted(SCOPE_CASES))
def test_scope_runs(fold, name):
    emits = SCOPE_CASES[name]
    runs, ems, span = fold.scope(SIZE, emits)
    want_runs, want_emits = model_runs(SIZE, emits)
    assert [(first, frames) for first, frames, at in runs] == [tuple(r) for r in want_runs]
    assert [(b, first, run) for b, first, run, off in ems] == want_emits
    assert len(runs) == {"contiguous": 1, "gap_of_4096_is_fetched_along": 1, "gap_of_4097_starts_a_run": 2,
                         "an_earlier_frame_starts_a_run": 2}[name]
    # the fetched buffer holds the runs back to back: every emit's offset lands on its own frame
    fetched = [f for first, frames, at in runs for f in range(first, first + frames)]
    assert span == len(fetched) and [at for first, frames, at in runs] == [sum(r[1] for r in runs[:k]) for k in range(len(runs))]
    for b, first, run, off in ems:
        assert fetched[off:off + SIZE] == list(range(first, first + SIZE))


# ---- capture ----
@pytest.mark.parametrize("w,r,want", [(5, 2, 3), (1, 6, 3), (4, 4, 0)])
def test_capture_avail(fold, w, r, want):
    cap = 8
    model = w - r if w > r else (cap - (r - w)) & (cap - 1)
    assert int(fold.ask("avail", w, r, cap - 1)[0][0]) == model == want


def test_wraps_to_empty(fold):
    for pushes in (0, 1, 31, 32, 33, 64, 96, 1000):
        assert int(fold.ask("wraps", pushes)[0][0]) == int(model_wraps(pushes))
