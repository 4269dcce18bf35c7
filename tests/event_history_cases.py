"""What the event-history tests share: a direct model of the reference's analyzer ring, and the native replay driver.

`RingModel` is runtime/elem/MultiChannelRingBuffer.h:34-83 as written there — an 8192-slot array, a write and a read position —
holding ABSOLUTE frame numbers instead of samples, so that a read tells which input frames it handed on. `model_events` drives it
the way the reference's offline caller does: a block written, one read attempt (offline-renderer/index.ts:112-120).
"""
from __future__ import annotations

import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORE_THAN, AT_LEAST = 0, 1        # scope: size() > size (Analyzers.h:192-245); fft: size() >= size (wasm/FFT.h:96)


class RingModel:
    CAP = 8192

    def __init__(self):
        self.buf = np.full(self.CAP, -1, np.int64)       # (never-written slots: the ring's initial zeros)
        self.w = 0
        self.r = 0
        self.written = 0

    def _full(self):
        return self.w - self.r if self.w > self.r else (self.CAP - (self.r - self.w)) & (self.CAP - 1)

    def _free(self):
        return self.r - self.w if self.r > self.w else self.CAP - (self.w - self.r)

    def write(self, n):                                   # :34-57
        move = n >= self._free()
        idx = (self.w + np.arange(n)) & (self.CAP - 1)
        self.buf[idx] = self.written + np.arange(n)
        self.written += n
        self.w = (self.w + n) & (self.CAP - 1)
        if move:
            self.r = (self.w + 1) & (self.CAP - 1)

    def read(self, size, cmp):                            # the node's comparison, then :59-83
        full = self._full()
        if not (full >= size if cmp == AT_LEAST else full > size):
            return None
        got = self.buf[(self.r + np.arange(size)) & (self.CAP - 1)]
        self.r = (self.r + size) & (self.CAP - 1)
        return got


def model_events(block, size, cmp, blocks):
    """[(block, first frame)] of a per-block relay over `blocks` blocks from an empty ring, and the (written, read) it ends at.
    Every frame a read hands on is checked to be `size` CONTIGUOUS input frames: that is what lets the relay name it by its first."""
    ring, out = RingModel(), []
    for b in range(blocks):
        ring.write(block)
        got = ring.read(size, cmp)
        if got is not None:
            assert got[0] >= 0 and np.array_equal(got, got[0] + np.arange(size)), (b, got[:4])
            out.append((b, int(got[0])))
    return out, (ring.written, ring.r)


def cxx():
    for c in (shutil.which("c++"), shutil.which("g++"), "/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    return None


class Replay:
    """tests/native/event_replay_host.cpp, built into `workdir` and kept running: `window(...)` replays one relay window."""

    def __init__(self, workdir):
        compiler = cxx()
        assert compiler, "a C++17 compiler builds the replay driver"
        exe = os.path.join(workdir, "event_replay_host")
        subprocess.run([compiler, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "elementary_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "event_replay_host.cpp"), "-o", exe], check=True)
        self.p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)

    def window(self, pos, block, size, cmp, blocks):
        """-> ([(block of the window, first frame)], end positions)"""
        self.p.stdin.write(f"{pos[0]} {pos[1]} {block} {size} {cmp} {blocks}\n")
        self.p.stdin.flush()
        out = []
        while True:
            t = self.p.stdout.readline().split()
            assert t, "the replay driver ended early"
            if t[0] == "end":
                return out, (int(t[1]), int(t[2]))
            out.append((int(t[1]), int(t[2])))

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=10)
