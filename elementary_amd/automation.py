"""Breakpoint automation lanes (``Runtime.automation``, ``OfflineRenderer.automate``): helpers that build lists of points, and the
value rule in plain Python.

A lane is a list of ``(frame, value, curve)`` points sorted by frame, ``curve`` ``"hold"`` (0) or ``"linear"`` (1), bound to one engine
input channel. Its value at absolute engine frame ``t``, with ``i`` the last point whose frame is ``<= t``:

* ``t`` before the first point: the first value; ``i`` the last point: its value;
* ``hold``, or ``t`` exactly on point ``i``: ``value_i``, bit for bit;
* ``linear``: ``a + (b - a) * ((t - f_i) / (f_next - f_i))`` in float64 with ``a = value_i`` and ``b = value_{i+1}``, rounded once to
  float32.

Several points on one frame make a jump: the last of them is the value from that frame on, the first of them is what a ramp into that
frame aims at. ``value`` below is that rule without numpy; the engine's kernel and ``runtime.automation_host`` give the same bits.
"""
from __future__ import annotations

import struct
from typing import Iterable, List, Sequence, Tuple

HOLD, LINEAR = 0, 1
MAX_CHANNELS = 32
MAX_POINTS = 1 << 20
MAX_SEGMENT = 1 << 52
_CURVES = {"hold": HOLD, "linear": LINEAR, HOLD: HOLD, LINEAR: LINEAR}

Point = Tuple[int, float, int]


def curve_code(curve) -> int:
    """``"hold"`` / ``"linear"`` (or 0 / 1) as the code the engine takes."""
    try:
        return _CURVES[curve]
    except (KeyError, TypeError):
        raise ValueError(f"a curve is 'hold' or 'linear', got {curve!r}") from None


def normalise(points: Iterable[Sequence]) -> List[Point]:
    """``(frame, value[, curve])`` rows (curve default ``"hold"``) as ``(int frame, float value, code)`` tuples, in the order given."""
    out = []
    for p in points:
        p = tuple(p)
        if len(p) not in (2, 3):
            raise ValueError(f"a point is (frame, value) or (frame, value, curve), got {p!r}")
        out.append((int(p[0]), float(p[1]), curve_code(p[2]) if len(p) == 3 else HOLD))
    return out


def ramp(t0: int, v0: float, t1: int, v1: float) -> List[Point]:
    """``v0`` up to ``t0``, a straight line to ``v1`` at ``t1``, ``v1`` from there on."""
    if t1 < t0:
        raise ValueError("a ramp ends at or behind its start")
    return [(int(t0), float(v0), LINEAR), (int(t1), float(v1), HOLD)]


def steps(times: Sequence[int], values: Sequence[float]) -> List[Point]:
    """``values[k]`` from ``times[k]`` until ``times[k + 1]`` (the first value also in front of ``times[0]``)."""
    if len(times) != len(values):
        raise ValueError("as many times as values")
    return [(int(t), float(v), HOLD) for t, v in zip(times, values)]


def to_frames(points: Iterable[Sequence], sample_rate: float) -> List[Point]:
    """Points whose first entry is seconds as points in frames: ``round(seconds * sample_rate)``."""
    return [(int(round(float(p[0]) * float(sample_rate))),) + tuple(p[1:]) for p in points]


def _f32(x: float) -> float:
    return struct.unpack("<f", struct.pack("<f", x))[0]


def segment_at(points: Sequence[Point], t: int) -> int:
    """The index of the last point whose frame is ``<= t``; -1 before the first."""
    lo, hi = 0, len(points)
    while lo < hi:
        mid = (lo + hi) // 2
        if points[mid][0] <= t:
            lo = mid + 1
        else:
            hi = mid
    return lo - 1


def value(points: Sequence[Point], t: int) -> float:
    """The lane's value at frame ``t`` (a Python float holding the float32)."""
    pts = normalise(points)
    i = segment_at(pts, t)
    if i < 0:
        return _f32(pts[0][1])
    f, v, c = pts[i]
    if i + 1 >= len(pts) or c == HOLD or t == f:
        return _f32(v)
    a, b = _f32(v), _f32(pts[i + 1][1])
    u = float(t - f) / float(pts[i + 1][0] - f)
    return _f32(a + (b - a) * u)
