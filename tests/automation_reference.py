"""A numpy float64 restatement of the automation value rule (include/elemhip.h, "breakpoint automation"). It does not import the
library: tests compare the library's bits with these.

A lane is a list of (frame, value, curve) rows sorted by frame, curve 0 = hold, 1 = linear. With i the LAST point whose frame is <= t:
t before the first point gives the first value, i the last point its value, hold or t == frame_i gives value_i bit for bit, linear
gives a + (b - a) * ((t - f_i) / (f_{i+1} - f_i)) in float64 (a, b the float32 values widened), rounded once to float32. Of several
points on one frame the last is the value from that frame on and the first is what a ramp into the frame aims at.
"""
import numpy as np

HOLD, LINEAR = 0, 1


def segment_scan(points, t):
    """The index of the last point whose frame is <= t, by a linear scan; -1 before the first."""
    i = -1
    for k, p in enumerate(points):
        if int(p[0]) <= t:
            i = k
    return i


def values(points, t0, n):
    """float32 [n]: the lane's value at frames t0 .. t0 + n - 1."""
    frames = np.array([int(p[0]) for p in points], dtype=np.int64)
    vals = np.array([p[1] for p in points], dtype=np.float32)
    curves = np.array([int(p[2]) if len(p) > 2 else HOLD for p in points], dtype=np.int64)
    t = np.int64(t0) + np.arange(int(n), dtype=np.int64)
    i = np.searchsorted(frames, t, side="right") - 1          # the last point with frame <= t
    ic = np.clip(i, 0, len(frames) - 1)
    nxt = np.clip(ic + 1, 0, len(frames) - 1)
    a, b = vals[ic].astype(np.float64), vals[nxt].astype(np.float64)
    span = (frames[nxt] - frames[ic]).astype(np.float64)
    ramp = (i >= 0) & (ic + 1 < len(frames)) & (curves[ic] == LINEAR) & (t != frames[ic])
    u = np.divide((t - frames[ic]).astype(np.float64), span, out=np.zeros(len(t)), where=ramp)
    y = np.where(ramp, a + (b - a) * u, a)
    out = y.astype(np.float32)
    out[~ramp] = vals[ic][~ramp]                               # (bit for bit: a -0.0 stays a -0.0)
    return out


def dense(lanes, t0, n):
    """{channel: points} -> {channel: float32 [n]}."""
    return {c: values(p, t0, n) for c, p in lanes.items()}
