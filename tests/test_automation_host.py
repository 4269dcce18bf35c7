"""Breakpoint automation without a GPU: the scalar twin (elemhip_automation_host) against tests/automation_reference.py bit for bit, the
kernel's search (elemhip_automation_segment_at) against a linear scan, and validation and read-back on a dry engine handle."""
import numpy as np
import pytest

import automation_reference as ref
from elementary_amd import automation as au
from elementary_amd.runtime import ElemHipError, Runtime, automation_host, automation_segment_at

H, L = au.HOLD, au.LINEAR

CASES = {
    "single point": ([(10, 0.75, L)], [(-5, 40)]),
    "hold and linear": ([(0, 0.0, L), (100, 1.0, H), (150, -2.5, L), (157, 3.25, L), (300, 0.1, H)], [(-20, 360)]),
    "a point exactly on t": ([(0, 0.1, L), (7, 0.7, L), (8, -0.0, L), (9, 0.3, H)], [(7, 1), (8, 1), (9, 1), (0, 12)]),
    "two points on one frame": ([(0, 0.0, L), (50, 1.0, L), (50, 0.25, L), (90, 0.5, H)], [(-3, 100)]),
    "three points on one frame": ([(0, 0.0, L), (50, 1.0, H), (50, 9.0, L), (50, 0.25, L), (90, 0.5, H)], [(-3, 100)]),
    "several points on the first frame": ([(5, 1.0, L), (5, 2.0, L), (5, 3.0, L), (25, 4.0, H)], [(0, 40)]),
    "a breakpoint on every frame": ([(k, float(np.float32(np.sin(0.37 * k))), k % 2) for k in range(200)], [(-2, 210)]),
    "segments of length 1": ([(0, 0.0, L), (1, 1.0, L), (2, -1.0, L), (3, 0.5, H), (4, 0.25, L), (5, 8.0, L)], [(-1, 9)]),
    "around 2^32": ([((1 << 32) - 100, 0.0, L), ((1 << 32) + 155, 1.0, L), ((1 << 32) + 156, 0.5, H)], [((1 << 32) - 130, 320)]),
    "around 2^40": ([((1 << 40) - 3, -1.0, L), ((1 << 40) + 1000003, 1.0, H)], [((1 << 40) - 10, 300), ((1 << 40) + 999900, 200)]),
    "negative times": ([(-(1 << 35) - 50, 0.3, L), (-(1 << 35) + 77, -0.9, L), (-10, 0.9, L), (10, 0.0, H)], [(-(1 << 35) - 60, 200), (-30, 60)]),
    "denormals up to 1e30": ([(0, 1e-45, L), (40, 3e-39, L), (80, 1.1754944e-38, L), (120, 1e30, L), (160, -1e30, L), (200, -1e-42, H)], [(-5, 215)]),
    "a long segment": ([(0, 0.0, L), (1 << 52, 1.0, H)], [(0, 64), ((1 << 51) - 32, 64), ((1 << 52) - 64, 80)]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_equals_the_reference(name):
    """Bit for bit, over windows that reach in front of the first point and behind the last."""
    points, windows = CASES[name]
    for t0, n in windows:
        got = automation_host(points, t0, n)
        want = ref.values(points, t0, n)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (name, t0, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:5])


def test_on_a_point_is_the_point():
    """t == f_i gives v_i bit for bit — the last of the points on that frame, a negative zero included."""
    points = [(0, 0.1, L), (7, -0.0, L), (20, 0.3, L), (20, -7.5, L), (31, 1e-40, L), (40, 2.0, H)]
    for f, v in ((0, 0.1), (7, -0.0), (20, -7.5), (31, 1e-40), (40, 2.0)):
        assert automation_host(points, f, 1).tobytes() == np.array([v], dtype=np.float32).tobytes()
    assert automation_host(points, 19, 1)[0] != np.float32(-7.5)      # the ramp into frame 20 aims at 0.3


def test_python_value_rule_agrees():
    points, _ = CASES["three points on one frame"]
    want = ref.values(points, -3, 100)
    got = np.array([au.value(points, t) for t in range(-3, 97)], dtype=np.float32)
    assert got.tobytes() == want.tobytes()


def test_twin_is_cut_invariant():
    points, _ = CASES["hold and linear"]
    whole = automation_host(points, -20, 360)
    cuts = [0, 1, 64, 127, 128, 193, 360]
    parts = [automation_host(points, -20 + a, b - a) for a, b in zip(cuts, cuts[1:])]
    assert np.concatenate(parts).tobytes() == whole.tobytes()


def test_segment_at_agrees_with_a_linear_scan():
    rng = np.random.default_rng(5)
    frames = np.sort(rng.integers(-20, 280, size=90))          # many repeated frames among them
    points = [(int(f), float(k), k % 2) for k, f in enumerate(frames)]
    for t in range(-40, 260):
        assert automation_segment_at(points, t) == ref.segment_scan(points, t), t
    assert automation_segment_at(points[:1], points[0][0] - 1) == -1 and automation_segment_at(points[:1], points[0][0]) == 0


def _code(call):
    with pytest.raises(ElemHipError) as e:
        call()
    return e.value.code


REFUSED = {
    "unsorted": [(0, 0.0, H), (10, 1.0, H), (9, 2.0, H)],
    "nan": [(0, float("nan"), H)],
    "inf": [(0, 0.0, L), (5, float("inf"), H)],
    "float32 overflow": [(0, 1e39, H)],
    "curve 2": [(0, 0.0, 2)],
    "long linear segment": [(0, 0.0, L), ((1 << 52) + 1, 1.0, H)],
    "long linear segment across zero": [(-(1 << 62), 0.0, L), (1 << 62, 1.0, H)],
}


def test_refusals_answer_6_and_change_nothing():
    rt = Runtime(48000.0, 64, device=-1)
    kept = [(0, 0.5, L), (64, 1.0, H)]
    rt.automation(3, kept)
    for name, points in REFUSED.items():
        arr = points
        if name == "curve 2":      # (the Python layer has no name for it: straight to the C-ABI's code)
            from elementary_amd.runtime import _AutomationPoint
            raw = (_AutomationPoint * 1)()
            raw[0].frame, raw[0].value, raw[0].curve = 0, 0.0, 2
            assert rt._lib.elemhip_automation_set(rt._h, 3, raw, 1) == 6
            assert rt._lib.elemhip_automation_host(raw, 1, 0, 0, None) == 6
        else:
            assert _code(lambda: rt.automation(3, arr)) == 6, name
            assert _code(lambda: automation_host(arr, 0, 4)) == 6, name
        assert rt.automation_read(3)["points"] == [(0, 0.5, L), (64, 1.0, H)], name
    # zero points (to the twin) and more than 2^20
    from elementary_amd.runtime import _AutomationPoint
    raw = (_AutomationPoint * 1)()
    assert rt._lib.elemhip_automation_host(raw, 0, 0, 0, None) == 6
    many = (_AutomationPoint * ((1 << 20) + 1))()
    assert rt._lib.elemhip_automation_set(rt._h, 3, many, len(many)) == 6
    assert rt._lib.elemhip_automation_set(rt._h, 4, many, 1 << 20) == 0      # (2^20 points, all on frame 0: allowed)
    assert _code(lambda: rt.automation(32, kept)) == 6                       # channels 0 .. 31
    got = rt.automation_read(3)
    assert got["points"] == [(0, 0.5, L), (64, 1.0, H)] and got["channels"] == [3, 4] and got["inputs"] == 5
    # a hold segment may be as long as it likes
    rt.automation(4, [(-(1 << 62), 1.0, H), (1 << 62, 2.0, H)])
    assert rt.automation_read(4)["points"] == [(-(1 << 62), 1.0, H), (1 << 62, 2.0, H)]
    rt.close()


def test_read_returns_what_was_set():
    rt = Runtime(48000.0, 64, device=-1)
    assert rt.automation_read(0) == {"points": [], "channels": [], "inputs": 0}
    a = [(5, 1.0, L), (5, 2.0, H), (1 << 40, -3.5, L), ((1 << 40) + 9, 1e-40, H)]
    b = au.ramp(10, 0.0, 20, 1.0) + au.steps([30, 40], [0.5, 0.25])
    rt.automation(7, a)
    rt.automation(2, b)
    f32 = lambda pts: [(f, float(np.float32(v)), c) for f, v, c in pts]
    assert rt.automation_read(7) == {"points": f32(a), "channels": [2, 7], "inputs": 8}
    assert rt.automation_read(2)["points"] == f32(b)
    rt.automation(7, a[:2])                      # replaced
    assert rt.automation_read(7)["points"] == f32(a[:2]) and rt.automation_read(2)["points"] == f32(b)
    rt.automation(7, [])                         # cleared
    assert rt.automation_read(7) == {"points": [], "channels": [2], "inputs": 3}
    # too small a buffer: code 6
    from elementary_amd.runtime import _AutomationInfo, _AutomationPoint
    import ctypes as C
    small, info = (_AutomationPoint * 1)(), _AutomationInfo()
    assert rt._lib.elemhip_automation_read(rt._h, 2, C.byref(info), small, 1) == 6 and info.count == len(b)
    rt.automation_reset()
    assert rt.automation_read(2) == {"points": [], "channels": [], "inputs": 0}
    rt.close()


def test_helpers():
    assert au.ramp(0, 0.0, 10, 1.0) == [(0, 0.0, L), (10, 1.0, H)]
    assert au.steps([0, 5], [1.0, 2.0]) == [(0, 1.0, H), (5, 2.0, H)]
    assert au.to_frames([(0.5, 1.0, "linear"), (1.0000104, 0.0)], 48000.0) == [(24000, 1.0, "linear"), (48000, 0.0)]
    assert au.normalise([(1, 2), (3, 4, "linear")]) == [(1, 2.0, H), (3, 4.0, L)]
    with pytest.raises(ValueError):
        au.normalise([(1, 2, "cubic")])
