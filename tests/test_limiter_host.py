"""The true-peak limiter without a GPU: elementary_amd/csrc/limiter.h — the header the limiter's kernels (limiter.hip) take their plan,
their per-frame arithmetic, their carried state and every lane's share of a tile from — compiled for the host and driven by
tests/native/limiter_host.cpp: the look-ahead's limits and the parameters that are refused; the header's scalar loop against the numpy
restatement of the formulas (tests/limiter_reference.py, which was not derived from the header) within one float32 ulp, and against
itself cut into calls; the kernels' schedule emulated workgroup by workgroup and lane by lane over block sizes 16, 128, 350 and 512,
look-aheads of 1, 18, 66 and 300 frames and links of 0, 1, 2 and 3 channels, a cut last block and sets shorter than the latency; the
same program once more under the address and undefined-behaviour sanitizers; the options on a dry handle; ``OfflineRenderer`` on an
engine without the option; and the frames ``write_wav`` takes out for the converter and the limiter together."""
import json
import os
import subprocess

import numpy as np
import pytest

import limiter_reference as ref
from test_resample_host import CSRC, ROOT, _cxx

RATE = 12000.0


def _build(workdir, name, extra):
    cxx = _cxx()
    assert cxx, "a C++17 compiler builds the host emulation"
    exe = os.path.join(str(workdir), name)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "limiter_host.cpp"), "-o", exe], check=True)
    return exe


def _build_and_run(workdir, name, extra):
    exe = _build(workdir, name, extra)
    res = subprocess.run([exe, str(workdir)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-3000:])
    return json.loads(res.stdout.strip().splitlines()[-1]), res.stderr


def host_loop(workdir, floats, rate, call=None, **params):
    """limiter_host() of the header over `floats` [channels, frames], one programme from frame 0 cut into calls of `call` frames:
    (the limited floats, the statistics)."""
    exe = os.path.join(str(workdir), "limiter_host")
    if not os.path.exists(exe):
        _build(workdir, "limiter_host", [])
    floats = np.ascontiguousarray(floats, dtype=np.float32)
    floats.tofile(os.path.join(str(workdir), "apply_in.f32"))
    p = {"ceiling_dbtp": -1.0, "gain_db": 0.0, "lookahead_ms": 1.5, "release_ms": 500.0, "link": 0, **params}
    subprocess.run([exe, str(workdir), "apply", repr(float(rate)), repr(float(p["ceiling_dbtp"])), repr(float(p["gain_db"])), repr(float(p["lookahead_ms"])),
                    repr(float(p["release_ms"])), str(int(p["link"])), str(floats.shape[0]), str(int(call or max(1, floats.shape[1])))],
                   check=True, capture_output=True, timeout=300)
    out = np.fromfile(os.path.join(str(workdir), "apply_out.f32"), dtype=np.float32).reshape(floats.shape)
    with open(os.path.join(str(workdir), "apply_stats.json")) as f:
        return out, json.load(f)


class Emulation:
    def __init__(self, workdir):
        self.dir = str(workdir)
        self.out = _build_and_run(workdir, "limiter_host_emu", [])[0]

    def floats(self, name):
        return np.fromfile(os.path.join(self.dir, name), dtype=np.float32)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return Emulation(tmp_path_factory.mktemp("limiter"))


def test_lookahead_limits_and_refusals(emu):
    """D = round(ms rate / 1000) must lie in 1 .. 1024; a plan that is refused leaves the caller's untouched."""
    plans = emu.out["plans"]
    ok = [(p["rate"], p["D"], p["R"], p["latency"], p["hist"]) for p in plans if p["ok"]]
    assert ok == [(48000, 72, 24000, 78, 89), (44100, 66, 22050, 72, 83), (12000, 1, 600, 7, 18), (12000, 1024, 600, 1030, 1041), (48000, 1024, 1, 1030, 1041)]
    assert len([p for p in plans if not p["ok"]]) == 13 and all(p["untouched"] for p in plans)
    for p in plans:
        if p["ok"]:
            assert p["D"] == ref.frames_of(p["lookahead_ms"], p["rate"])
        elif p["rate"] == 12000:
            assert ref.frames_of(p["lookahead_ms"], p["rate"]) in (0, 1025)


def test_scalar_loop_is_within_an_ulp_of_the_reference(emu):
    """Six channels with a NaN and an inf among them, 2 dB of gain, every look-ahead and link: the floats within one float32 ulp, the
    statistics as limiter_reference.check_stats asks."""
    x = emu.floats("x.f32").reshape(6, 3000)
    assert len(emu.out["scalar"]) == 16
    for s in emu.out["scalar"]:
        params = dict(ceiling_dbtp=-1.0, gain_db=2.0, lookahead_ms=s["D"] * 1000.0 / RATE, release_ms=50.0, link=s["link"])
        assert ref.plan(RATE, **params)["D"] == s["D"]
        want, g, stats = ref.limit(x, RATE, **params)
        got = emu.floats(f"y_{s['D']}_{s['link']}.f32").reshape(6, 3000)
        ok = ref.within(got, want)
        assert ok.all(), (s["D"], s["link"], int((~ok).sum()), np.argwhere(~ok)[:4].tolist())
        assert np.isnan(got[1, 1200 + s["D"] + 6]) and np.isinf(got[1, 1400 + s["D"] + 6])
        ref.check_stats(s["max_reduction"], s["limited_frames"], stats)
        assert 0.3 < (g < 1.0).mean() < 0.99 and (g == 1.0).mean() > 0.005, (s["D"], s["link"], float((g < 1.0).mean()))
        fin = np.isfinite(got)
        assert float(np.abs(got[fin]).max()) <= np.float32(10.0 ** (-1.0 / 20.0)) + np.spacing(np.float32(10.0 ** (-1.0 / 20.0)))


def test_one_call_equals_calls_of_1_37_511_and_1453_frames(emu):
    for s in emu.out["scalar"]:
        assert [c["call_frames"] for c in s["cuts"]] == [1, 37, 511, 1453]
        assert all(c["same_bits"] for c in s["cuts"]), (s["D"], s["link"], s["cuts"])


def test_lane_schedule_equals_the_scalar_loop(emu):
    """Every frame of every set written exactly once and inside its half, the half's tail zero, and floats, carried state and
    statistics the scalar loop's bit for bit."""
    seen = set()
    for e in emu.out["lanes"]:
        seen.add((e["bs"], e["D"], e["link"], e["set_blocks"]))
        assert e["limited"] > 0, e
        for key in ("differing", "written_twice", "unwritten", "tail_not_zero", "outside", "state_differs", "stats_differ"):
            assert e[key] == 0, (key, e)
    for bs in (16, 128, 350, 512):
        for D in (1, 18, 66, 300):
            for link in (0, 1, 2, 3):
                assert (bs, D, link, 8) in seen
    # sets shorter than the latency: one block of 16 or 128 frames against 306; a halo of 35 frames over more than two blocks of 16
    assert (16, 300, 0, 1) in seen and (128, 300, 2, 1) in seen and (16, 18, 0, 1) in seen
    assert all(e["frames"] % e["bs"] != 0 for e in emu.out["lanes"])          # (a cut last block everywhere)


def test_emulation_is_clean_under_asan_and_ubsan(tmp_path):
    out, err = _build_and_run(tmp_path, "limiter_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert len(out["lanes"]) >= 64 and "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]


def test_host_loop_tool_cut_into_calls(tmp_path):
    """The `apply` mode the GPU tests use: the same bits however it is cut."""
    x = ref.signal(128)
    params = dict(ceiling_dbtp=-1.0, lookahead_ms=18 * 1000.0 / RATE, release_ms=50.0, link=1)
    a, sa = host_loop(tmp_path, x, RATE, **params)
    b, sb = host_loop(tmp_path, x, RATE, call=256, **params)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and sa == sb
    want, _, stats = ref.limit(x, RATE, **params)
    assert ref.within(a, want).all()
    ref.check_stats(sa["max_reduction"], sa["limited_frames"], stats)


def test_options_on_a_dry_handle():
    """The options, their ranges and the plan's read-out need no device; a render does."""
    from elementary_amd.runtime import ElemHipError, Runtime
    dry = Runtime(48000.0, 512, device=-1)
    for call in (dry.limiter_read, dry.limiter_reset):
        with pytest.raises(ElemHipError):
            call()                                               # off: nothing to read
    for key, bad in (("limiter_ceiling_dbtp", 0.5), ("limiter_ceiling_dbtp", -41), ("limiter_gain_db", 61), ("limiter_gain_db", -60.5),
                     ("limiter_lookahead_ms", 0.005), ("limiter_lookahead_ms", 21.4), ("limiter_release_ms", 0.001), ("limiter_link", -1),
                     ("limiter_link", 1.5), ("limiter", 2), ("limiter_colour", 1)):
        with pytest.raises(ElemHipError) as e:
            dry.set_option(key, bad)
        assert getattr(e.value, "code", 6) == 6
    dry.set_option("limiter", 1)
    got = dry.limiter_read()
    assert (got["lookahead_frames"], got["latency_frames"], got["release_frames"], got["link"], got["groups"], got["frames"]) == (72, 78, 24000, 0, 0, 0)
    assert got["max_reduction"].shape == got["limited_frames"].shape == (0,)
    dry.set_option("limiter_lookahead_ms", 21.0)
    dry.set_option("limiter_release_ms", 50)
    dry.set_option("limiter_link", 2)
    got = dry.limiter_read()
    assert (got["lookahead_frames"], got["latency_frames"], got["release_frames"], got["link"]) == (1008, 1014, 2400, 2)
    with pytest.raises(ElemHipError):
        dry.set_option("limiter_lookahead_ms", 22.0)             # D = 1056: refused, the plan stays
    assert dry.limiter_read()["lookahead_frames"] == 1008
    # the plan follows the delivery rate, whichever option is set first; a rate that leaves no plan is refused
    dry.set_option("limiter_lookahead_ms", 1.5)
    dry.set_option("resample_rate", 44100)
    assert dry.limiter_read()["lookahead_frames"] == 66 and dry.limiter_read()["release_frames"] == 2205
    dry.set_option("limiter_lookahead_ms", 22.0)                 # 970 frames at 44100
    with pytest.raises(ElemHipError):
        dry.set_option("resample_rate", 0)                       # back to 48000: D = 1056
    assert dry.resample_read()["up"] == 147 and dry.limiter_read()["lookahead_frames"] == 970
    dry.limiter_reset()
    with pytest.raises(ElemHipError) as e:
        dry.process_blocks_host(None, 2, 1024, np.zeros((2, dry.resample_frames(1024)), dtype=np.float32))
    assert "101" in str(e.value) or getattr(e.value, "code", None) == 101          # kNoDevice
    dry.set_option("limiter", 0)
    with pytest.raises(ElemHipError):
        dry.limiter_read()
    other = Runtime(44100.0, 512, device=-1)
    other.set_option("resample_rate", 48000)
    other.set_option("limiter", 1)
    assert other.limiter_read()["lookahead_frames"] == 72


class _Plain:                                                    # the CRuntime surface of the CPU checkers: no options at all
    def __init__(self, sr, bs):
        pass


class _Deaf(_Plain):                                             # options, but not this one
    def set_option(self, key, value):
        raise RuntimeError(f"unknown option {key!r}")

    def limiter_read(self):
        raise RuntimeError("off")


def test_limiter_on_an_engine_without_the_option_raises():
    from elementary_amd.offline import OfflineRenderer
    for engine in (_Plain, _Deaf):
        for want in (True, {"ceiling_dbtp": -2.0}):
            with pytest.raises(RuntimeError):
                OfflineRenderer(engine).initialize(num_output_channels=2, sample_rate=48000, limiter=want)
        core = OfflineRenderer(engine)
        core.initialize(num_output_channels=2, sample_rate=48000)             # without it: as before
        for call in (core.limiter,):
            with pytest.raises(RuntimeError):
                call()
        core.initialize(num_output_channels=2, sample_rate=48000, limiter=False)
        assert core._file_span(1000) == (1000, 0, 1000)


class _Fake(_Plain):
    """Keeps what the renderer sets and answers with the plans of 48000 -> 44100 and a look-ahead of 66 frames."""
    def __init__(self, sr, bs):
        self.options, self.resets = {}, []

    def set_option(self, key, value):
        self.options[key] = value

    def add_shared_resource(self, *a):
        pass

    def resample_read(self):
        return {"up": 147, "down": 160, "taps": 70, "latency_frames": 33, "frames_in": 0, "frames_out": 0}

    def resample_reset(self):
        self.resets.append("resample")

    def limiter_read(self):
        return {"lookahead_frames": 66, "latency_frames": 72, "release_frames": 22050, "link": 0, "groups": 0, "frames": 0,
                "max_reduction": np.zeros(0), "limited_frames": np.zeros(0, dtype=np.uint64)}

    def limiter_reset(self):
        self.resets.append("limiter")


def test_file_span_takes_both_latencies_out():
    """Skip Do + D + 6 delivered frames, render ceil((Do + D + 6) down / up) further frames, keep ceil(frames up / down); new programmes."""
    from elementary_amd.offline import OfflineRenderer
    core = OfflineRenderer(_Fake)
    core.initialize(num_output_channels=2, sample_rate=48000, output_sample_rate=44100, limiter={"lookahead_ms": 1.5, "link": 2})
    assert core.runtime.options == {"resample_rate": 44100.0, "limiter_lookahead_ms": 1.5, "limiter_link": 2.0, "limiter": 1}
    assert list(core.runtime.options)[-1] == "limiter"                        # (the parameters first: turning it on cannot fail on them later)
    assert core._file_span(10000) == (10000 + -((-(33 + 72) * 160) // 147), 33 + 72, -((-10000 * 147) // 160))
    assert core.runtime.resets == ["resample", "limiter"]
    assert core.limiter()["max_reduction_db"] == 0.0
    only = OfflineRenderer(_Fake)
    only.initialize(num_output_channels=2, sample_rate=48000, limiter=True)
    assert only.runtime.options == {"limiter": 1}
    assert only._file_span(10000) == (10072, 72, 10000) and only.runtime.resets == ["limiter"]
    with pytest.raises(ValueError):
        OfflineRenderer(_Fake).initialize(num_output_channels=2, sample_rate=48000, limiter={"colour": 1})
    plain = OfflineRenderer(_Fake)
    plain.initialize(num_output_channels=2, sample_rate=48000, output_sample_rate=44100)
    assert plain._file_span(10000) == (10000 + -((-33 * 160) // 147), 33, -((-10000 * 147) // 160)) and plain.runtime.resets == ["resample"]
