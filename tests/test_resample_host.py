"""The delivery-rate converter without a GPU: elementary_amd/csrc/resample.h — the header the converter's kernels (resample.hip) take
their plan, their tables, their tap sum and their tile schedule from — compiled for the host and driven by
tests/native/resample_host.cpp: the plans of the five ratios and the rates that have none; the filter measured from the table the
header built; the header's scalar loop against the numpy restatement of the formulas (tests/resample_reference.py, which was not
derived from the header) within the reference's bound B, and against itself cut into calls; the kernel's schedule emulated
workgroup by workgroup and lane by lane over block sizes 128, 512 and 350 (and 16, through the one-channel kernel), a cut last block
and sets shorter than the filter; the same program once more under the address and undefined-behaviour sanitizers; the option on a
dry handle; and ``OfflineRenderer`` on an engine without the option."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import resample_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elementary_amd", "csrc")
RATIOS = [(48000, 44100), (44100, 48000), (176400, 44100), (8000, 12000), (12000, 8000)]
PLANS = {(48000, 44100): (147, 160, 70, 33), (44100, 48000): (160, 147, 64, 35), (176400, 44100): (1, 4, 256, 32),
         (8000, 12000): (3, 2, 64, 48), (12000, 8000): (2, 3, 96, 32)}


def _cxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++")):
        if c and os.path.exists(c):
            return c
    return None


def _build_and_run(workdir, name, extra):
    cxx = _cxx()
    assert cxx, "a C++17 compiler builds the host emulation"
    exe = os.path.join(str(workdir), name)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "resample_host.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe, str(workdir)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-3000:])
    return json.loads(res.stdout.strip().splitlines()[-1]), res.stderr


class Emulation:
    def __init__(self, workdir):
        self.dir = str(workdir)
        self.out = _build_and_run(workdir, "resample_host", [])[0]

    def floats(self, kind, fin, fout):
        return np.fromfile(os.path.join(self.dir, f"{kind}_{fin}_{fout}.f32"), dtype=np.float32)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return Emulation(tmp_path_factory.mktemp("resample"))


def test_plans(emu):
    got = {(p["fin"], p["fout"]): (p["L"], p["M"], p["T"], p["Do"]) for p in emu.out["plans"]}
    assert got == PLANS
    for p in emu.out["plans"]:
        pl = ref.plan(p["fin"], p["fout"])
        assert (p["L"], p["M"], p["T"], p["Do"], p["Wc"]) == (pl["L"], pl["M"], pl["T"], pl["Do"], pl["Wc"])
        assert p["H"] == p["T"] + -(-p["M"] // p["L"]) + 1


def test_rates_without_a_plan_are_refused(emu):
    refused = {(r["fin"], r["fout"]): r["refused"] for r in emu.out["refused"]}
    assert refused[(44100, 44101)] and refused[(8000, 192000)]
    assert all(refused.values()), refused          # (also: a rate that is not integral, a rate of 0, more than 1024 taps)


@pytest.mark.parametrize("fin,fout", RATIOS)
def test_filter_measured_from_the_header_s_table(emu, fin, fout):
    """Within +-0.001 dB up to 0.9 of the lower Nyquist, at or below -96 dB from 1.1 of it to fin L / 2 (the design gives +-0.0001 dB
    and -98.4 dB in float64; the margins cover float32 coefficients)."""
    pl = ref.plan(fin, fout)
    proto = emu.floats("proto", fin, fout)
    assert proto.shape == (pl["T"] * pl["L"],)
    # ... and it is the reference's prototype, rounded once
    m = np.arange(len(proto), dtype=np.float64)
    want = ref.prototype((m - pl["Wc"] * pl["L"]) / pl["L"], pl)
    assert np.abs(proto - want).max() <= 3 * 2.0 ** -24 * np.abs(want).max()
    f, db = ref.response_db(proto, pl["L"], fin)
    nyq = min(fin, fout) / 2.0
    ripple, stop = float(np.abs(db[f <= 0.9 * nyq]).max()), float(db[f >= 1.1 * nyq].max())
    print(fin, fout, "ripple dB", ripple, "stop band dB", stop)
    assert ripple <= 0.001 and stop <= -96.0


@pytest.mark.parametrize("fin,fout", RATIOS)
def test_scalar_loop_is_within_the_bound_of_the_reference(emu, fin, fout):
    x, y = emu.floats("x", fin, fout), emu.floats("y", fin, fout)
    assert x.shape == (3000,)
    want, bound = ref.resample(x, fin, fout)
    assert y.shape == want[0].shape == (ref.frames_out(3000, ref.plan(fin, fout)),)
    err = np.abs(y.astype(np.float64) - want[0])
    print(fin, fout, "worst error / bound", float((err / bound[0]).max()))
    assert (err <= bound[0]).all()
    assert float(np.abs(want[0]).max()) > 0.5          # (not silence)


def test_one_call_equals_calls_of_1_37_511_and_1453_frames(emu):
    assert len(emu.out["scalar"]) == 5
    for s in emu.out["scalar"]:
        assert s["outputs"] == ref.frames_out(s["frames"], ref.plan(s["fin"], s["fout"]))
        assert [c["call_frames"] for c in s["cuts"]] == [1, 37, 511, 1453]
        for c in s["cuts"]:
            assert c["same_bits"] and c["counts_wrong"] == 0, (s["fin"], s["fout"], c)


def test_lane_schedule_equals_the_scalar_loop(emu):
    """Every output of every set produced exactly once, every LDS slot in range and staged, the converted half's tail zero, and the
    programme the scalar loop's bit for bit."""
    seen = set()
    for e in emu.out["lanes"]:
        seen.add((e["L"], e["M"], e["bs"], e["group"]))
        assert e["outputs"] == -((-e["frames"] * e["L"]) // e["M"]) and e["outputs"] > 0, e
        for key in ("differing", "lds_out", "lds_unstaged", "span_over", "written_twice", "unwritten", "out_of_half", "tail_not_zero", "over_cap"):
            assert e[key] == 0, (key, e)
    for L, M, _, _ in PLANS.values():
        for bs in (128, 512, 350):
            assert (L, M, bs, 4) in seen
        assert (L, M, 16, 1) in seen
    # a set shorter than T: 128 frames against 256 taps
    assert any(e["set_blocks"] == 1 and e["bs"] == 128 and (e["L"], e["M"]) == (1, 4) for e in emu.out["lanes"])


def test_emulation_is_clean_under_asan_and_ubsan(tmp_path):
    out, err = _build_and_run(tmp_path, "resample_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert len(out["lanes"]) >= 25 and "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]


def test_dry_handle_plans_and_counts():
    """The option, the plan's read-out and the frame count need no device."""
    from elementary_amd.runtime import ElemHipError, Runtime
    for (fin, fout), (L, M, T, Do) in PLANS.items():
        dry = Runtime(float(fin), 512, device=-1)
        with pytest.raises(ElemHipError):
            dry.resample_read()                                  # off: nothing to read
        assert dry.resample_frames(1000) == 1000
        dry.set_option("resample_rate", fout)
        got = dry.resample_read()
        assert (got["up"], got["down"], got["taps"], got["latency_frames"], got["frames_in"], got["frames_out"]) == (L, M, T, Do, 0, 0)
        assert dry.resample_frames(1000) == -((-1000 * L) // M)
        dry.resample_reset()
        dry.set_option("resample_rate", 0)
        with pytest.raises(ElemHipError):
            dry.resample_read()
    dry = Runtime(44100.0, 512, device=-1)
    for bad in (44101, 0.5):
        with pytest.raises(ElemHipError):
            dry.set_option("resample_rate", bad)
    dry = Runtime(8000.0, 512, device=-1)
    with pytest.raises(ElemHipError):
        dry.set_option("resample_rate", 192000)
    dry.set_option("resample_rate", 8000)                        # the engine's own rate: off
    assert dry.resample_frames(77) == 77


def test_output_sample_rate_on_an_engine_without_the_option_raises():
    from elementary_amd.offline import OfflineRenderer

    class Plain:                                                 # the CRuntime surface of the CPU checkers: no options at all
        def __init__(self, sr, bs):
            pass

    class Deaf(Plain):                                           # options, but not this one
        def set_option(self, key, value):
            raise RuntimeError(f"unknown option {key!r}")

    for engine in (Plain, Deaf):
        core = OfflineRenderer(engine)
        with pytest.raises(RuntimeError):
            core.initialize(num_output_channels=2, sample_rate=48000, output_sample_rate=44100)
        OfflineRenderer(engine).initialize(num_output_channels=2, sample_rate=48000)            # without it: as before
