"""The input-rate converter without a GPU: the input side of elementary_amd/csrc/resample.h — the pull schedule ``inputs_before``, the
scalar pull loop ``resample_in_host`` and the tile functions the kernels of resample_in.hip take — compiled for the host with
pcm_unpack.h and driven by tests/native/resample_in_host.cpp: the plans of the five ratios and the rates that have none; the schedule
by brute force; the scalar loop against the numpy restatement of the formulas (tests/resample_reference.py) within that reference's
own bound B, and against itself cut into calls; the kernels' schedule emulated workgroup by workgroup and lane by lane over s16, s24
and f32 streams of 1, 3, 8 and 40 channels, block sizes 128, 512, 350 and 16, a cut last block and sets shorter than the filter; the
same program once more under the address and undefined-behaviour sanitizers; the option on a dry handle; ``OfflineRenderer`` on an
engine without the option; and ``_file_span`` with only the older options, pinned."""
import json
import os
import subprocess

import numpy as np
import pytest

import resample_reference as ref
from test_resample_host import CSRC, ROOT, _cxx          # (the compiler the delivery side's host test picks)

RATIOS = [(44100, 176400), (44100, 48000), (48000, 44100), (8000, 12000), (12000, 8000)]          # (input rate, engine rate)
PLANS = {(44100, 176400): (4, 1, 64, 128), (44100, 48000): (160, 147, 64, 35), (48000, 44100): (147, 160, 70, 33),
         (8000, 12000): (3, 2, 64, 48), (12000, 8000): (2, 3, 96, 32)}
CHECKS = ("differing", "lds_out", "lds_unstaged", "span_over", "written_twice", "unwritten", "out_of_half", "tail_not_zero", "src_out",
          "hist_front", "over_cap")


def need(n, L, M):
    return 0 if n == 0 else (n - 1) * M // L + 1


def build_host_program(workdir, name="resample_in_host", extra=()):
    cxx = _cxx()
    assert cxx, "a C++17 compiler builds the host emulation"
    exe = os.path.join(str(workdir), name)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "resample_in_host.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, workdir):
    res = subprocess.run([exe, str(workdir)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-3000:])
    return json.loads(res.stdout.strip().splitlines()[-1]), res.stderr


class Emulation:
    def __init__(self, workdir):
        self.dir = str(workdir)
        self.out = _run(build_host_program(workdir), workdir)[0]

    def floats(self, kind, fin, fout):
        return np.fromfile(os.path.join(self.dir, f"{kind}_{fin}_{fout}.f32"), dtype=np.float32)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return Emulation(tmp_path_factory.mktemp("resample_in"))


def test_plans(emu):
    got = {(p["fin"], p["fout"]): (p["L"], p["M"], p["T"], p["Do"]) for p in emu.out["plans"]}
    assert got == PLANS
    for p in emu.out["plans"]:
        pl = ref.plan(p["fin"], p["fout"])
        assert (p["L"], p["M"], p["T"], p["Do"], p["Wc"]) == (pl["L"], pl["M"], pl["T"], pl["Do"], pl["Wc"])
        assert p["H"] == p["T"] + -(-p["M"] // p["L"]) + 1


def test_rates_without_a_plan_are_refused(emu):
    refused = {(r["fin"], r["fout"]): r for r in emu.out["refused"]}
    assert all(r["refused"] for r in refused.values()), refused
    assert set(refused) >= {(44101, 44100), (0.5, 44100), (72000, 8000), (136000, 8000)}      # not integral (twice), M > 8 L, T > 1024
    assert refused[(72000, 8000)]["output_side"]          # 9:1 is the input side's limit alone: the output side has that plan


def test_need_is_the_smallest_count_that_yields_the_output(emu):
    assert [p["need_wrong"] for p in emu.out["plans"]] == [0] * 5
    for (fin, fout), (L, M, _, _) in PLANS.items():      # ... and the restatement the other tests use agrees with the brute force
        t = 0
        for n in range(0, 600):
            while -((-t * L) // M) < n:
                t += 1
            assert need(n, L, M) == t


@pytest.mark.parametrize("fin,fout", RATIOS)
def test_scalar_loop_is_within_the_bound_of_the_reference(emu, fin, fout):
    L, M, _, _ = PLANS[(fin, fout)]
    x, y = emu.floats("in_x", fin, fout), emu.floats("in_y", fin, fout)
    assert y.shape == (3000,) and x.shape == (need(3000, L, M),)
    want, bound = ref.resample(x, fin, fout)
    assert want[0].shape[0] >= 3000
    err = np.abs(y.astype(np.float64) - want[0][:3000])
    print(fin, fout, "worst error / bound", float((err / bound[0][:3000]).max()))
    assert (err <= bound[0][:3000]).all()
    assert float(np.abs(want[0][:3000]).max()) > 0.5          # (not silence)


def test_one_call_equals_calls_of_1_37_511_and_1453_engine_frames(emu):
    assert len(emu.out["scalar"]) == 5
    for s in emu.out["scalar"]:
        L, M, _, _ = PLANS[(s["fin"], s["fout"])]
        assert s["frames"] == 3000 and s["consumed"] == need(3000, L, M)
        assert [c["call_frames"] for c in s["cuts"]] == [1, 37, 511, 1453]
        for c in s["cuts"]:
            assert c["same_bits"] and c["counts_wrong"] == 0, (s["fin"], s["fout"], c)


def test_lane_schedule_equals_the_scalar_loop(emu):
    """Every engine frame of every set written exactly once, every byte read inside its stream's stride, every LDS slot and image byte
    in range and staged, no tap in front of the carried frames, zeros behind the last valid frame, and the programme the scalar loop's
    bit for bit."""
    seen = set()
    for e in emu.out["lanes"]:
        seen.add((e["L"], e["M"], e["fmt"], e["G"], e["bs"], e["group"]))
        assert e["consumed"] == need(e["frames"], e["L"], e["M"]) and e["frames"] > 0, e
        for key in CHECKS:
            assert e[key] == 0, (key, e)
    combos = {(fmt, G) for _, _, fmt, G, _, _ in seen}
    assert combos >= {(fmt, G) for fmt in (1, 2, 3) for G in (1, 3, 8, 40)}
    for L, M, _, _ in PLANS.values():
        sizes = {(G, bs, group) for l, m, _, G, bs, group in seen if (l, m) == (L, M)}
        assert sizes >= {(1, 350, 1), (3, 128, 4), (8, 512, 4), (40, 128, 4), (1, 16, 1)}, (L, M, sizes)
    # sets shorter than T: 16 engine frames against 64 taps and more
    assert all(e["short_sets"] == 41 for e in emu.out["lanes"] if e["bs"] == 16)
    # a plan too large for four rows: the one-channel kernel reads a three-channel stream sample by sample
    assert (1, 8, 2, 3, 128, 1) in seen


def test_emulation_is_clean_under_asan_and_ubsan(tmp_path):
    exe = build_host_program(tmp_path, "resample_in_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out, err = _run(exe, tmp_path)
    assert len(out["lanes"]) >= 26 and "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]
    assert all(e[key] == 0 for e in out["lanes"] for key in CHECKS)


def test_dry_handle_plans_and_counts():
    """The option, the plan's read-out and the frame count need no device."""
    from elementary_amd.runtime import ElemHipError, Runtime
    for (fin, fout), (L, M, T, Do) in PLANS.items():
        dry = Runtime(float(fout), 512, device=-1)
        with pytest.raises(ElemHipError):
            dry.input_resample_read()                            # off: nothing to read
        with pytest.raises(ElemHipError):
            dry.input_resample_reset()
        assert dry.input_resample_frames(77) == 77
        dry.set_option("input_rate", fin)
        got = dry.input_resample_read()
        assert (got["up"], got["down"], got["taps"], got["latency_frames"], got["frames_in"], got["frames_out"]) == (L, M, T, Do, 0, 0)
        for n in (0, 1, 2, 77, 1000, 12345):
            assert dry.input_resample_frames(n) == need(n, L, M)
        assert dry.resample_frames(1000) == 1000                 # the delivery side is another option
        dry.input_resample_reset()
        dry.set_option("input_rate", 0)
        with pytest.raises(ElemHipError):
            dry.input_resample_read()
    dry = Runtime(44100.0, 512, device=-1)
    dry.set_option("input_rate", 48000)
    for bad in (44101, 0.5):                                     # a refused rate changes nothing
        with pytest.raises(ElemHipError):
            dry.set_option("input_rate", bad)
        assert dry._lib.elemhip_set_option(dry._h, b"input_rate", float(bad)) == 6
        assert dry.input_resample_read()["down"] == 160
    dry = Runtime(8000.0, 512, device=-1)
    for bad in (72000, 136000):                                  # M > 8 L; more than 1024 taps
        with pytest.raises(ElemHipError):
            dry.set_option("input_rate", bad)
    dry.set_option("input_rate", 8000)                           # the engine's own rate: off
    assert dry.input_resample_frames(77) == 77
    # both options on together: each counts its own side
    dry = Runtime(176400.0, 512, device=-1)
    dry.set_option("input_rate", 44100)
    dry.set_option("resample_rate", 44100)
    assert dry.input_resample_frames(1000) == need(1000, 4, 1) == 250 and dry.resample_frames(1000) == 250
    assert dry.input_resample_read()["up"] == 4 and dry.resample_read()["down"] == 4
    dry.set_option("resample_rate", 0)
    assert dry.input_resample_read()["up"] == 4 and dry.resample_frames(1000) == 1000


def test_input_sample_rate_on_an_engine_without_the_option_raises():
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
            core.initialize(num_input_channels=1, num_output_channels=2, sample_rate=176400, input_sample_rate=44100)
        core = OfflineRenderer(engine)
        core.initialize(num_input_channels=1, num_output_channels=2, sample_rate=48000)          # without it: as before
        assert core.input_sample_rate == 48000.0
        core.initialize(num_input_channels=1, num_output_channels=2, sample_rate=48000, input_sample_rate=48000)      # the engine's own: off
        with pytest.raises(RuntimeError):
            core.input_resample()


def _dry_renderer(**kw):
    from elementary_amd.offline import OfflineRenderer
    from elementary_amd.runtime import Runtime
    core = OfflineRenderer(lambda sr, bs: Runtime(sr, bs, device=-1))
    core.initialize(num_input_channels=0, num_output_channels=2, block_size=512, **kw)
    return core


def test_file_span_without_the_option_is_what_it_was():
    """Tuples taken from the code as it stood before the input side existed."""
    assert _dry_renderer(sample_rate=48000)._file_span(1000) == (1000, 0, 1000)
    core = _dry_renderer(sample_rate=48000, output_sample_rate=44100)
    assert core._file_span(1000) == (1036, 33, 919) and core._file_span(0) == (36, 33, 0)
    assert _dry_renderer(sample_rate=176400, output_sample_rate=44100)._file_span(4097) == (4225, 32, 1025)
    assert _dry_renderer(sample_rate=44100, output_sample_rate=48000)._file_span(777) == (810, 35, 846)


def test_file_span_with_the_input_side():
    """A file of F frames renders ceil(F L / M) engine frames; the input latency is taken out in delivered frames, rounded to nearest."""
    core = _dry_renderer(sample_rate=176400, input_sample_rate=44100, output_sample_rate=44100)
    # Di = 128 engine frames = 32 delivered, Do = 32: 64 dropped, 4 * 64 more engine frames rendered
    assert core._file_span(1000, input_frames=True) == (4000 + 256, 64, 1000)
    core = _dry_renderer(sample_rate=44100, input_sample_rate=48000)
    # L / M = 147 / 160, Di = 33 engine frames, delivered at the engine's rate
    assert core._file_span(1000, input_frames=True) == (919 + 33, 33, 919)
    core = _dry_renderer(sample_rate=48000, input_sample_rate=44100, output_sample_rate=44100)
    # Di = 35 engine frames = 32.16 delivered -> 32 (under half a frame off), Do = 33: 65 dropped, ceil(65 * 160 / 147) = 71 more
    assert core._file_span(441, input_frames=True) == (480 + 71, 65, 441)
