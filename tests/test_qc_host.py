"""The inspector without a GPU: the scalar twin (elemhip_qc_host) against tests/qc_reference.py, the cut into calls, the associativity
of the run summaries and the kernels' phases emulated lane by lane (tests/native/qc_host.cpp), the thresholds at equality, and
validation on a dry engine handle."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import qc_reference as ref
from elementary_amd.runtime import ElemHipError, Runtime, _QcChannel, qc_host
from test_fft_host import ROOT, _clangxx

PAIRS = [(0, 2), (1, 0)]


def programme(n, channels, seed=1):
    """float32 [channels, n]: noise with planted silence (head, inner runs of 64 and 63, a long one), clipped runs (2, 3, at frame 0,
    to the last frame), a NaN and an inf, where the length allows; channel 2 is channel 0 in anti-phase from frame 200 on."""
    rng = np.random.default_rng(seed * 104729 + n)
    x = (0.3 * rng.standard_normal((channels, n))).astype(np.float32)
    x[np.abs(x) < 1e-3] = np.float32(0.01)            # (no accidental digital silence)
    x = np.clip(x, -0.95, 0.95).astype(np.float32)
    if n >= 65:
        x[:, :5] = 0.0
    if n > 4096:
        for c in range(channels):
            o = 97 * c
            x[c, :133] = 0.0
            x[c, 300 + o:364 + o] = 0.0                # exactly dropout_frames
            x[c, 500 + o:563 + o] = 0.0                # one fewer
            x[c, 4000 + o:4000 + o + 2 * 4096 + 100] = 0.0
            x[c, 700 + o:702 + o] = 1.0                # clip_run - 1
            x[c, 800 + o:803 + o] = -1.25              # clip_run
            x[c, 900 + o] = np.nan
            x[c, 950 + o] = np.inf
        x[0, :4] = 1.0                                 # a clipped run at frame 0 (the head silence of channel 0 goes)
        if channels > 1:
            x[1, n - 7:] = -1.0                        # ... and one that reaches the last frame
        if channels > 2:
            x[2, 200:] = -x[0, 200:]
    return x


def one_call(x, **kw):
    return qc_host(x, **kw)[0]


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 3 * 4096 + 37])
def test_twin_equals_the_reference(n, channels):
    """Programmes of 0, 1, 63, 64, 65 and 3 * 4096 + 37 frames, 1 and 3 channels (pairs (0, 2) and (1, 0) with 3); buckets off, 96 and
    1000; what was planted is found."""
    x = programme(n, channels)
    pairs = PAIRS if channels == 3 else []
    for bucket in (0, 96, 1000):
        got = one_call(x, pairs=pairs, bucket=bucket)
        want = ref.inspect(x, pairs=pairs, bucket=bucket)
        ref.compare(got, want, (n, channels, bucket), overview=got["overview"])
    if n > 4096:
        # (channel 0's head silence lies behind its clipped run at frame 0: a dropout at frame 4; channel 2 mirrors channel 0 from 200 on)
        assert got["dropouts"]["count"].tolist() == [3, 2, 2][:channels] and (got["dropouts"]["longest"] >= 2 * 4096).all()       # (whole sets of silence)
        assert got["dropouts"]["first_at"].tolist() == [4, 397, 300][:channels]
        assert (got["nonfinite"] == 2).all() and got["head_silence"].tolist() == [0] + [133] * (channels - 1)
        assert got["clip_events"]["count"].tolist() == ([2] + [2] + [1] * (channels - 2))[:channels]
        assert got["clip_events"]["first_at"][0] == 0 and got["clip_events"]["longest"][0] == 4
        if channels == 3:
            assert got["clip_events"]["longest_at"][1] == n - 7 and got["clip_events"]["longest"][1] == 7
            assert ref.correlation(got, 0) < -0.95


def test_the_cut_into_calls_changes_no_bit():
    """Two and three calls with the state handed on: the sums bit for bit, everything else identical, the overview too."""
    n = 3 * 4096 + 37
    x = programme(n, 3, seed=2)
    for bucket in (96, 1000, 8192):
        whole = one_call(x, pairs=PAIRS, bucket=bucket)
        for cuts in ([0, 4097, n], [0, 9 * 64 + 5, 9 * 64 + 5 + 41 * 64, n], [0, 1, 64, n], [0, n - 1, n]):
            state, got = None, None
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                got, state = qc_host(x[:, lo:hi], state=state, pairs=PAIRS, bucket=bucket)
                ref.compare(got, ref.inspect(x[:, :hi], pairs=PAIRS, bucket=bucket), (bucket, cuts, hi), overview=got["overview"])
            assert ref.exact_bytes(got) == ref.exact_bytes(whole), (bucket, cuts)
            assert got["overview"].tobytes() == whole["overview"].tobytes()


def test_skip_and_limit_window_the_programme():
    n = 5000
    x = programme(n, 2, seed=3)
    for skip, limit in ((0, 0), (100, 0), (0, 777), (129, 4096), (6000, 0), (10, 1)):
        state, got = None, None
        for lo, hi in ((0, 64), (64, 3000), (3000, n)):
            got, state = qc_host(x[:, lo:hi], state=state, skip=skip, limit=limit, bucket=96)
        ref.compare(got, ref.inspect(x, skip=skip, limit=limit, bucket=96), (skip, limit), overview=got["overview"])


def test_thresholds_at_equality():
    """A run of exactly clip_run frames counts and one of clip_run - 1 does not; the same for dropout_frames; |x| == silence_level is
    quiet and |x| == clip_level is clipped."""
    s, c = np.float32(0.001), np.float32(0.891)
    x = np.full((1, 400), 0.5, dtype=np.float32)
    x[0, 10:15] = c                     # clip_run
    x[0, 30:34] = -c                    # clip_run - 1
    x[0, 50:55] = np.nextafter(c, np.float32(0))        # just below: not clipped
    x[0, 100:120] = s                   # dropout_frames, at the level
    x[0, 150:169] = -s                  # dropout_frames - 1
    x[0, 200:220] = np.nextafter(s, np.float32(1))      # just above: not quiet
    kw = dict(silence_level=float(s), clip_level=float(c), clip_run=5, dropout_frames=20)
    got = one_call(x, **kw)
    ref.compare(got, ref.inspect(x, **kw), "equality")
    assert got["clipped_frames"][0] == 9 and got["quiet_frames"][0] == 39
    assert got["clip_events"]["count"][0] == 1 and got["clip_events"]["first_at"][0] == 10 and got["clip_events"]["longest"][0] == 5
    assert got["dropouts"]["count"][0] == 1 and got["dropouts"]["first_at"][0] == 100 and got["dropouts"]["longest"][0] == 20
    # all quiet: head = tail = frames, no dropout; then a non-quiet frame behind it makes the tail run no dropout either (it touches 0)
    z = np.zeros((1, 300), dtype=np.float32)
    got, st = qc_host(z)
    assert got["head_silence"][0] == got["tail_silence"][0] == 300 and got["dropouts"]["count"][0] == 0
    got, st = qc_host(np.array([[0.5, 0.0, 0.0]], dtype=np.float32), state=st)
    assert got["head_silence"][0] == 300 and got["tail_silence"][0] == 2 and got["dropouts"]["count"][0] == 0
    got, st = qc_host(np.concatenate([np.zeros(62, dtype=np.float32), [0.5]])[None, :].astype(np.float32), state=st)
    assert got["dropouts"]["count"][0] == 1 and got["dropouts"]["first_at"][0] == 301 and got["dropouts"]["longest"][0] == 64
    # all clipped: one event from frame 0 that keeps growing over calls
    got, st = qc_host(np.ones((1, 100), dtype=np.float32))
    got, st = qc_host(np.ones((1, 100), dtype=np.float32), state=st)
    assert got["clip_events"]["count"][0] == 1 and got["clip_events"]["longest"][0] == 200 and got["clip_events"]["longest_at"][0] == 0


def _build(d, sanitize=False):
    cxx = _clangxx()
    assert cxx, "the ROCm toolchain's clang++ builds the host emulation"
    exe = os.path.join(d, "qc_host")
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off"] + (["-fsanitize=address,undefined", "-g"] if sanitize else []) +
                   ["-I", os.path.join(ROOT, "elementary_amd", "csrc"), os.path.join(ROOT, "tests", "native", "qc_host.cpp"), "-o", exe], check=True)
    return exe


def test_native_associativity_and_emulation():
    """tests/native/qc_host.cpp, built as test_spectrum_host.py builds its program. `assoc`: random flag strings with empty, all-set and
    all-clear stretches, two- and three-way splits in both association orders. `emulate`: the kernels' phases lane by lane, set by
    set, against the twin in the program (the carried states byte for byte) and against elemhip_qc_host here."""
    with tempfile.TemporaryDirectory() as d:
        exe = _build(d)
        out = subprocess.run([exe, "assoc", "7", "20000"], check=True, capture_output=True, text=True).stdout
        assert "20000 strings, all equal" in out
        n = 3 * 4096 + 37
        x = programme(n, 3, seed=5)
        fx, fo = os.path.join(d, "x.f32"), os.path.join(d, "out.bin")
        x.astype("<f4").tofile(fx)
        for bs, blocks, bucket in ((64, 8, 96), (64, 8, 1000), (512, 8, 96), (350, 3, 16), (64, 8, 65536), (64, 1024, 1000)):
            run = subprocess.run([exe, "emulate", "3", str(n), str(bs), str(blocks), "0", "1.0", "3", "64", str(bucket), "0:2,1:0", fx, fo],
                                 capture_output=True, text=True)
            assert run.returncode == 0, (bs, blocks, bucket, run.stdout, run.stderr)
            twin = one_call(x, pairs=PAIRS, bucket=bucket)
            raw = open(fo, "rb").read()
            size = C.sizeof(_QcChannel)
            recs = [_QcChannel.from_buffer_copy(raw[c * size:(c + 1) * size]) for c in range(3)]
            assert [r.sum for r in recs] == twin["sum"].tolist() and [r.sum_sq for r in recs] == twin["sum_sq"].tolist()
            assert [r.dropouts.count for r in recs] == twin["dropouts"]["count"].tolist() and [r.tail_silence for r in recs] == twin["tail_silence"].tolist()
            rest = raw[3 * size:]
            assert np.frombuffer(rest[:16], dtype="<f8").tolist() == twin["sum_xy"].tolist()
            assert rest[16:] == twin["overview"].tobytes(), (bs, blocks, bucket)


def test_validation_on_a_dry_handle():
    """Each parameter out of range is refused with code 6 on a handle without a device — by the twin too — and leaves the previous
    spec in force; a good spec is accepted there, and so is turning the inspector off."""
    rt = Runtime(48000.0, 512, device=-1)
    rt.qc(clip_run=7)
    bad = [dict(silence_level=-0.1), dict(silence_level=float("nan")), dict(clip_level=0.0), dict(clip_level=-1.0), dict(clip_run=0), dict(clip_run=65536),
           dict(dropout_frames=0), dict(dropout_frames=2 ** 31), dict(bucket=15), dict(bucket=1048577), dict(pairs=[(1, 1)]),
           dict(pairs=[(0, 1)] * 129)]
    for kw in bad:
        with pytest.raises(ElemHipError) as e:
            rt.qc(**kw)
        assert e.value.code == 6, kw
        with pytest.raises(ElemHipError) as e:
            qc_host(np.zeros((2, 8), dtype=np.float32), **kw)
        assert e.value.code == 6, kw
    with pytest.raises(ElemHipError) as e:
        qc_host(np.zeros((2, 8), dtype=np.float32), pairs=[(0, 2)])      # a pair past the channels of the call
    assert e.value.code == 6
    rt.qc(bucket=16, pairs=[(0, 1)] * 128, clip_run=65535, dropout_frames=2 ** 31 - 1, silence_level=0.0, clip_level=1e-30)
    rt.qc({"bucket": 1048576})
    rt.qc(None)
    with pytest.raises(ValueError):
        rt.qc(bucket_size=3)


def test_report_and_findings():
    """elementary_amd.qc: DC, RMS, correlation (nan where a side is silent) and silence in seconds; findings against limits."""
    from elementary_amd import qc as qcmod
    n, sr = 48000, 48000.0
    t = np.arange(n)
    x = np.zeros((4, n), dtype=np.float32)
    x[0] = (0.5 * np.sin(2 * np.pi * 440.0 * t / sr) + 0.25).astype(np.float32)
    x[1] = -x[0]
    x[2, 4800:] = 0.1
    x[2, 20000:20100] = 0.0
    x[2, n - 2400:] = 0.0
    got = qc_host(x, pairs=[(0, 1), (0, 3)], clip_level=0.74, clip_run=2)[0]
    rep = qcmod.report(got, sr)
    assert abs(rep["dc"][0] - 0.25) < 1e-6 and abs(rep["dc"][1] + 0.25) < 1e-6 and rep["dc"][3] == 0.0
    assert abs(rep["rms_dbfs"][0] - 10 * np.log10(0.125 + 0.0625)) < 1e-3 and rep["rms_dbfs"][3] == -np.inf
    assert abs(rep["correlation"][0] + 1.0) < 1e-12 and np.isnan(rep["correlation"][1])
    assert rep["head_silence_s"][2] == 0.1 and rep["tail_silence_s"][2] == 0.05
    found = qcmod.findings(got, sr, max_head_s=0.05, max_tail_s=0.01, max_dc=0.1, min_correlation=-0.5)
    kinds = sorted((f["kind"], f["channel"]) for f in found)
    assert ("head_silence", 2) in kinds and ("tail_silence", 2) in kinds and ("dropout", 2) in kinds and ("dc", 0) in kinds and ("dc", 1) in kinds
    assert ("correlation", 0) in kinds and ("clip", 0) in kinds and ("head_silence", 3) in kinds
    drop = [f for f in found if f["kind"] == "dropout"][0]
    assert (drop["at"], drop["length"], drop["value"]) == (20000, 100, 1.0)
    assert qcmod.findings(qc_host(np.zeros((1, 0), dtype=np.float32))[0], sr, 0.0, 0.0, 0.0, 1.0) == []
