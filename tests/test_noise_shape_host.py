"""Noise-shaped requantisation on the host (elementary_amd/csrc/noise_shape.h through elemhip_noise_shape_host; no GPU): the scalar
twin against tests/noise_shape_reference.py code for code and state for state, cut invariance, the validation of coefficient sets, the
spectrum of the shaped error against plain TPDF, the presets' figures, and the kernel's tile schedule emulated lane by lane by
tests/native/noise_shape_host.cpp. The oracle of everything but the spectrum is exact."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import noise_shape_reference as ref
import pcm_reference
from elementary_amd import noise_shape as presets
from elementary_amd import runtime as R
from helpers import lcg_noise_fast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elementary_amd", "csrc")
TAPS = {1: presets.PRESETS["first"], 2: presets.PRESETS["second"], 5: presets.PRESETS["lipshitz5"], 9: presets.PRESETS["fweighted9"],
        12: presets.PRESETS["fweighted9"] + [0.31, -0.17, 0.05]}


def _signals(n=700):
    t = np.arange(n)
    noise = np.stack([lcg_noise_fast(n, 5 + c, 0.8) for c in range(2)]).astype(np.float32)
    sine = (1.5 * np.sin(2.0 * np.pi * 997.0 * t / 44100.0)).astype(np.float32)[None, :]
    odd = lcg_noise_fast(n, 9, 0.5).astype(np.float32)
    odd[3::41] = np.nan; odd[7::53] = np.inf; odd[11::59] = -np.inf; odd[13::61] = 3e38; odd[17::67] = -1e-42
    return np.concatenate([noise, sine, odd[None, :]])


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("K", [1, 2, 5, 9, 12])
def test_twin_equals_the_reference(K, bits):
    """Noise at 0.8, a sine at 1.5 x full scale (it clips; at 16 bits the feedback saturates with the larger filters), non-finite and
    huge samples, with and without dither, at a time that straddles 2^32: codes, errors and saturation counts."""
    x = _signals()
    for seed in (None, 77):
        t0 = (1 << 32) - 300
        got, st = R.noise_shape_host(TAPS[K], x, bits, seed, channel0=3, time0=t0)
        want, wst = ref.shape(TAPS[K], x, bits, seed, channel0=3, time0=t0)
        assert np.array_equal(got.astype(np.int64), want), (K, bits, seed)
        assert np.array_equal(st, ref.state_bytes(wst)), (K, bits, seed)
        S = 1 << (bits - 1)
        assert want[2].min() == -S and want[2].max() == S - 1
        print(K, bits, seed, "saturated", wst["saturated"].tolist())


def test_dither_is_pcm_packs_hashes():
    """dq is the top 8 bits of the two hashes whose top 24 make pcm_pack's dither: floor-consistent with it."""
    t = np.arange(4096, dtype=np.int64) + (1 << 32) - 2048
    d24 = pcm_reference.dither(12345, 4, t).astype(np.float64) * 2.0 ** 24
    dq = ref.dither_q8(12345, 4, t)
    assert np.all(np.abs(d24 / 65536.0 - dq) < 1.0) and dq.min() < -200 and dq.max() > 200


def test_cutting_the_input_changes_nothing():
    x = _signals(1200)
    for K, seed in ((9, 5), (12, None), (1, 9)):
        whole, wst = R.noise_shape_host(TAPS[K], x, 16, seed, time0=1000)
        parts, st, at = [], None, 0
        for end in (100, 101, 612, 1200):
            got, st = R.noise_shape_host(TAPS[K], x[:, at:end], 16, seed, time0=1000 + at, state=st)
            parts.append(got)
            at = end
        assert np.array_equal(np.concatenate(parts, axis=1), whole) and np.array_equal(st, wst)


def test_refused_coefficient_sets():
    x = np.zeros((1, 8), np.float32)
    for bad in ([], [0.1] * 13, [1.0, float("nan")], [float("inf")], [64.0], [32.0, -32.0]):
        assert ref.quantise_coeffs(bad) is None
        with pytest.raises(R.ElemHipError) as e:
            R.noise_shape_host(bad, x)
        assert e.value.code == 6
    for good in ([63.99951171875], [32.0, -31.99951171875], [0.0]):          # sum |cq| = 131071, and a filter of nothing
        assert ref.quantise_coeffs(good) is not None
        R.noise_shape_host(good, x)
    assert ref.quantise_coeffs([2.033, -2.165]) == [4164, -4434]


def test_handle_validation_on_a_dry_runtime():
    """elemhip_noise_shape_set through Runtime: off by default, K = 0 means off, refused sets change nothing."""
    rt = R.Runtime(44100.0, 64, device=-1)
    assert rt.noise_shape_read()["taps"] == 0
    rt.noise_shape(presets.PRESETS["lipshitz5"])
    got = rt.noise_shape_read()
    assert got["taps"] == 5 and got["coeffs_q"].tolist() == ref.quantise_coeffs(presets.PRESETS["lipshitz5"]) and got["channels"] == 0 and got["frames"] == 0
    for bad in ([0.1] * 13, [1.0, float("nan")], [64.0]):
        with pytest.raises(R.ElemHipError) as e:
            rt.noise_shape(bad)
        assert e.value.code == 6
        assert rt.noise_shape_read()["coeffs_q"].tolist() == got["coeffs_q"].tolist()
    rt.noise_shape_reset()
    rt.noise_shape([])
    assert rt.noise_shape_read()["taps"] == 0
    rt.noise_shape(None)
    assert rt.noise_shape_read()["taps"] == 0


def _error_spectrum(codes, x):
    err = np.asarray(codes, dtype=np.float64) - 32768.0 * x.astype(np.float64)
    return np.abs(np.fft.rfft(err)) ** 2


@pytest.mark.parametrize("name,total,low", [("first", (1.7, 2.3), 0.26), ("fweighted9", (55.0, 83.0), 0.05)])
def test_error_spectrum(name, total, low):
    """A 997 Hz sine of amplitude 0.001 at 16 bits, 16384 frames, seed 7: the shaped error's power over plain TPDF's (pcm_pack's
    quantiser, from pcm_reference) is 1 + sum c^2 in all (2; 69.2), and in rfft bins 0 .. N / 8 what the NTF leaves there (`first`:
    2 (a - sin a) / a at a = pi / 4 = 0.199). Nothing saturates."""
    N = 16384
    n = np.arange(N)
    x = (0.001 * np.sin(2.0 * np.pi * 997.0 * n / 44100.0)).astype(np.float32)
    codes, st = R.noise_shape_host(presets.PRESETS[name], x, 16, 7, channel0=0, time0=0)
    plain = pcm_reference.quant(x, 16, pcm_reference.dither(7, 0, n.astype(np.int64)))
    ps, pp = _error_spectrum(codes[0], x), _error_spectrum(plain, x)
    ratio, ratio_low = ps.sum() / pp.sum(), ps[:N // 8 + 1].sum() / pp[:N // 8 + 1].sum()
    print(name, "total", ratio, "low", ratio_low, "theory", presets.power_gain(presets.PRESETS[name]))
    assert total[0] <= ratio <= total[1]
    assert ratio_low < low
    assert int(st[0, 48:56].view("<u8")[0]) == 0
    wcodes, wst = ref.shape(presets.PRESETS[name], x, 16, 7)
    assert np.array_equal(codes.astype(np.int64), wcodes) and wst["saturated"][0] == 0


@pytest.mark.parametrize("name,fmin,db20k,gain", [("lipshitz5", 4056.0, 18.7, 16.56), ("fweighted9", 3150.0, 25.5, 69.17), ("modified_e9", 3452.0, 13.2, 5.71)])
def test_preset_figures(name, fmin, db20k, gain):
    """The shipped psychoacoustic presets at 44.1 kHz: the NTF's minimum within 50 Hz, its gain at 20 kHz and 1 + sum c^2 within 1 %."""
    c = presets.PRESETS[name]
    f = np.arange(20.0, 22050.0, 1.0)
    at = f[np.argmin(presets.ntf_db(c, f, 44100.0))]
    g20 = presets.ntf_db(c, [20000.0], 44100.0)[0]
    print(name, at, g20, presets.power_gain(c))
    assert abs(at - fmin) <= 50.0
    assert abs(g20 - db20k) <= 0.01 * db20k
    assert abs(presets.power_gain(c) - gain) <= 0.01 * gain


def test_presets_and_rates():
    assert presets.resolve(None) is None and presets.resolve([]) is None
    assert presets.resolve("first", 96000.0) == [1.0] and presets.resolve([0.5, 0.25], 96000.0) == [0.5, 0.25]
    for name in presets.PSYCHOACOUSTIC:
        assert presets.resolve(name, 44100.0) == presets.PRESETS[name] == presets.resolve(name, 48000.0)
        with pytest.raises(ValueError):
            presets.resolve(name, 96000.0)
        assert ref.quantise_coeffs(presets.PRESETS[name]) is not None
    with pytest.raises(ValueError):
        presets.resolve("nonesuch", 44100.0)
    with pytest.raises(ValueError):
        presets.resolve([0.1] * 13)
    assert abs(presets.ntf_db([1.0], [11025.0], 44100.0)[0] - 20.0 * np.log10(np.sqrt(2.0))) < 1e-9


def _cxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++")):
        if c and os.path.exists(c):
            return c
    pytest.skip("no C++ compiler")


def test_kernel_schedule_emulated_lane_by_lane(tmp_path):
    """tests/native/noise_shape_host.cpp: phases A, B and C with the header's index functions against shape_host()."""
    exe = str(tmp_path / "noise_shape_host")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "noise_shape_host.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-3000:])
    out = json.loads(res.stdout.strip().splitlines()[-1])
    print(out)
    assert out["ok"] and out["failures"] == 0 and out["cases"] >= 100
    assert out["bank_conflicts"] == 0 and out["walk_steps"] > 0 and out["clipped"] > 0


def test_the_kernel_takes_its_indices_from_the_header():
    hip = open(os.path.join(CSRC, "noise_shape.hip")).read()
    for call in ("ns::tile_valid(", "ns::tile_count(", "ns::tile_first(", "ns::tiles_per_block(", "ns::group_channels(", "ns::group_count(", "ns::sample_index(",
                 "ns::sweep_row(", "ns::sweep_frame(", "ns::pair_dword(", "ns::code_dword(", "ns::split(", "ns::step(", "ns::dither_q8(", "ns::kPairDwords", "ns::kCodeDwords"):
        assert call in hip, call
