"""LPC subframes of FLAC delivery (option flac_lpc_order, elementary_amd/csrc/flac_lpc.h) without a GPU.

1. tests/native/flac_lpc_host.cpp: the encode kernel's LPC path emulated lane by lane against encode_frame_host(..., lpcOrder), byte
   for byte, plain and under the address and undefined-behaviour sanitizers (a stand-alone program, run directly).
   What the counts show: LPC chosen at both priced orders, FIXED beating LPC, escape partitions inside LPC subframes, and orders
   dropped because lag 0 is zero — all on frames. The other three reasons to drop an order (a non-positive error, a negative shift, a
   residual outside int32) did not occur on any frame of the 2607 cases, and for the first two that is no accident: while the error
   stays positive every reflection coefficient is below 1 in magnitude, the predictor is minimum-phase, and its coefficients are bounded
   by the binomial ones (924 at order 12) — measured on windowed signals they stay near 2 — so neither guard can trip on lags that come
   from samples. The program therefore drives those rules directly: lpc_design on lags no signal gives, lpc_quantise on coefficients no
   recursion gives, and for the overflow the +-full-scale alternating 24-bit side channel under a plan written by hand, through the
   lanes' tree and the twin's rows alike.
2. elemhip_flac_encode_lpc (the twin behind the C-ABI) through tests/flac_reference.py: lossless on every signal, order 0 gives
   elemhip_flac_encode's bytes, and a bright signal is coded as LPC throughout and comes out smaller.
3. The option on a dry handle: refused values, and the getter."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import flac_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elementary_amd", "csrc")


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
                    os.path.join(ROOT, "tests", "native", "flac_lpc_host.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-800:], res.stderr[-3000:])
    return json.loads(res.stdout.strip().splitlines()[-1]), res.stderr


def test_lpc_lane_schedule_gives_the_scalar_twins_bytes(tmp_path):
    out, _ = _build_and_run(tmp_path, "flac_lpc_host", [])
    print(out)
    assert out["ok"] and out["failures"] == 0
    # frames 256 and 4096 x G 1, 2, 3, 8 x 16 and 24 bits x P 1, 8, 12 x whole / 1 / 2 / P / P + 1 / 15 / 255 samples x the content kinds
    # (three per whole frame of 4096; every third start for G > 2), the alternating pairs, the constant blocks
    # (frames of 256: 7 sizes x 12 kinds for G 1, 2 and x 4 for G 3, 8; frames of 4096: 6 sizes likewise and 3 whole frames)
    assert out["cases"] == 6 * (2 * 84 + 2 * 28) + 6 * (2 * 75 + 2 * 27) + 2 * 3 * 3 * 2 + 3, out["cases"]
    assert out["lpc_half_order"] > 0 and out["lpc_full_order"] > 0                      # LPC chosen at both priced orders
    assert all(n > 0 for n in out["lpc_orders"][:5]) and out["lpc_orders"][5] == 0       # orders 1, 4, 6, 8, 12 and no other
    assert out["fixed_beats_lpc"] > 0 and out["lpc_escapes"] > 0 and out["constant"] > 0 and out["verbatim"] > 0
    assert out["drop_zero_lag"] > 0
    assert all(n > 0 for n in out["modes"])
    # the guards that lags from samples do not reach (see the module's text), driven directly
    assert all(n > 0 for n in out["design_drops"]) and out["forced_overflow"] == 1
    assert (out["drop_error"], out["drop_shift"], out["drop_overflow"]) == (0, 0, 0)


def test_lpc_emulation_is_clean_under_asan_and_ubsan(tmp_path):
    out, err = _build_and_run(tmp_path, "flac_lpc_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert out["ok"] and out["failures"] == 0, out["failures"]
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]


def test_the_kernel_takes_the_lpc_arithmetic_from_the_headers():
    hip = open(os.path.join(CSRC, "flac_encode.hip")).read()
    for call in ("fe::lpc_windowed(", "fe::lpc_lags(", "fe::lpc_design(", "fe::leaf_lpc(", "fe::lpc_row(", "fe::lpc_order_ok("):
        assert call in hip, call
    head = open(os.path.join(CSRC, "flac_encode.h")).read()
    assert '#include "flac_lpc.h"' in head
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "flac_lpc.h" in mk


# ---- 2. the twin through the decoder ---------------------------------------------------------------------------------------------------
def _signals(bits, n):
    lim = 1 << (bits - 1)
    i = np.arange(n)
    rng = np.random.default_rng(bits * 1000 + n)
    sine = np.rint(0.5 * lim * np.sin(2 * math.pi * 440.0 * i / 44100.0)).astype(np.int32)
    white = rng.integers(-lim, lim, size=n, dtype=np.int64).astype(np.int32)
    alt = np.where(i & 1, lim - 1, -lim).astype(np.int32)
    outlier = np.zeros(n, np.int32)
    outlier[n // 3] = lim - 1
    return {
        "silence": np.zeros((1, n), np.int32),
        "dc": np.full((1, n), -lim, np.int32),
        "ramp": ((i % 1000) - 500).astype(np.int32)[None, :],
        "sine": sine[None, :],
        "white": white[None, :],
        "alternating": alt[None, :],
        "alternating_stereo": np.stack([alt, -1 - alt]),          # L = +-full scale, R its mirror: the side channel needs all its 25 bits
        "equal": np.stack([sine, sine]),
        "opposite": np.stack([sine, -sine]),
        "outlier": outlier[None, :],
        "outlier_stereo": np.stack([outlier, white]),
    }


def _bright(bits, n, seed=5):
    """0.3 sin 5 kHz + 0.2 sin 9 kHz at 44.1 kHz, white noise 60 dB below full scale."""
    i = np.arange(n)
    rng = np.random.default_rng(seed)
    x = 0.3 * np.sin(2 * math.pi * 5000.0 * i / 44100.0) + 0.2 * np.sin(2 * math.pi * 9000.0 * i / 44100.0) + 1e-3 * rng.standard_normal(n)
    return np.rint(((1 << (bits - 1)) - 1) * x).astype(np.int32)[None, :]


@pytest.mark.parametrize("order", [1, 8, 12])
@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("ff", [256, 4096])
def test_twin_with_lpc_is_lossless_and_no_longer_than_the_format_allows(bits, ff, order):
    from elementary_amd.runtime import flac_encode
    n = 2 * ff + 100
    sig = _signals(bits, n)
    sig["bright"] = _bright(bits, n)
    for name, x in sig.items():
        data, lens = flac_encode(x, bits=bits, flac_frame=ff, sample_rate=44100, lpc_order=order)
        frames, chans = ref.decode_frames(data)
        G = x.shape[0]
        assert [f["bytes"] for f in frames] == lens.tolist() and sum(lens.tolist()) == len(data), name
        assert [f["blocksize"] for f in frames] == [ff, ff, 100] and [f["number"] for f in frames] == [0, 1, 2], name
        assert np.array_equal(np.array(chans, dtype=np.int64), x), name
        for f in frames:
            m, hb = f["blocksize"], f["header_bytes"]
            assert f["bytes"] <= hb + (G * (8 + bits * m) + 7) // 8 + 2, (name, f["number"])
            assert all(sub["bits"] <= 8 + sub["bps"] * m for sub in f["subframes"]), name
            assert all(sub["kind"] != "LPC" or sub["order"] in (order, (order + 1) // 2) for sub in f["subframes"]), name
            if name in ("silence", "dc"):
                assert f["subframes"][0]["kind"] == "CONSTANT", name
        base, _ = flac_encode(x, bits=bits, flac_frame=ff, sample_rate=44100)
        # every candidate's bits are a minimum over a superset of the FIXED-only candidates, and so is the cheapest stereo mode's sum
        assert len(data) <= len(base), (name, len(data), len(base))


@pytest.mark.parametrize("bits", [16, 24])
def test_order_0_gives_elemhip_flac_encodes_bytes(bits):
    import ctypes as C
    from elementary_amd.runtime import flac_encode, load_library
    lib = load_library()
    x = _signals(bits, 256 * 3 + 31)["outlier_stereo"]
    want, lens = flac_encode(x, bits=bits, flac_frame=256)
    cap = int(lib.elemhip_flac_bound(x.shape[1], 2, bits))
    out = np.zeros(cap, np.uint8)
    fb = np.zeros(8, np.uint32)
    keep = [np.ascontiguousarray(x[c]) for c in range(2)]
    rows = (C.POINTER(C.c_int32) * 2)(*[k.ctypes.data_as(C.POINTER(C.c_int32)) for k in keep])
    nb, nf = C.c_size_t(0), C.c_size_t(0)
    rc = lib.elemhip_flac_encode_lpc(rows, 2, x.shape[1], 256, bits, 44100, 0, 1, out.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(nb),
                                     fb.ctypes.data_as(C.POINTER(C.c_uint32)), 8, C.byref(nf), 0)
    assert rc == 0 and out[:nb.value].tobytes() == want and fb[:nf.value].tolist() == lens.tolist()
    rc = lib.elemhip_flac_encode_lpc(rows, 2, x.shape[1], 256, bits, 44100, 0, 1, out.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(nb),
                                     fb.ctypes.data_as(C.POINTER(C.c_uint32)), 8, C.byref(nf), 13)
    assert rc == 6


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("ff", [256, 4096])
def test_a_bright_signal_is_coded_as_lpc_and_comes_out_smaller(bits, ff):
    """Above about 5 kHz no FIXED predictor helps (FIXED 0 wins, barely under VERBATIM); an order-8 LPC predictor removes both tones."""
    from elementary_amd.runtime import flac_encode
    n = 3 * ff + 77
    x = _bright(bits, n)
    plain, _ = flac_encode(x, bits=bits, flac_frame=ff)
    lpc, _ = flac_encode(x, bits=bits, flac_frame=ff, lpc_order=8)
    frames, chans = ref.decode_frames(lpc)
    assert np.array_equal(np.array(chans, dtype=np.int64), x)
    whole = [f for f in frames if f["blocksize"] == ff]
    assert len(whole) == 3 and all(sub["kind"] == "LPC" and sub["order"] in (4, 8) for f in whole for sub in f["subframes"])
    print("bright", bits, ff, "lpc / fixed-only bytes", len(lpc) / len(plain), "lpc / pcm", len(lpc) / (n * bits // 8))
    assert len(lpc) < len(plain)
    base, _ = ref.decode_frames(plain)
    assert all(sub["kind"] in ("FIXED", "VERBATIM") for f in base for sub in f["subframes"])


def test_twin_cuts_frames_like_one_call_with_lpc():
    from elementary_amd.runtime import flac_encode
    x = np.concatenate([_bright(16, 256 * 5 + 77), _signals(16, 256 * 5 + 77)["white"]])
    whole, lens = flac_encode(x, flac_frame=256, lpc_order=12)
    a, la = flac_encode(x[:, :512], flac_frame=256, flush=False, lpc_order=12)
    b, lb = flac_encode(x[:, 512:], flac_frame=256, first_frame_number=2, lpc_order=12)
    assert a + b == whole and la.tolist() + lb.tolist() == lens.tolist()


def test_twin_refuses_orders_outside_0_to_12():
    from elementary_amd.runtime import flac_encode, ElemHipError
    for bad in (13, -1, 2.5, 1 << 40):
        with pytest.raises(ElemHipError) as e:
            flac_encode(np.zeros((1, 16), np.int32), lpc_order=bad)
        assert e.value.code == 6, bad


# ---- 3. the option on a dry handle -------------------------------------------------------------------------------------------------------
def test_option_values_on_a_dry_handle():
    from elementary_amd.runtime import Runtime, ElemHipError
    dry = Runtime(44100.0, 64, device=-1)
    assert dry.flac_read()["lpc_order"] == 0
    for good in (12, 1, 8, 0, 8.0):
        dry.set_option("flac_lpc_order", good)
        assert dry.flac_read()["lpc_order"] == int(good)
    for bad in (13, -1, 2.5, 1e9, float("nan"), float("inf")):
        with pytest.raises(ElemHipError) as e:
            dry.set_option("flac_lpc_order", bad)
        assert e.value.code == 6, bad
    assert dry.flac_read()["lpc_order"] == 8            # a refused value changes nothing
    dry.flac_reset()
    assert dry.flac_read()["lpc_order"] == 8            # the option outlives a programme
