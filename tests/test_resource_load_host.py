"""The resource loader without a GPU: elementary_amd/csrc/resource_load.h — the header resource_load.hip takes its arithmetic, its
pieces and every index from — compiled for the host and driven by tests/native/resource_load_host.cpp (both kernels emulated lane by
lane into poisoned rows against load_host(), once more under the address and undefined-behaviour sanitizers); load_host() through the
C-ABI of a handle without a device against tests/resource_load_reference.py, a float64 restatement of the specification; the centred
filter's alignment; the codes of a malformed source; a FLAC source and a frame with a broken CRC; keys and prune."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import flac_writer as fw
import pcm_unpack_reference as uref
import resource_load_reference as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elementary_amd", "csrc")
SR = 44100


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
                    os.path.join(ROOT, "tests", "native", "resource_load_host.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-3000:])
    return json.loads(res.stdout.strip().splitlines()[-1]), res.stderr


def _check_emulation(out):
    print(out)
    # 4 groups x 3 formats x 4 lengths x 5 rate pairs x 3 piece sizes, and 4 wide or long sources
    assert out["ok"] and out["failures"] == 0 and out["cases"] == 4 * 3 * 4 * 5 * 3 + 4, out["cases"]
    assert out["pieces"] > out["cases"]                       # (files were cut)
    assert out["wide_loads"] > 0 and out["wide_stores"] > 0 and out["narrow_stores"] > 0
    assert out["taps_96000_44100"] == 140
    # the copy kernel: pcm_pack.h's skewed rows — no half-wave hits a bank twice, writing transposed or reading quads
    assert out["half_wave_writes"] > 0 and out["write_conflicts"] == 0
    assert out["half_wave_reads"] > 0 and out["read_conflicts"] == 0
    # the converting kernel: resample.h's padded rows — a half-wave's tap read is 2-way at worst, and conflict-free when upsampling;
    # the narrow staging write 2-way at worst
    assert out["tap_reads"] > 0 and out["tap_over_2way"] == 0 and out["tap_upsampling_conflicts"] == 0
    assert out["stage_writes"] > 0 and out["stage_max_way"] <= 2


def test_lane_schedule_writes_every_frame_once_with_the_scalar_loops_bits(tmp_path):
    _check_emulation(_build_and_run(tmp_path, "resource_load_host", [])[0])


def test_lane_schedule_under_the_sanitizers(tmp_path):
    out, err = _build_and_run(tmp_path, "resource_load_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]
    _check_emulation(out)


# ---- through the C-ABI, a handle without a device -------------------------------------------------------------------------------------
def _dry(bs=128, **opts):
    from elementary_amd.runtime import Runtime
    rt = Runtime(SR, bs, device=-1)
    for k, v in opts.items():
        rt.set_option(k, v)
    return rt


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("fmt", ["s16", "s24", "f32"])
def test_same_rate_equals_the_reference_and_the_float_path(fmt):
    rt = _dry()
    for G, N in ((1, 1), (2, 257), (3, 1000), (8, 63)):
        stream = uref.random_streams(fmt, N, G, 1, 10 * G + N)[0]
        want = rref.decode(stream, fmt)
        name = f"{fmt}_{G}_{N}"
        assert rt.add_shared_resource_pcm(name, stream, fmt, G) is True
        assert rt.shared_resource_info(name) == {"channels": G, "frames": N}
        got = rt.shared_resource_read(name)
        assert np.array_equal(_bits(got), _bits(want)), (fmt, G, N)
        assert rt.add_shared_resource(name + "_f", want) and np.array_equal(_bits(rt.shared_resource_read(name + "_f")), _bits(got))
        assert np.array_equal(_bits(rt.shared_resource_read(name, G - 1, N // 2, N - N // 2)), _bits(want[G - 1, N // 2:]))


@pytest.mark.parametrize("fin", [48000, 96000, 22050])
def test_other_rate_stays_within_the_float32_bound_of_the_reference(fin):
    rt = _dry()
    for fmt, G, N in (("s16", 2, 257), ("s24", 1, 1000), ("f32", 3, 63), ("s16", 1, 1)):
        stream = uref.random_streams(fmt, N, G, 1, fin % 97 + N)[0]
        want, bound = rref.convert(rref.decode(stream, fmt), fin, SR)
        name = f"{fmt}_{G}_{N}"
        assert rt.add_shared_resource_pcm(name, stream, fmt, G, sample_rate=fin) is True
        assert rt.shared_resource_info(name) == {"channels": G, "frames": rref.out_frames(N, fin, SR)}
        got = rt.shared_resource_read(name).astype(np.float64)
        err = np.abs(got - want)
        print(fin, fmt, G, N, "worst error", float(err.max()), "of a bound of", float(bound.max()))
        assert got.shape == want.shape and bool((err <= bound).all()), (fin, fmt, G, N, float((err - bound).max()))


def test_the_filter_is_centred_a_sine_stays_in_place():
    """1 kHz at amplitude 0.5 from 48000 to 44100 Hz: every frame at least Wc input frames from either end of the file is the analytic
    sine at the new rate within the filter's pass-band figure (+-0.001 dB) plus the float32 accumulation bound."""
    fin, N, A = 48000, 4800, 0.5
    p = rref.plan(fin, SR)
    x = (A * np.sin(2 * np.pi * 1000.0 * np.arange(N) / fin)).astype(np.float32)
    rt = _dry()
    assert rt.add_shared_resource_pcm("sine", x[:, None], "f32", 1, sample_rate=fin)
    got = rt.shared_resource_read("sine", 0).astype(np.float64)
    n = np.arange(len(got))
    i0 = n * p["M"] // p["L"]
    inner = (i0 >= p["Wc"]) & (i0 + p["Wc"] <= N - 1)
    assert int(inner.sum()) > 4000
    want = A * np.sin(2 * np.pi * 1000.0 * n / SR)
    _, bound = rref.convert(x[None, :], fin, SR)
    ripple = A * (10.0 ** (0.001 / 20.0) - 1.0)
    dev = np.abs(got - want)[inner]
    print("worst deviation from the analytic sine", float(dev.max()), "allowed", ripple, "+", float(bound[0][inner].max()))
    assert bool((dev <= ripple + bound[0][inner]).all())


def test_frame_0_of_an_impulse_is_the_centre_tap():
    fin = 48000
    p = rref.plan(fin, SR)
    x = np.zeros((40, 1), dtype=np.float32)
    x[0, 0] = 0.5
    rt = _dry()
    assert rt.add_shared_resource_pcm("imp", x, "f32", 1, sample_rate=fin)
    got = rt.shared_resource_read("imp", 0)
    centre = np.float32(rref.prototype(0.0, p["L"], p["M"]))
    assert centre == np.float32(p["L"] / p["M"])                 # g(0) = s
    assert got[0] == np.float32(0.5) * centre and abs(got[0]) == np.abs(got).max()


def test_a_taken_name_inserts_nothing_and_leaves_the_old_floats():
    rt = _dry()
    old = np.arange(12, dtype=np.float32).reshape(2, 6)
    assert rt.add_shared_resource("x", old)
    stream = uref.random_streams("s16", 100, 2, 1, 3)[0]
    assert rt.add_shared_resource_pcm("x", stream, "s16", 2) is False
    assert np.array_equal(rt.shared_resource_read("x"), old)
    assert rt.add_shared_resource_pcm("y", stream, "s16", 2) is True and rt.add_shared_resource_pcm("y", stream[:50], "s16", 2) is False
    assert rt.shared_resource_info("y")["frames"] == 100


def _keys(rt):
    f = rt._lib.elemhip_shared_resource_keys_json
    f.argtypes, f.restype = [C.c_void_p, C.c_char_p, C.c_size_t], C.c_size_t
    buf = C.create_string_buffer(4096)
    f(rt._h, buf, 4096)
    return json.loads(buf.value.decode())


def test_malformed_sources_give_the_documented_codes_and_insert_nothing():
    from elementary_amd.runtime import ElemHipError, _ResourceSrc
    rt = _dry()
    data = np.zeros(64, dtype=np.int16)

    def call(fmt, channels, frames, nbytes, rate=0.0):
        src = _ResourceSrc()
        src.format, src.channels, src.sample_rate, src.frames, src.data, src.bytes = fmt, channels, rate, frames, data.ctypes.data, nbytes
        done = C.c_int(7)
        rc = rt._lib.elemhip_add_shared_resource_pcm(rt._h, b"bad", C.byref(src), C.byref(done))
        assert done.value == 0
        return rc

    assert call(0, 1, 8, 128) == 8 and call(5, 1, 8, 128) == 8          # a format outside 1 .. 4
    assert call(1, 0, 8, 128) == 8 and call(1, 33, 1, 128) == 8         # 0 or 33 channels
    assert call(1, 2, 32, 127) == 8                                     # a short byte count
    assert call(4, 2, 8, 128) == 8                                      # FLAC without its struct
    assert call(1, 1, 8, 128, 44101.0) == 6 and call(1, 1, 8, 128, 1000.5) == 6 and call(1, 1, 8, 128, 4000.0) == 6      # no plan: L, a fraction, L > 8 M
    with pytest.raises(ElemHipError) as e:
        rt.shared_resource_info("nothing")
    assert e.value.code == 6
    with pytest.raises(ElemHipError):
        rt.set_option("resource_load_frames", 63)
    rt.set_option("resource_load_frames", 64)
    assert "bad" not in _keys(rt)


def _flac(bits, n=1000, seed=5):
    from elementary_amd.runtime import FlacChunk, flac_index
    chans = [fw._noise(n, bits, seed + c) for c in range(2)]
    data = fw.write_stream(chans, bits, 256)
    off, first = flac_index(data, 2, bits, 256)
    pcm = np.array(chans, dtype=np.int32).T
    stream = pcm.astype(np.int16) if bits == 16 else uref.s24_bytes(pcm)
    return data, off, first, stream, lambda d: FlacChunk(np.frombuffer(bytes(d), dtype=np.uint8), off, first, 2, bits, n, 0, n)


@pytest.mark.parametrize("bits", [16, 24])
def test_flac_source_equals_the_pcm_of_the_same_samples(bits):
    data, off, first, stream, chunk = _flac(bits)
    fmt = "s16" if bits == 16 else "s24"
    rt = _dry()
    for rate in (None, 48000):
        assert rt.add_shared_resource_pcm(f"f{rate}", chunk(data), sample_rate=rate) and rt.add_shared_resource_pcm(f"p{rate}", stream, fmt, 2, sample_rate=rate)
        a, b = rt.shared_resource_read(f"f{rate}"), rt.shared_resource_read(f"p{rate}")
        assert a.shape == (2, 1000 if rate is None else rref.out_frames(1000, 48000, SR)) and np.array_equal(_bits(a), _bits(b))


def test_a_broken_flac_crc_gives_106_names_the_frame_and_inserts_nothing():
    from elementary_amd.runtime import ElemHipError
    data, off, first, stream, chunk = _flac(16)
    bad = bytearray(data)
    bad[int(off[3]) - 1] ^= 1                                 # the CRC-16 of frame 2
    rt = _dry()
    with pytest.raises(ElemHipError) as e:
        rt.add_shared_resource_pcm("broken", chunk(bad))
    err = rt.flac_in_error()
    assert e.value.code == 106 and err["frame"] == 2 and err["reason"] == 1 and "broken" not in _keys(rt)


def test_keys_list_the_name_and_prune_removes_it():
    rt = _dry()
    assert rt.add_shared_resource_pcm("kept", uref.random_streams("s16", 10, 1, 1, 1)[0], "s16", 1)
    assert "kept" in _keys(rt)
    rt.prune_shared_resources()
    assert "kept" not in _keys(rt)


def test_the_piece_size_does_not_change_the_bits():
    stream = uref.random_streams("s24", 1000, 3, 1, 77)[0]
    got = []
    for frames in (64, 256, 1 << 20):
        rt = _dry(resource_load_frames=frames)
        assert rt.add_shared_resource_pcm("r", stream, "s24", 3, sample_rate=96000)
        got.append(_bits(rt.shared_resource_read("r")))
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
