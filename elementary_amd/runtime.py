"""``Runtime`` — host-side mirror of ``elem::Runtime<float>`` backed by libelemhip.so (HIP, gfx950).

There is no CPU fallback: constructing a ``Runtime`` without the compiled extension or without
a usable GPU raises.  Method names/arguments follow the reference class
(runtime/elem/Runtime.h:39-153); see ``_cabi.CRuntime`` for the shared surface.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Any, Dict, Optional

from ._cabi import CRuntime, RETURN_CODES

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libelemhip.so")
_lib: Optional[C.CDLL] = None


class ElemHipError(RuntimeError):
    pass


def sum_buses(dst_ptr: int, partial_ptrs, num_floats: int, device: int = 0, hip_stream: int = 0) -> None:
    """``elemhip_sum_buses``: dst = ((partials[0] + partials[1]) + ...) in the order given — the rank-ordered, bit-reproducible
    sum of the ranks' output buses once they sit on one device (raw device pointers, ``num_floats`` float32 each)."""
    lib = load_library()
    arr = (C.c_void_p * len(partial_ptrs))(*[C.c_void_p(p) for p in partial_ptrs])
    rc = lib.elemhip_sum_buses(int(device), C.c_void_p(hip_stream or None), C.c_void_p(dst_ptr), arr, len(partial_ptrs), int(num_floats))
    if rc != 0:
        raise ElemHipError(f"elemhip_sum_buses failed: {describe(rc)} (code {rc})")


def load_library() -> C.CDLL:
    """Load the in-tree HIP engine. Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ElemHipError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C elementary_amd/csrc`). The HIP engine has no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        lib.elemhip_create.argtypes = [C.c_double, C.c_int, C.c_int]
        lib.elemhip_create.restype = C.c_void_p
        lib.elemhip_last_create_error.restype = C.c_int
        lib.elemhip_describe.argtypes = [C.c_int]
        lib.elemhip_describe.restype = C.c_char_p
        lib.elemhip_process_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int64]
        lib.elemhip_process_blocks.restype = C.c_int
        _fpp = C.POINTER(C.POINTER(C.c_float))
        lib.elemhip_process_blocks_host.argtypes = [C.c_void_p, _fpp, C.c_size_t, _fpp, C.c_size_t, C.c_size_t, C.c_int64]
        lib.elemhip_process_blocks_host.restype = C.c_int
        lib.elemhip_process_blocks_pcm.argtypes = [C.c_void_p, _fpp, C.c_size_t, C.POINTER(C.c_void_p), C.c_size_t, _fpp, C.c_size_t, C.c_int64,
                                                   C.POINTER(_PcmSpec), C.POINTER(_PcmChannelStats)]
        lib.elemhip_process_blocks_pcm.restype = C.c_int
        lib.elemhip_process_blocks_pcm_io.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(_PcmInSpec), C.POINTER(C.c_void_p), C.c_size_t,
                                                      C.POINTER(_PcmSpec), _fpp, C.c_size_t, C.c_size_t, C.c_int64, C.POINTER(_PcmChannelStats)]
        lib.elemhip_process_blocks_pcm_io.restype = C.c_int
        lib.elemhip_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        lib.elemhip_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        lib.elemhip_get_stats.argtypes = [C.c_void_p, C.c_void_p]
        lib.elemhip_time_launches.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_float), C.c_size_t]
        lib.elemhip_time_launches.restype = C.c_int
        lib.elemhip_describe_plan.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        lib.elemhip_describe_plan.restype = C.c_size_t
        lib.elemhip_sum_buses.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.c_size_t]
        lib.elemhip_sum_buses.restype = C.c_int
        _dp = C.POINTER(C.c_double)
        lib.elemhip_loudness_read.argtypes = [C.c_void_p, C.POINTER(_LoudnessInfo), _dp, C.c_size_t, _dp, C.POINTER(C.c_float)]
        lib.elemhip_loudness_read.restype = C.c_int
        lib.elemhip_loudness_reset.argtypes = [C.c_void_p]
        lib.elemhip_loudness_reset.restype = C.c_int
        lib.elemhip_loudness_gate.argtypes = [_dp, C.c_size_t, C.c_size_t, _dp, C.POINTER(_LoudnessResult)]
        lib.elemhip_loudness_gate.restype = C.c_int
        lib.elemhip_resample_frames.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        lib.elemhip_resample_frames.restype = C.c_int
        lib.elemhip_resample_read.argtypes = [C.c_void_p, C.POINTER(_ResampleInfo)]
        lib.elemhip_resample_read.restype = C.c_int
        lib.elemhip_resample_reset.argtypes = [C.c_void_p]
        lib.elemhip_resample_reset.restype = C.c_int
        lib.elemhip_input_resample_frames.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        lib.elemhip_input_resample_frames.restype = C.c_int
        lib.elemhip_input_resample_read.argtypes = [C.c_void_p, C.POINTER(_ResampleInfo)]
        lib.elemhip_input_resample_read.restype = C.c_int
        lib.elemhip_input_resample_reset.argtypes = [C.c_void_p]
        lib.elemhip_input_resample_reset.restype = C.c_int
        lib.elemhip_limiter_read.argtypes = [C.c_void_p, C.POINTER(_LimiterInfo), _dp, C.POINTER(C.c_uint64), C.c_size_t]
        lib.elemhip_limiter_read.restype = C.c_int
        lib.elemhip_limiter_reset.argtypes = [C.c_void_p]
        lib.elemhip_limiter_reset.restype = C.c_int
        _vpp, _szp, _u32p = C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)
        lib.elemhip_process_blocks_flac.argtypes = [C.c_void_p, _vpp, C.c_size_t, C.POINTER(_PcmInSpec), _vpp, _szp, _szp, C.c_size_t,
                                                    C.POINTER(_FlacSpec), C.c_size_t, C.c_int64, C.POINTER(_PcmChannelStats)]
        lib.elemhip_process_blocks_flac.restype = C.c_int
        lib.elemhip_flac_bound.argtypes = [C.c_size_t, C.c_uint32, C.c_uint32]
        lib.elemhip_flac_bound.restype = C.c_size_t
        lib.elemhip_flac_flush.argtypes = [C.c_void_p, _vpp, _szp, _szp, C.c_size_t]
        lib.elemhip_flac_flush.restype = C.c_int
        lib.elemhip_flac_read.argtypes = [C.c_void_p, C.POINTER(_FlacInfo), C.POINTER(_FlacStreamInfo), C.c_size_t, _u32p, C.c_size_t]
        lib.elemhip_flac_read.restype = C.c_int
        lib.elemhip_flac_reset.argtypes = [C.c_void_p]
        lib.elemhip_flac_reset.restype = C.c_int
        lib.elemhip_flac_encode.argtypes = [C.POINTER(C.POINTER(C.c_int32)), C.c_uint32, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                            C.POINTER(C.c_uint8), C.c_size_t, _szp, _u32p, C.c_size_t, _szp]
        lib.elemhip_flac_encode.restype = C.c_int
        lib.elemhip_flac_encode_lpc.argtypes = lib.elemhip_flac_encode.argtypes + [C.c_uint32]
        lib.elemhip_flac_encode_lpc.restype = C.c_int
        lib.elemhip_flac_lpc_order.argtypes = [C.c_void_p, _u32p]
        lib.elemhip_flac_lpc_order.restype = C.c_int
        _u8p = C.POINTER(C.c_uint8)
        lib.elemhip_flac_md5.argtypes = [C.c_void_p, _u8p, C.c_size_t, _u32p]
        lib.elemhip_flac_md5.restype = C.c_int
        lib.elemhip_flac_md5_record_bytes.argtypes = []
        lib.elemhip_flac_md5_record_bytes.restype = C.c_size_t
        lib.elemhip_flac_md5_init.argtypes = [_u8p]
        lib.elemhip_flac_md5_init.restype = C.c_int
        lib.elemhip_flac_md5_update.argtypes = [_u8p, C.POINTER(C.POINTER(C.c_int32)), C.c_uint32, C.c_size_t, C.c_uint32]
        lib.elemhip_flac_md5_update.restype = C.c_int
        lib.elemhip_flac_md5_final.argtypes = [_u8p, _u8p]
        lib.elemhip_flac_md5_final.restype = C.c_int
        _u64p = C.POINTER(C.c_uint64)
        _fp, _i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        lib.elemhip_noise_shape_set.argtypes = [C.c_void_p, _fp, C.c_uint32]
        lib.elemhip_noise_shape_set.restype = C.c_int
        lib.elemhip_noise_shape_read.argtypes = [C.c_void_p, C.POINTER(_NoiseShapeInfo), _i32p, _u64p, C.c_size_t]
        lib.elemhip_noise_shape_read.restype = C.c_int
        lib.elemhip_noise_shape_reset.argtypes = [C.c_void_p]
        lib.elemhip_noise_shape_reset.restype = C.c_int
        lib.elemhip_noise_shape_state_bytes.argtypes = []
        lib.elemhip_noise_shape_state_bytes.restype = C.c_size_t
        lib.elemhip_noise_shape_host.argtypes = [_fp, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_int64, _fp, C.c_uint32, C.c_size_t,
                                                 C.c_size_t, _u8p, _i32p]
        lib.elemhip_noise_shape_host.restype = C.c_int
        _spp = C.POINTER(_SpectrumSpec)
        lib.elemhip_spectrum_set.argtypes = [C.c_void_p, _spp]
        lib.elemhip_spectrum_set.restype = C.c_int
        lib.elemhip_spectrum_read.argtypes = [C.c_void_p, C.POINTER(_SpectrumInfo), _fp, C.c_size_t, _dp, C.c_size_t]
        lib.elemhip_spectrum_read.restype = C.c_int
        lib.elemhip_spectrum_flush.argtypes = [C.c_void_p]
        lib.elemhip_spectrum_flush.restype = C.c_int
        lib.elemhip_spectrum_reset.argtypes = [C.c_void_p]
        lib.elemhip_spectrum_reset.restype = C.c_int
        lib.elemhip_spectrum_frames.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_uint64, C.c_int]
        lib.elemhip_spectrum_frames.restype = C.c_uint64
        lib.elemhip_spectrum_host.argtypes = [_spp, _fp, C.c_uint32, C.c_size_t, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64, _fp, _dp, _fp]
        lib.elemhip_spectrum_host.restype = C.c_int
        lib.elemhip_spectrum_launches.argtypes = []
        lib.elemhip_spectrum_launches.restype = C.c_uint64
        _qsp, _qcp = C.POINTER(_QcSpec), C.POINTER(_QcChannel)
        lib.elemhip_qc_set.argtypes = [C.c_void_p, _qsp]
        lib.elemhip_qc_set.restype = C.c_int
        lib.elemhip_qc_read.argtypes = [C.c_void_p, C.POINTER(_QcInfo), _qcp, C.c_size_t, _dp, C.c_size_t]
        lib.elemhip_qc_read.restype = C.c_int
        lib.elemhip_qc_overview.argtypes = [C.c_void_p, _fp, C.c_size_t]
        lib.elemhip_qc_overview.restype = C.c_int
        lib.elemhip_qc_reset.argtypes = [C.c_void_p]
        lib.elemhip_qc_reset.restype = C.c_int
        lib.elemhip_qc_state_bytes.argtypes = [C.c_uint32, C.c_uint32]
        lib.elemhip_qc_state_bytes.restype = C.c_size_t
        lib.elemhip_qc_host.argtypes = [_qsp, _fp, C.c_uint32, C.c_size_t, C.c_size_t, C.c_uint64, _u8p, _qcp, _dp, _fp]
        lib.elemhip_qc_host.restype = C.c_int
        lib.elemhip_qc_launches.argtypes = []
        lib.elemhip_qc_launches.restype = C.c_uint64
        _app = C.POINTER(_AutomationPoint)
        lib.elemhip_automation_set.argtypes = [C.c_void_p, C.c_uint32, _app, C.c_size_t]
        lib.elemhip_automation_set.restype = C.c_int
        lib.elemhip_automation_read.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(_AutomationInfo), _app, C.c_size_t]
        lib.elemhip_automation_read.restype = C.c_int
        lib.elemhip_automation_reset.argtypes = [C.c_void_p]
        lib.elemhip_automation_reset.restype = C.c_int
        lib.elemhip_automation_host.argtypes = [_app, C.c_size_t, C.c_int64, C.c_size_t, _fp]
        lib.elemhip_automation_host.restype = C.c_int
        lib.elemhip_automation_segment_at.argtypes = [_app, C.c_size_t, C.c_int64]
        lib.elemhip_automation_segment_at.restype = C.c_int64
        lib.elemhip_automation_launches.argtypes = []
        lib.elemhip_automation_launches.restype = C.c_uint64
        lib.elemhip_flac_index.argtypes = [C.POINTER(C.c_uint8), C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, _u64p, _u64p, C.c_size_t, _szp]
        lib.elemhip_flac_index.restype = C.c_int
        lib.elemhip_flac_decode.argtypes = [C.POINTER(_FlacIn), C.c_size_t, C.POINTER(C.POINTER(C.c_int32)), _szp, _u32p]
        lib.elemhip_flac_decode.restype = C.c_int
        lib.elemhip_flac_in_error.argtypes = [C.c_void_p, _u32p, _u64p, _u32p]
        lib.elemhip_flac_in_error.restype = C.c_int
        lib.elemhip_flac_in_md5.argtypes = [C.c_void_p, _u8p, _u32p, _u64p, C.c_size_t, _szp]
        lib.elemhip_flac_in_md5.restype = C.c_int
        lib.elemhip_flac_in_md5_reset.argtypes = [C.c_void_p]
        lib.elemhip_flac_in_md5_reset.restype = C.c_int
        lib.elemhip_flac_in_md5_update.argtypes = [_u8p, C.POINTER(C.POINTER(C.c_int32)), C.c_uint32, C.c_size_t, C.c_uint32]
        lib.elemhip_flac_in_md5_update.restype = C.c_int
        lib.elemhip_shared_resource_md5.argtypes = [C.c_void_p, C.c_char_p, _u8p, _u32p]
        lib.elemhip_shared_resource_md5.restype = C.c_int
        lib.elemhip_add_shared_resource_pcm.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(_ResourceSrc), C.POINTER(C.c_int)]
        lib.elemhip_add_shared_resource_pcm.restype = C.c_int
        lib.elemhip_shared_resource_info.argtypes = [C.c_void_p, C.c_char_p, _u32p, _u64p]
        lib.elemhip_shared_resource_info.restype = C.c_int
        lib.elemhip_shared_resource_read.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_float)]
        lib.elemhip_shared_resource_read.restype = C.c_int
        _lib = lib
    return _lib


class _AutomationPoint(C.Structure):
    _fields_ = [("frame", C.c_int64), ("value", C.c_float), ("curve", C.c_uint32)]


class _AutomationInfo(C.Structure):
    _fields_ = [("lanes", C.c_uint32), ("inputs", C.c_uint32), ("count", C.c_uint64)]


def _automation_points(points):
    """``(frame, value[, curve])`` rows as a ctypes array of ``_AutomationPoint`` and their count."""
    from . import automation as au
    pts = au.normalise(points)
    arr = (_AutomationPoint * max(1, len(pts)))()
    for i, (f, v, c) in enumerate(pts):
        if not -(1 << 63) <= f < (1 << 63):
            raise ValueError(f"frame {f} does not fit 64 bits")
        arr[i].frame, arr[i].curve = f, c
        # (a value float32 cannot hold goes in as the infinity it rounds to: the engine refuses it)
        arr[i].value = v if v != v or abs(v) <= 3.4028235677973366e38 else (float("inf") if v > 0 else float("-inf"))
    return arr, len(pts)


def automation_host(points, t0: int, n: int):
    """``elemhip_automation_host``: the scalar twin of the automation kernel, pure host arithmetic — float32 ``[n]``, the lane's value
    at frames ``t0 .. t0 + n - 1``. Raises with ``.code`` 6 for a lane the engine refuses."""
    import numpy as np
    arr, count = _automation_points(points)
    out = np.zeros(max(int(n), 0), dtype=np.float32)
    rc = load_library().elemhip_automation_host(arr, count, int(t0), out.size, out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != 0:
        err = ElemHipError(f"elemhip_automation_host failed: {describe(rc)} (code {rc})")
        err.code = rc
        raise err
    return out


def automation_segment_at(points, t: int) -> int:
    """``elemhip_automation_segment_at``: the index of the last point whose frame is ``<= t`` (-1 before the first)."""
    arr, count = _automation_points(points)
    return int(load_library().elemhip_automation_segment_at(arr, count, int(t)))


def automation_launches() -> int:
    """``elemhip_automation_launches``: automation kernels this process has launched so far (an engine without lanes adds none)."""
    return int(load_library().elemhip_automation_launches())


class _PcmSpec(C.Structure):
    _fields_ = [("format", C.c_uint32), ("channels_per_stream", C.c_uint32), ("dither", C.c_uint32), ("seed", C.c_uint32)]


class _PcmInSpec(C.Structure):
    _fields_ = [("format", C.c_uint32), ("channels_per_stream", C.c_uint32)]


class _PcmChannelStats(C.Structure):
    _fields_ = [("peak", C.c_float), ("reserved", C.c_uint32), ("over", C.c_uint64), ("nonfinite", C.c_uint64)]


class _LoudnessInfo(C.Structure):
    _fields_ = [("channels", C.c_uint32), ("hop", C.c_uint32), ("sub_blocks", C.c_uint64), ("frames", C.c_uint64)]


class _ResampleInfo(C.Structure):
    _fields_ = [("up", C.c_uint32), ("down", C.c_uint32), ("taps", C.c_uint32), ("latency_frames", C.c_uint32),
                ("frames_in", C.c_uint64), ("frames_out", C.c_uint64)]


class _LimiterInfo(C.Structure):
    _fields_ = [("lookahead_frames", C.c_uint32), ("latency_frames", C.c_uint32), ("release_frames", C.c_uint32), ("link", C.c_uint32),
                ("groups", C.c_uint32), ("reserved", C.c_uint32), ("frames", C.c_uint64)]


class _FlacSpec(C.Structure):
    _fields_ = [("bits", C.c_uint32), ("channels_per_stream", C.c_uint32), ("dither", C.c_uint32), ("seed", C.c_uint32),
                ("drop", C.c_uint64), ("take", C.c_uint64)]


class _FlacInfo(C.Structure):
    _fields_ = [("flac_frame", C.c_uint32), ("bits", C.c_uint32), ("channels_per_stream", C.c_uint32), ("streams", C.c_uint32),
                ("sample_rate", C.c_uint32), ("flushed", C.c_uint32), ("frames", C.c_uint64)]


class _FlacStreamInfo(C.Structure):
    _fields_ = [("frames", C.c_uint64), ("total_samples", C.c_uint64), ("min_frame_bytes", C.c_uint32), ("max_frame_bytes", C.c_uint32)]


def flac_encode(codes, bits: int = 16, flac_frame: int = 4096, sample_rate: int = 44100, first_frame_number: int = 0, flush: bool = True,
                lpc_order: int = 0):
    """``elemhip_flac_encode``: the scalar twin of the FLAC kernels, pure host arithmetic — ``codes`` int32 ``[channels, frames]`` (one
    stream) -> ``(frame bytes back to back, uint32 array of the frames' byte lengths)``. Whole frames of ``flac_frame``; with ``flush``
    the remainder as one short final frame. ``lpc_order`` (0 .. 12; ``elemhip_flac_encode_lpc``): the twin of a programme with option
    ``flac_lpc_order``; 0 gives ``elemhip_flac_encode``'s bytes."""
    import numpy as np
    lib = load_library()
    a = np.ascontiguousarray(codes, dtype=np.int32)
    if a.ndim == 1:
        a = a[None, :]
    ch, n = int(a.shape[0]), int(a.shape[1])
    cap = int(lib.elemhip_flac_bound(n, max(ch, 1), int(bits)))
    out = np.zeros(cap, dtype=np.uint8)
    count = n // max(int(flac_frame), 1) + 2
    lens = np.zeros(count, dtype=np.uint32)
    rows = (C.POINTER(C.c_int32) * max(1, ch))(*[a[c].ctypes.data_as(C.POINTER(C.c_int32)) for c in range(ch)])
    nbytes, nframes = C.c_size_t(0), C.c_size_t(0)
    args = (rows, ch, n, int(flac_frame), int(bits), int(sample_rate), int(first_frame_number), 1 if flush else 0,
            out.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(nbytes), lens.ctypes.data_as(C.POINTER(C.c_uint32)), count, C.byref(nframes))
    if int(lpc_order) != lpc_order or not 0 <= int(lpc_order) <= 0xFFFFFFFF:
        rc = 6          # (what the C side answers to an order above 12: kInvalidPropertyValue)
    else:
        rc = lib.elemhip_flac_encode_lpc(*args, int(lpc_order)) if lpc_order else lib.elemhip_flac_encode(*args)
    if rc != 0:
        err = ElemHipError(f"elemhip_flac_encode failed: {describe(rc)} (code {rc})")
        err.code = rc
        raise err
    return out[:nbytes.value].tobytes(), lens[:nframes.value].copy()


class _NoiseShapeInfo(C.Structure):
    _fields_ = [("taps", C.c_uint32), ("channels", C.c_uint32), ("frames", C.c_uint64)]


def noise_shape_host(coeffs, x, bits: int = 16, dither_seed: Optional[int] = None, channel0: int = 0, time0: int = 0, state=None):
    """``elemhip_noise_shape_host``: the scalar twin of the noise-shaping kernel, pure host arithmetic — ``x`` float32
    ``[channels, frames]`` at absolute frame ``time0`` (row c = channel ``channel0 + c`` of the dither's key) -> ``(codes, state)``:
    int32 ``[channels, frames]`` and the carried state, uint8 ``[channels, 64]`` (int32 ``e[12]`` newest first, uint64 ``saturated``,
    8 bytes reserved). ``state``: the one a former call returned, or None at a programme's start. ``dither_seed`` None: no dither."""
    import numpy as np
    lib = load_library()
    a = np.ascontiguousarray(x, dtype=np.float32)
    if a.ndim == 1:
        a = a[None, :]
    ch, n = a.shape
    c = np.ascontiguousarray(coeffs, dtype=np.float32).reshape(-1)
    sb = int(lib.elemhip_noise_shape_state_bytes())
    st = np.zeros((ch, sb), dtype=np.uint8) if state is None else np.array(state, dtype=np.uint8).reshape(ch, sb)
    codes = np.zeros((ch, n), dtype=np.int32)
    fp = C.POINTER(C.c_float)
    rc = lib.elemhip_noise_shape_host(c.ctypes.data_as(fp), c.size, int(bits), 0 if dither_seed is None else 1,
                                      0 if dither_seed is None else int(dither_seed) & 0xFFFFFFFF, int(channel0), int(time0), a.ctypes.data_as(fp), ch,
                                      max(n, 1), n, st.ctypes.data_as(C.POINTER(C.c_uint8)), codes.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        err = ElemHipError(f"elemhip_noise_shape_host failed: {describe(rc)} (code {rc})")
        err.code = rc
        raise err
    return codes, st


class _SpectrumSpec(C.Structure):
    _fields_ = [("size", C.c_uint32), ("hop", C.c_uint32), ("center", C.c_uint32), ("bands", C.c_uint32), ("window", C.POINTER(C.c_double)),
                ("band_first", C.POINTER(C.c_uint32)), ("band_count", C.POINTER(C.c_uint32)), ("weights", C.POINTER(C.c_float))]


class _SpectrumInfo(C.Structure):
    _fields_ = [("channels", C.c_uint32), ("columns", C.c_uint32), ("size", C.c_uint32), ("hop", C.c_uint32), ("center", C.c_uint32),
                ("bands", C.c_uint32), ("flushed", C.c_uint32), ("reserved", C.c_uint32), ("first_frame", C.c_uint64), ("queued", C.c_uint64),
                ("frames", C.c_uint64), ("delivered", C.c_uint64)]


def _spectrum_spec(size: int, hop: int, window="hann", bands=None, center: bool = False):
    """``(spec, keep)``: the C struct of an analyser spec and the arrays it points into (keep them alive for the call)."""
    import numpy as np
    from . import spectrum as sp
    if isinstance(window, str):
        if int(size) not in sp.SIZES:          # (the engine refuses the size; a table of some length lets it say so)
            win = np.ones(max(int(size), 1), dtype=np.float64)
        else:
            win = sp.window(window, int(size))
    else:
        win = np.ascontiguousarray(window, dtype=np.float64).reshape(-1)
        if win.size != int(size):
            raise ValueError(f"the window holds {win.size} values, the size is {size}")
    win = np.ascontiguousarray(win, dtype=np.float64)
    spec = _SpectrumSpec()
    spec.size, spec.hop, spec.center = int(size), int(hop), 1 if center else 0
    spec.window = win.ctypes.data_as(C.POINTER(C.c_double))
    keep = [win]
    if bands is not None:
        first, count, weights = sp.pack_rows(bands)
        if first.size == 0:
            raise ValueError("bands: at least one row (None: power mode)")
        if weights.size == 0:
            weights = np.zeros(1, dtype=np.float32)
        spec.bands = int(first.size)
        spec.band_first = first.ctypes.data_as(C.POINTER(C.c_uint32))
        spec.band_count = count.ctypes.data_as(C.POINTER(C.c_uint32))
        spec.weights = weights.ctypes.data_as(C.POINTER(C.c_float))
        keep += [first, count, weights]
    return spec, keep


def spectrum_frames(size: int, hop: int, center: bool, delivered: int, flushed: bool = False) -> int:
    """``elemhip_spectrum_frames``: the analyser frames out after ``delivered`` programme frames, or after a flush behind them."""
    return int(load_library().elemhip_spectrum_frames(int(size), int(hop), 1 if center else 0, int(delivered), 1 if flushed else 0))


def spectrum_launches() -> int:
    """``elemhip_spectrum_launches``: analyser kernels this process has launched so far (an engine whose analyser is off adds none)."""
    return int(load_library().elemhip_spectrum_launches())


def spectrum_host(x, size: int, hop: int, window="hann", bands=None, center: bool = False, flush: bool = True, state=None):
    """``elemhip_spectrum_host``: the scalar twin of the analyser's kernels, pure host arithmetic — ``x`` float32 ``[channels, frames]``
    delivered behind the programme ``state`` describes (None: a programme's start) -> ``(frames, sums, state)``: float32
    ``[channels, n, columns]``, float64 ``[channels, columns]`` and the carried state, a dict of ``tail`` float32
    ``[channels, size - 1]``, ``sums``, ``delivered`` and ``emitted``. With ``flush`` the frames zero padding completes are included and
    the returned state is None."""
    import numpy as np
    lib = load_library()
    a = np.ascontiguousarray(x, dtype=np.float32)
    if a.ndim == 1:
        a = a[None, :]
    ch, n = a.shape
    spec, keep = _spectrum_spec(size, hop, window, bands, center)
    cols = int(spec.bands) if spec.bands else int(size) // 2 + 1
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)

    def call(planar, frames, n0, j0, j1, tail, sums):
        out = np.zeros((ch, max(j1 - j0, 0), cols), dtype=np.float32)
        rc = lib.elemhip_spectrum_host(C.byref(spec), planar.ctypes.data_as(fp) if frames else None, ch, max(n, 1), frames, n0, j0, j1,
                                       tail.ctypes.data_as(fp), sums.ctypes.data_as(dp), out.ctypes.data_as(fp))
        if rc != 0:
            err = ElemHipError(f"elemhip_spectrum_host failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err
        return out

    if state is None:
        tail, sums, n0, j0 = np.zeros((ch, int(size) - 1), dtype=np.float32), np.zeros((ch, cols), dtype=np.float64), 0, 0
    else:
        tail = np.array(state["tail"], dtype=np.float32).reshape(ch, int(size) - 1)
        sums = np.array(state["sums"], dtype=np.float64).reshape(ch, cols)
        n0, j0 = int(state["delivered"]), int(state["emitted"])
    j1 = spectrum_frames(size, hop, center, n0 + n)
    parts = [call(a, n, n0, j0, j1, tail, sums)]
    if flush:
        j2 = spectrum_frames(size, hop, center, n0 + n, True)
        parts.append(call(a, 0, n0 + n, j1, j2, tail, sums))
    frames = np.concatenate(parts, axis=1)
    del keep
    return frames, sums, (None if flush else {"tail": tail, "sums": sums, "delivered": n0 + n, "emitted": j1})


class _QcSpec(C.Structure):
    _fields_ = [("silence_level", C.c_float), ("clip_level", C.c_float), ("clip_run", C.c_uint32), ("dropout_frames", C.c_uint32),
                ("bucket", C.c_uint32), ("num_pairs", C.c_uint32), ("pairs", C.POINTER(C.c_uint32)), ("skip", C.c_uint64), ("limit", C.c_uint64)]


class _QcInfo(C.Structure):
    _fields_ = [("channels", C.c_uint32), ("pairs", C.c_uint32), ("bucket", C.c_uint32), ("reserved", C.c_uint32), ("frames", C.c_uint64),
                ("delivered", C.c_uint64), ("first_bucket", C.c_uint64), ("queued", C.c_uint64)]


class _QcRuns(C.Structure):
    _fields_ = [("count", C.c_uint64), ("longest", C.c_uint64), ("longest_at", C.c_uint64), ("first_at", C.c_uint64)]


class _QcChannel(C.Structure):
    _fields_ = [("frames", C.c_uint64), ("nonfinite", C.c_uint64), ("quiet_frames", C.c_uint64), ("clipped_frames", C.c_uint64),
                ("peak_at", C.c_uint64), ("head_silence", C.c_uint64), ("tail_silence", C.c_uint64), ("dropouts", _QcRuns),
                ("clip_events", _QcRuns), ("sum", C.c_double), ("sum_sq", C.c_double), ("min", C.c_float), ("max", C.c_float),
                ("bucket_min", C.c_float), ("bucket_max", C.c_float), ("bucket_frames", C.c_uint32), ("reserved", C.c_uint32)]


QC_DEFAULTS = {"silence_level": 0.0, "clip_level": 1.0, "clip_run": 3, "dropout_frames": 64, "bucket": 0, "pairs": (), "skip": 0, "limit": 0}


def _qc_spec(params: Dict[str, Any]):
    """``(spec, keep)``: the C struct of an inspector spec (``QC_DEFAULTS`` under the caller's keys) and the array it points into."""
    import numpy as np
    unknown = set(params) - set(QC_DEFAULTS)
    if unknown:
        raise ValueError(f"qc: unknown keys {sorted(unknown)}; known: {sorted(QC_DEFAULTS)}")
    p = dict(QC_DEFAULTS, **params)
    pairs = np.ascontiguousarray(np.array(list(p["pairs"]), dtype=np.int64).reshape(-1, 2))
    if pairs.size and (pairs.min() < 0 or pairs.max() > 0xFFFFFFFF):
        raise ValueError("qc: pairs are (a, b) channel indices")
    flat = np.ascontiguousarray(pairs.astype(np.uint32).reshape(-1)) if pairs.size else np.zeros(2, dtype=np.uint32)
    for key, top in (("clip_run", 0xFFFFFFFF), ("dropout_frames", 0xFFFFFFFF), ("bucket", 0xFFFFFFFF), ("skip", 2 ** 64 - 1), ("limit", 2 ** 64 - 1)):
        if not 0 <= int(p[key]) <= top:
            raise ValueError(f"qc: {key} {p[key]} is no unsigned integer")
    spec = _QcSpec()
    spec.silence_level, spec.clip_level = float(p["silence_level"]), float(p["clip_level"])
    spec.clip_run, spec.dropout_frames, spec.bucket = int(p["clip_run"]), int(p["dropout_frames"]), int(p["bucket"])
    spec.num_pairs = int(pairs.shape[0])
    spec.pairs = flat.ctypes.data_as(C.POINTER(C.c_uint32))
    spec.skip, spec.limit = int(p["skip"]), int(p["limit"])
    return spec, [flat]


def _qc_signed(v: int) -> int:
    return -1 if v == 0xFFFFFFFFFFFFFFFF else int(v)


def _qc_channels(recs, pair_list, pair_sums) -> Dict[str, Any]:
    """The records of a read as arrays: one entry per channel under every key; "none" positions are -1."""
    import numpy as np
    n = len(recs)
    u = lambda f: np.array([f(r) for r in recs], dtype=np.int64).reshape(n)
    runs = lambda name: {k: u(lambda r, k=k: _qc_signed(getattr(getattr(r, name), k)) if k.endswith("_at") else int(getattr(getattr(r, name), k)))
                         for k in ("count", "longest", "longest_at", "first_at")}
    out = {k: u(lambda r, k=k: int(getattr(r, k))) for k in ("frames", "nonfinite", "quiet_frames", "clipped_frames", "head_silence", "tail_silence")}
    out["peak_at"] = u(lambda r: _qc_signed(r.peak_at))
    out["min"] = np.array([r.min for r in recs], dtype=np.float32)
    out["max"] = np.array([r.max for r in recs], dtype=np.float32)
    out["sum"] = np.array([r.sum for r in recs], dtype=np.float64)
    out["sum_sq"] = np.array([r.sum_sq for r in recs], dtype=np.float64)
    out["dropouts"], out["clip_events"] = runs("dropouts"), runs("clip_events")
    out["open_bucket"] = {"min": np.array([r.bucket_min for r in recs], dtype=np.float32), "max": np.array([r.bucket_max for r in recs], dtype=np.float32),
                          "frames": u(lambda r: int(r.bucket_frames))}
    out["pairs"] = [tuple(int(v) for v in ab) for ab in pair_list]
    out["sum_xy"] = np.array(pair_sums, dtype=np.float64).reshape(len(out["pairs"]))
    out["channels"] = n
    return out


def qc_launches() -> int:
    """``elemhip_qc_launches``: inspector kernels this process has launched so far (an engine whose inspector is off adds none)."""
    return int(load_library().elemhip_qc_launches())


def qc_host(x, state=None, **params):
    """``elemhip_qc_host``: the scalar twin of the inspector's kernels, pure host arithmetic — ``x`` float32 ``[channels, frames]`` behind
    the programme ``state`` describes (None: a programme's start) -> ``(read, state)``: ``read`` as ``Runtime.qc_read`` returns it (with
    ``overview`` float32 ``[channels, buckets, 2]``, every complete bucket of the programme so far), and the state to hand on. ``skip``
    and ``limit`` are applied here as the engine applies them."""
    import numpy as np
    lib = load_library()
    a = np.ascontiguousarray(x, dtype=np.float32)
    if a.ndim == 1:
        a = a[None, :]
    ch = a.shape[0]
    spec, keep = _qc_spec(params)
    npairs, bucket = int(spec.num_pairs), int(spec.bucket)
    if state is None:
        state = {"bytes": np.zeros(max(int(lib.elemhip_qc_state_bytes(ch, npairs)), 1), dtype=np.uint8), "frames": 0, "delivered": 0,
                 "overview": np.zeros((ch, 0, 2), dtype=np.float32)}
    else:
        state = {"bytes": np.array(state["bytes"], dtype=np.uint8), "frames": int(state["frames"]), "delivered": int(state["delivered"]),
                 "overview": state["overview"]}
    skip, limit, p0 = int(spec.skip), int(spec.limit), state["frames"]
    lead = min(max(skip - state["delivered"], 0), a.shape[1])
    take = a.shape[1] - lead
    if limit:
        take = min(take, max(limit - p0, 0))
    part = np.ascontiguousarray(a[:, lead:lead + take])
    buckets = ((p0 + take) // bucket - p0 // bucket) if bucket else 0
    recs = (_QcChannel * max(ch, 1))()
    sums = np.zeros(max(npairs, 1), dtype=np.float64)
    ov = np.zeros((ch, buckets, 2), dtype=np.float32)
    ovbuf = np.zeros(max(ov.size, 1), dtype=np.float32)
    rc = lib.elemhip_qc_host(C.byref(spec), part.ctypes.data_as(C.POINTER(C.c_float)) if take else None, ch, max(take, 1), take, p0,
                             state["bytes"].ctypes.data_as(C.POINTER(C.c_uint8)), recs, sums.ctypes.data_as(C.POINTER(C.c_double)),
                             ovbuf.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != 0:
        err = ElemHipError(f"elemhip_qc_host failed: {describe(rc)} (code {rc})")
        err.code = rc
        raise err
    ov[...] = ovbuf[:ov.size].reshape(ov.shape)
    pair_list = np.ctypeslib.as_array(spec.pairs, shape=(2 * max(npairs, 1),))[:2 * npairs].reshape(-1, 2).copy()
    del keep
    state["frames"], state["delivered"] = p0 + take, state["delivered"] + a.shape[1]
    state["overview"] = np.concatenate([state["overview"], ov], axis=1)
    read = _qc_channels([recs[c] for c in range(ch)], pair_list, sums[:npairs])
    read["overview"], read["bucket"], read["delivered"] = state["overview"], bucket, state["delivered"]
    return read, state


class FlacMd5:
    """The host twin of the MD5 FLAC delivery computes on the GPU (option ``flac_md5``; ``elemhip_flac_md5_init`` / ``_update`` /
    ``_final``): the digest of one stream's codes as STREAMINFO wants it — for every frame, then channel, the low ``bits / 8`` bytes of
    the code, little-endian. ``update(codes[G, n], bits)`` may be called piece by piece; ``digest()`` leaves the record as it is."""

    def __init__(self):
        import numpy as np
        self._lib = load_library()
        self.record = np.zeros(int(self._lib.elemhip_flac_md5_record_bytes()), dtype=np.uint8)
        self._check(self._lib.elemhip_flac_md5_init(self._p()), "init")

    def _p(self):
        return self.record.ctypes.data_as(C.POINTER(C.c_uint8))

    @staticmethod
    def _check(rc, what):
        if rc != 0:
            err = ElemHipError(f"elemhip_flac_md5_{what} failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err

    def update(self, codes, bits: int = 16) -> "FlacMd5":
        import numpy as np
        a = np.ascontiguousarray(codes, dtype=np.int32)
        if a.ndim == 1:
            a = a[None, :]
        ch, n = int(a.shape[0]), int(a.shape[1])
        rows = (C.POINTER(C.c_int32) * max(1, ch))(*[a[c].ctypes.data_as(C.POINTER(C.c_int32)) for c in range(ch)])
        self._check(self._lib.elemhip_flac_md5_update(self._p(), rows, ch, n, int(bits)), "update")
        return self

    def digest(self) -> bytes:
        import numpy as np
        out = np.zeros(16, dtype=np.uint8)
        self._check(self._lib.elemhip_flac_md5_final(self._p(), out.ctypes.data_as(C.POINTER(C.c_uint8))), "final")
        return out.tobytes()


class FlacInMd5(FlacMd5):
    """The host twin of the MD5 the GPU computes over FLAC inputs and resources (option ``flac_in_md5``;
    ``elemhip_flac_in_md5_update``): the digest STREAMINFO announces — for every stream sample, then channel, the low
    ``(bits + 7) // 8`` bytes of the code, little-endian. ``update(codes[G, n], bits)`` takes 8 / 12 / 16 / 20 / 24 bits and 1 .. 8
    channels, piece by piece; ``digest()`` leaves the record as it is."""

    def update(self, codes, bits: int = 16) -> "FlacInMd5":
        import numpy as np
        a = np.ascontiguousarray(codes, dtype=np.int32)
        if a.ndim == 1:
            a = a[None, :]
        ch, n = int(a.shape[0]), int(a.shape[1])
        rows = (C.POINTER(C.c_int32) * max(1, ch))(*[a[c].ctypes.data_as(C.POINTER(C.c_int32)) for c in range(ch)])
        self._check(self._lib.elemhip_flac_in_md5_update(self._p(), rows, ch, n, int(bits)), "update")
        return self


class FlacMd5Mismatch(ElemHipError):
    """A FLAC input or resource whose decoded samples do not have the MD5 its STREAMINFO announces (``verify_input=True`` /
    ``verify=True``): ``.stream`` (the input's index, or the resource's name), ``.expected`` (the file's 16 bytes), ``.computed`` (the
    GPU's) and ``.output`` (the files the render wrote before the mismatch was known — closed and left in place; None where nothing was
    written)."""

    def __init__(self, stream, expected: bytes, computed: bytes, output=None):
        self.stream, self.expected, self.computed, self.output = stream, bytes(expected), bytes(computed), output
        where = f"; the output was written and is left in place: {output}" if output else ""
        super().__init__(f"FLAC input {stream!r}: the decoded samples' MD5 {self.computed.hex()} is not the {self.expected.hex()} STREAMINFO announces{where}")


def flac_md5_verdict(state: int, computed: bytes, expected: bytes) -> str:
    """What a slot (``Runtime.flac_in_md5``) or a resource (``Runtime.shared_resource_md5``) says about a file that announces
    ``expected``: 'absent' (sixteen zeros: "not computed"), 'incomplete' (the stream was not hashed from sample 0 to its end), 'ok' or
    'mismatch'."""
    if bytes(expected) == bytes(16):
        return "absent"
    if int(state) != 2:
        return "incomplete"
    return "ok" if bytes(computed) == bytes(expected) else "mismatch"


class _FlacIn(C.Structure):
    _fields_ = [("data", C.c_void_p), ("bytes", C.c_uint64), ("frame_offsets", C.c_void_p), ("frame_first_samples", C.c_void_p),
                ("frames", C.c_uint64), ("channels", C.c_uint32), ("bits", C.c_uint32), ("total_samples", C.c_uint64), ("position", C.c_uint64)]


class _ResourceSrc(C.Structure):
    _fields_ = [("format", C.c_uint32), ("channels", C.c_uint32), ("sample_rate", C.c_double), ("frames", C.c_uint64), ("data", C.c_void_p),
                ("bytes", C.c_uint64), ("flac", C.POINTER(_FlacIn))]


FLAC_IN_REASONS = {1: "bad CRC", 2: "reserved value", 3: "bits missing", 4: "non-zero padding", 5: "sample out of range", 6: "unsupported"}


class FlacChunk:
    """A FLAC input (``in_fmt='flac'``): the frames that cover stream samples ``[position, position + count)`` — ``data`` (uint8, the
    frames' bytes), ``offsets`` / ``first_samples`` (uint64, ``frames + 1`` entries: byte offsets into ``data``, stream samples) — of a
    stream of ``channels`` channels and ``bits`` bits that holds ``total_samples`` samples. What ``FlacReader.read`` returns."""

    def __init__(self, data, offsets, first_samples, channels: int, bits: int, total_samples: int, position: int, count: int):
        import numpy as np
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.first_samples = np.ascontiguousarray(first_samples, dtype=np.uint64)
        if len(self.offsets) != len(self.first_samples) or len(self.offsets) < 1:
            raise ValueError("a FLAC table holds frames + 1 entries of offset and first sample")
        self.channels, self.bits, self.total_samples, self.position, self.count = int(channels), int(bits), int(total_samples), int(position), int(count)
        self.md5 = None         # the MD5 the stream's STREAMINFO announces, where the chunk comes from a file (FlacReader.read)

    @property
    def frames(self) -> int:
        return len(self.offsets) - 1

    def at(self, offset: int, count: int) -> "FlacChunk":
        """The same frames read from ``position + offset`` on for ``count`` samples (the engine looks the covering frames up itself)."""
        c = FlacChunk(self.data, self.offsets, self.first_samples, self.channels, self.bits, self.total_samples, self.position + int(offset), count)
        c.md5 = self.md5
        return c

    def struct(self) -> "_FlacIn":
        return _FlacIn(self.data.ctypes.data, self.data.size, self.offsets.ctypes.data, self.first_samples.ctypes.data, self.frames,
                       self.channels, self.bits, self.total_samples, self.position)


def _need_chunks(chunks, call: str) -> None:
    """Input format 4 points the engine at ``elemhip_flac_in`` structs: anything but a ``FlacChunk`` is refused here, with the code the
    engine gives a malformed one."""
    if any(not isinstance(c, FlacChunk) for c in chunks):
        err = ElemHipError(f"{call} failed: {describe(8)} (code 8): a FLAC input stream is a FlacChunk")
        err.code = 8
        raise err


def _flac_in_pointers(chunks):
    """The ``elemhip_flac_in`` structs of a call's chunks and the pointer array over them (both have to outlive the call)."""
    structs = (_FlacIn * max(1, len(chunks)))(*[c.struct() for c in chunks])
    ptrs = (C.c_void_p * max(1, len(chunks)))(*[C.addressof(structs[i]) for i in range(len(chunks))])
    return structs, ptrs


def flac_index(data, channels: int, bits: int, block_size: int = 0):
    """``elemhip_flac_index``: a stream's frame bytes (behind its metadata) -> ``(offsets, first_samples)``, uint64 arrays of
    ``frames + 1`` entries (the closing entry: ``len(data)`` and the samples in all)."""
    import numpy as np
    lib = load_library()
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    cap = 0
    while True:
        off, first = np.zeros(max(cap, 1), dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.uint64)
        need = C.c_size_t(0)
        rc = lib.elemhip_flac_index(a.ctypes.data_as(C.POINTER(C.c_uint8)), a.size, int(channels), int(bits), int(block_size),
                                    off.ctypes.data_as(C.POINTER(C.c_uint64)), first.ctypes.data_as(C.POINTER(C.c_uint64)), cap, C.byref(need))
        if rc != 0:
            err = ElemHipError(f"elemhip_flac_index failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err
        if need.value <= cap:
            return off[:need.value].copy(), first[:need.value].copy()
        cap = need.value


def flac_decode(chunk: "FlacChunk", count: Optional[int] = None):
    """``elemhip_flac_decode``: the scalar twin of the decode kernels — the chunk's samples ``[position, position + count)`` as int32
    ``[channels, count]`` (zeros past the stream's end). A frame that does not decode raises with ``.code`` 106, ``.frame``, ``.reason``."""
    import numpy as np
    lib = load_library()
    n = chunk.count if count is None else int(count)
    out = np.zeros((chunk.channels, max(n, 1)), dtype=np.int32)
    rows = (C.POINTER(C.c_int32) * max(1, chunk.channels))(*[out[c].ctypes.data_as(C.POINTER(C.c_int32)) for c in range(chunk.channels)])
    st = chunk.struct()
    bad, reason = C.c_size_t(0), C.c_uint32(0)
    rc = lib.elemhip_flac_decode(C.byref(st), n, rows, C.byref(bad), C.byref(reason))
    if rc != 0:
        err = ElemHipError(f"elemhip_flac_decode failed: {describe(rc)} (code {rc}; frame {bad.value}: {FLAC_IN_REASONS.get(reason.value, reason.value)})")
        err.code, err.frame, err.reason = rc, bad.value, reason.value
        raise err
    return out[:, :n]


class _LoudnessResult(C.Structure):
    _fields_ = [("integrated", C.c_double), ("momentary_max", C.c_double), ("short_term_max", C.c_double),
                ("blocks", C.c_uint64), ("gated_blocks", C.c_uint64)]


PCM_FORMATS = {"s16": 1, "s24": 2, "f32": 3, "flac": 4}


def pcm_format(fmt) -> int:
    """'s16' / 's24' / 'f32' (or the C-ABI's 1 / 2 / 3; as an input also 'flac', 4) -> the C-ABI's format number; anything else is handed on for the engine to refuse."""
    return PCM_FORMATS.get(fmt.lower(), 0) if isinstance(fmt, str) else int(fmt)


class _Stats(C.Structure):
    _fields_ = [
        ("blocks_rendered", C.c_uint64), ("plans_built", C.c_uint64), ("last_plan_build_ms", C.c_double),
        ("num_islands", C.c_uint32), ("num_levels", C.c_uint32), ("num_tasks", C.c_uint32),
        ("num_nodes_in_plan", C.c_uint32), ("max_lds_bytes", C.c_uint32), ("num_hbm_buffers", C.c_uint32),
        ("graph_replays", C.c_uint64), ("graph_captures", C.c_uint64), ("batch_launches", C.c_uint64),
        ("spec_launches", C.c_uint64), ("spec_shapes", C.c_uint32), ("spec_islands", C.c_uint32), ("last_jit_wait_ms", C.c_double), ("last_graph_capture_ms", C.c_double),
        ("resident_launches", C.c_uint64), ("resident_blocks", C.c_uint64),
        ("fft_launches", C.c_uint64), ("fft_frames", C.c_uint64),
    ]


def describe(code: int) -> str:
    try:
        return load_library().elemhip_describe(int(code)).decode()
    except ElemHipError:
        return RETURN_CODES.get(code, "Return code not recognized")


class Runtime(CRuntime):
    """``elem::Runtime<float>`` on one MI355X (``device`` = HIP ordinal; -1 = dry host-logic handle)."""

    def __init__(self, sample_rate: float, block_size: int, device: int = 0):
        lib = load_library()
        h = lib.elemhip_create(float(sample_rate), int(block_size), int(device))
        if not h:
            code = lib.elemhip_last_create_error()
            raise ElemHipError(f"elemhip_create failed: {describe(code)} (code {code})")
        super().__init__(lib, "elemhip_", C.c_void_p(h), sample_rate, block_size)
        self.device = int(device)

    # -- shared resources from a file's bytes (resource_load.h) ------------------------------
    def add_shared_resource_pcm(self, name: str, data, fmt=None, channels: Optional[int] = None, sample_rate: Optional[float] = None) -> bool:
        """``elemhip_add_shared_resource_pcm``: a shared resource from interleaved samples as a file holds them, decoded on the GPU —
        ``data`` int16 ``[frames, channels]`` ('s16'), uint8 ``[frames, channels, 3]`` ('s24'), float32 ``[frames, channels]`` ('f32')
        or raw bytes of ``fmt`` with ``channels`` given; or a ``FlacChunk`` (``FlacReader.read``), whose frames are decoded there too.
        ``sample_rate`` other than the engine's (None: the engine's): the resource is converted with the centred filter and holds
        ``ceil(frames * L / M)`` frames. Returns False where the name is taken; raises ``ElemHipError`` with ``.code`` otherwise
        (8 a malformed source, 6 no plan for the rate pair or too many frames, 106 a FLAC frame that does not decode)."""
        import numpy as np
        src = _ResourceSrc()
        src.sample_rate = 0.0 if sample_rate is None else float(sample_rate)
        if isinstance(data, FlacChunk):
            st = data.struct()
            src.format, src.channels, src.frames, src.flac = 4, data.channels, data.count, C.pointer(st)
        else:
            code = pcm_format(fmt) if fmt is not None else 0
            if isinstance(data, (bytes, bytearray, memoryview)):
                a = np.frombuffer(data, dtype=np.uint8)
            else:
                a = np.ascontiguousarray(data)
                if channels is None and a.ndim >= 2:
                    channels = a.shape[1]
                if fmt is None:
                    code = {np.dtype(np.int16): 1, np.dtype(np.uint8): 2, np.dtype(np.float32): 3}.get(a.dtype, 0)
                a = a.reshape(-1).view(np.uint8)
            G = int(channels) if channels is not None else 1
            width = {1: 2, 2: 3, 3: 4}.get(code, 1) * max(G, 1)
            src.format, src.channels, src.frames, src.data, src.bytes = code, G, a.size // width, a.ctypes.data, a.size
        done = C.c_int(0)
        rc = self._lib.elemhip_add_shared_resource_pcm(self._h, name.encode(), C.byref(src), C.byref(done))
        if rc != 0:
            err = ElemHipError(f"elemhip_add_shared_resource_pcm failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err
        return bool(done.value)

    def shared_resource_info(self, name: str) -> Dict[str, int]:
        """``elemhip_shared_resource_info``: ``{'channels', 'frames'}`` of any shared resource."""
        ch, fr = C.c_uint32(0), C.c_uint64(0)
        rc = self._lib.elemhip_shared_resource_info(self._h, name.encode(), C.byref(ch), C.byref(fr))
        if rc != 0:
            err = ElemHipError(f"elemhip_shared_resource_info failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err
        return {"channels": int(ch.value), "frames": int(fr.value)}

    def shared_resource_md5(self, name: str) -> Dict[str, Any]:
        """``elemhip_shared_resource_md5``: ``{'state', 'md5'}`` — what the load of a FLAC resource left under option ``flac_in_md5``:
        state 0 not hashed (the option was off, or the source was no FLAC), 1 incomplete (the load did not cover the stream from
        sample 0 to its end), 2 ``md5`` is the digest of the FILE's samples (also where the resource was rate-converted)."""
        import numpy as np
        st, out = C.c_uint32(0), np.zeros(16, dtype=np.uint8)
        rc = self._lib.elemhip_shared_resource_md5(self._h, name.encode(), out.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(st))
        if rc != 0:
            err = ElemHipError(f"elemhip_shared_resource_md5 failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err
        return {"state": int(st.value), "md5": out.tobytes()}

    def shared_resource_read(self, name: str, channel: Optional[int] = None, first: int = 0, count: Optional[int] = None):
        """``elemhip_shared_resource_read``: the floats the nodes see — one channel's frames ``[first, first + count)``, or with
        ``channel`` None all channels as ``[channels, count]``."""
        import numpy as np
        info = self.shared_resource_info(name)
        n = info["frames"] - int(first) if count is None else int(count)
        chans = range(info["channels"]) if channel is None else [int(channel)]
        out = np.zeros((len(chans), max(n, 0)), dtype=np.float32)
        for i, c in enumerate(chans):
            rc = self._lib.elemhip_shared_resource_read(self._h, name.encode(), c, int(first), max(n, 0) if n >= 0 else (1 << 63),
                                                        out[i].ctypes.data_as(C.POINTER(C.c_float)))
            if rc != 0:
                err = ElemHipError(f"elemhip_shared_resource_read failed: {describe(rc)} (code {rc})")
                err.code = rc
                raise err
        return out if channel is None else out[0]

    # -- offline / throughput path --------------------------------------------------------
    def process_blocks(self, num_blocks: int, num_outputs: int, out_ptr: int = 0, in_ptr: int = 0, num_inputs: int = 0,
                       sample_time: Optional[int] = None) -> None:
        """Render ``num_blocks`` full blocks with device-resident I/O (raw device pointers).

        ``out_ptr`` -> float32 [num_blocks][num_outputs][block_size] in HBM (0 = discard),
        ``in_ptr``  -> float32 [num_blocks][num_inputs][block_size] in HBM (0 when no inputs).
        """
        st = self.sample_time if sample_time is None else int(sample_time)
        rc = self._lib.elemhip_process_blocks(self._h, C.c_void_p(in_ptr or None), num_inputs,
                                              C.c_void_p(out_ptr or None), num_outputs, int(num_blocks), st)
        if rc != 0:
            raise ElemHipError(f"elemhip_process_blocks failed: {describe(rc)} (code {rc})")
        if sample_time is None:
            self.sample_time += int(num_blocks) * self.block_size

    def process_blocks_host(self, inputs, num_outputs: int, num_frames: Optional[int] = None, out=None,
                            sample_time: Optional[int] = None):
        """``elemhip_process_blocks_host``: the offline caller's whole block loop over HOST arrays.

        ``inputs``: float32 ``[num_inputs, num_frames]`` (or None); returns / fills ``out``: float32
        ``[num_outputs, num_frames]`` (C-contiguous rows). ``ceil(num_frames / block_size)`` full blocks are rendered. With option
        ``resample_rate`` on, ``num_frames`` stays the rendered count and the rows hold ``resample_frames(num_frames)`` frames. With
        option ``input_rate`` on, ``inputs`` holds ``input_resample_frames(num_frames)`` frames at that rate; without ``num_frames``
        the call renders as many frames as the inputs cover.
        """
        import numpy as np
        from ._cabi import _ptr_array
        rows = []
        if inputs is not None:
            a = np.ascontiguousarray(inputs, dtype=np.float32)
            if a.ndim == 1:
                a = a[None, :]
            rows = [a[i] for i in range(a.shape[0])]
            num_frames = self._frames_for_inputs(a.shape[1], num_frames)
        if num_frames is None:
            num_frames = out.shape[1]
        n_out = self.resample_frames(num_frames)
        if out is None:
            out = np.empty((num_outputs, n_out), dtype=np.float32)
        assert out.dtype == np.float32 and out.shape[0] == num_outputs and out.shape[1] >= n_out and out.strides[1] == 4
        st = self.sample_time if sample_time is None else int(sample_time)
        rc = self._lib.elemhip_process_blocks_host(self._h, _ptr_array(rows), len(rows),
                                                   _ptr_array([out[i] for i in range(num_outputs)]), num_outputs, int(num_frames), st)
        if rc != 0:
            err = ElemHipError(f"elemhip_process_blocks_host failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err
        if sample_time is None:
            nb = (int(num_frames) + self.block_size - 1) // self.block_size
            self.sample_time += nb * self.block_size
        return out

    def process_blocks_pcm(self, inputs, num_streams: int, channels_per_stream: int, num_frames: Optional[int] = None, fmt="s16",
                           dither_seed: Optional[int] = None, want_float: bool = False, sample_time: Optional[int] = None):
        """``elemhip_process_blocks_pcm``: the offline block loop delivered as interleaved PCM, packed on the GPU.

        The ``num_streams * channels_per_stream`` output channels come back as ``num_streams`` arrays — ``int16 [frames, G]`` for
        ``fmt`` 's16', ``uint8 [frames, G, 3]`` (little-endian) for 's24', ``float32 [frames, G]`` for 'f32'; sample ``(frame, g)`` of
        stream ``s`` is output channel ``s * G + g``. ``dither_seed``: None = no dither, else TPDF dither keyed on it and on the
        absolute frame time. Returns ``(streams, stats, planar)``: ``stats`` = ``{'peak': float32[nOut], 'over': uint64[nOut],
        'nonfinite': uint64[nOut]}`` over the delivered frames, ``planar`` = float32 ``[nOut, frames]`` (the very samples that were
        packed) when ``want_float``, else None.
        """
        import numpy as np
        from ._cabi import _ptr_array
        rows = []
        if inputs is not None:
            a = np.ascontiguousarray(inputs, dtype=np.float32)
            if a.ndim == 1:
                a = a[None, :]
            rows = [a[i] for i in range(a.shape[0])]
            num_frames = self._frames_for_inputs(a.shape[1], num_frames)
        if num_frames is None:
            raise ValueError("num_frames is needed without inputs")
        n, S, G, code = int(num_frames), int(num_streams), int(channels_per_stream), pcm_format(fmt)
        nd = self.resample_frames(n)          # frames delivered (option "resample_rate"; n while it is off)
        shape, dtype = {1: ((nd, G), np.int16), 2: ((nd, G, 3), np.uint8)}.get(code, ((nd, G), np.float32))
        streams = [np.zeros(shape, dtype=dtype) for _ in range(S)]
        planar = np.zeros((S * G, nd), dtype=np.float32) if want_float else None
        stats = (_PcmChannelStats * max(1, S * G))()
        spec = _PcmSpec(code, G, 0 if dither_seed is None else 1, 0 if dither_seed is None else int(dither_seed) & 0xFFFFFFFF)
        sp = (C.c_void_p * max(1, S))(*[C.c_void_p(a.ctypes.data) for a in streams])
        st = self.sample_time if sample_time is None else int(sample_time)
        rc = self._lib.elemhip_process_blocks_pcm(self._h, _ptr_array(rows), len(rows), sp, S,
                                                  _ptr_array([planar[i] for i in range(S * G)]) if want_float else None,
                                                  n, st, C.byref(spec), stats)
        if rc != 0:
            err = ElemHipError(f"elemhip_process_blocks_pcm failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err
        if sample_time is None:
            self.sample_time += ((n + self.block_size - 1) // self.block_size) * self.block_size
        out_stats = {"peak": np.array([stats[c].peak for c in range(S * G)], dtype=np.float32),
                     "over": np.array([stats[c].over for c in range(S * G)], dtype=np.uint64),
                     "nonfinite": np.array([stats[c].nonfinite for c in range(S * G)], dtype=np.uint64)}
        return streams, out_stats, planar

    def process_blocks_pcm_io(self, in_streams, in_fmt, num_outputs: Optional[int] = None, num_frames: Optional[int] = None, out_fmt=None,
                              num_streams: Optional[int] = None, channels_per_stream: Optional[int] = None, dither_seed: Optional[int] = None,
                              want_float: bool = False, sample_time: Optional[int] = None, in_channels_per_stream: Optional[int] = None):
        """``elemhip_process_blocks_pcm_io``: the offline block loop FED with interleaved PCM, unpacked on the GPU.

        ``in_streams``: a list of arrays in the layout ``process_blocks_pcm`` returns — ``int16 [frames, G]`` for ``in_fmt`` 's16',
        ``uint8 [frames, G, 3]`` (little-endian) for 's24', ``float32 [frames, G]`` for 'f32'; sample ``(frame, g)`` of stream ``s``
        is input channel ``s * G + g`` (``G`` is read off the arrays unless ``in_channels_per_stream`` says it). s16 samples are worth
        ``code * 2**-15``, s24 ``code * 2**-23``, f32 passes as bits. ``out_fmt`` None: returns float32 ``[num_outputs, frames]`` as
        ``process_blocks_host`` does; else ``(streams, stats, planar)`` as ``process_blocks_pcm`` does for ``num_streams`` streams of
        ``channels_per_stream`` channels in ``out_fmt``. ``in_fmt`` 'flac': ``in_streams`` is a list of ``FlacChunk`` objects, one per
        stream — FLAC frames, decoded on the GPU into the s16 / s24 stream of the same samples; a frame that does not decode raises
        with ``.code`` 106 (``flac_in_error()`` names it).
        """
        import numpy as np
        from ._cabi import _ptr_array
        in_code = pcm_format(in_fmt)
        want = {1: (np.int16, 2), 2: (np.uint8, 3), 3: (np.float32, 2)}.get(in_code)
        ins = []
        chunks = list(in_streams or []) if in_code == 4 else []      # FLAC: FlacChunk objects, decoded on the GPU
        _need_chunks(chunks, "elemhip_process_blocks_pcm_io")
        if chunks and num_frames is None:
            num_frames = chunks[0].count
        for a in ([] if in_code == 4 else (in_streams or [])):
            a = np.ascontiguousarray(a)
            if want is not None and (a.dtype != want[0] or a.ndim != want[1] or (in_code == 2 and a.shape[2] != 3)):
                raise ValueError(f"a {in_fmt} input stream is {np.dtype(want[0]).name} [frames, G{', 3' if in_code == 2 else ''}], got {a.dtype} {a.shape}")
            if a.dtype.byteorder == ">":
                a = a.byteswap().newbyteorder()
            ins.append(a)
        if ins and (any(a.shape[0] != ins[0].shape[0] for a in ins) or any(a.ndim > 1 and a.shape[1] != ins[0].shape[1] for a in ins)):
            raise ValueError("the input streams differ in frames or in channels per stream")
        in_g = int(in_channels_per_stream) if in_channels_per_stream is not None else (int(ins[0].shape[1]) if ins and ins[0].ndim > 1 else 1)
        if num_frames is None:
            if not ins:
                raise ValueError("num_frames is needed without inputs")
            num_frames = self._frames_for_inputs(ins[0].shape[0], None)
        n = int(num_frames)
        need = self.input_resample_frames(n) if ins else n      # input frames consumed (option "input_rate"; n while it is off)
        if ins and want is not None and in_channels_per_stream is None and ins[0].shape[0] < need:
            raise ValueError(f"the input streams hold {ins[0].shape[0]} frames, {need} are asked for")
        ip = (C.c_void_p * max(1, len(ins)))(*[C.c_void_p(a.ctypes.data) for a in ins])
        if chunks:
            keep, ip = _flac_in_pointers(chunks)
            ins, in_g = chunks, (int(in_channels_per_stream) if in_channels_per_stream is not None else chunks[0].channels)
        in_spec = _PcmInSpec(in_code, in_g)
        st = self.sample_time if sample_time is None else int(sample_time)
        nd = self.resample_frames(n)          # frames delivered (option "resample_rate"; n while it is off)
        if out_fmt is None:
            if num_outputs is None:
                raise ValueError("num_outputs is needed for planar float output")
            # (a FLAC-fed call can end after some launch sets, code 106: what it did not deliver is then zeros, not stale memory)
            out = (np.zeros if chunks else np.empty)((int(num_outputs), nd), dtype=np.float32)
            rc = self._lib.elemhip_process_blocks_pcm_io(self._h, ip, len(ins), C.byref(in_spec), None, 0, None,
                                                         _ptr_array([out[i] for i in range(int(num_outputs))]), int(num_outputs), n, st, None)
            result = out
        else:
            S, G, code = int(num_streams), int(channels_per_stream), pcm_format(out_fmt)
            shape, dtype = {1: ((nd, G), np.int16), 2: ((nd, G, 3), np.uint8)}.get(code, ((nd, G), np.float32))
            streams = [np.zeros(shape, dtype=dtype) for _ in range(S)]
            planar = np.zeros((S * G, nd), dtype=np.float32) if want_float else None
            stats = (_PcmChannelStats * max(1, S * G))()
            spec = _PcmSpec(code, G, 0 if dither_seed is None else 1, 0 if dither_seed is None else int(dither_seed) & 0xFFFFFFFF)
            sp = (C.c_void_p * max(1, S))(*[C.c_void_p(a.ctypes.data) for a in streams])
            rc = self._lib.elemhip_process_blocks_pcm_io(self._h, ip, len(ins), C.byref(in_spec), sp, S, C.byref(spec),
                                                         _ptr_array([planar[i] for i in range(S * G)]) if want_float else None, S * G if want_float else 0,
                                                         n, st, stats)
            result = (streams, {"peak": np.array([stats[c].peak for c in range(S * G)], dtype=np.float32),
                                "over": np.array([stats[c].over for c in range(S * G)], dtype=np.uint64),
                                "nonfinite": np.array([stats[c].nonfinite for c in range(S * G)], dtype=np.uint64)}, planar)
        if rc != 0:
            err = ElemHipError(f"elemhip_process_blocks_pcm_io failed: {describe(rc)} (code {rc})")
            err.code = rc
            err.result = result       # (after 106: the whole launch sets in front of the failing one, zeros behind them)
            raise err
        if sample_time is None:
            self.sample_time += ((n + self.block_size - 1) // self.block_size) * self.block_size
        return result

    def process_blocks_flac(self, inputs, num_streams: int, channels_per_stream: int, num_frames: Optional[int] = None, bits: Optional[int] = None,
                            dither_seed: Optional[int] = None, sample_time: Optional[int] = None, drop: int = 0, take: Optional[int] = None,
                            in_fmt=None):
        """``elemhip_process_blocks_flac``: the offline block loop delivered as FLAC frames, encoded on the GPU.

        The ``num_streams * channels_per_stream`` output channels (laid out as in ``process_blocks_pcm``) come back as one ``bytes``
        per stream: the whole FLAC frames this call completed in the programme (``flac_reset`` .. ``flac_flush``), possibly empty —
        the open frame's samples stay on the device for the next call. Decoded, the samples are the s16 / s24 codes
        ``process_blocks_pcm`` delivers for the same render, ``dither_seed`` and ``sample_time``. ``bits``: 16 or 24 (None: option
        ``flac_bits``); the block size is option ``flac_frame``. ``inputs``: float32 ``[num_inputs, frames]`` (or None), or — with
        ``in_fmt`` — a list of PCM stream arrays as ``process_blocks_pcm_io`` takes them. ``drop`` / ``take``: of the frames this call
        delivers, the first ``drop`` stay out of the programme and at most ``take`` enter it (a file that leaves a converter's or the
        limiter's latency out: frames cannot be cut on the host). Returns ``(streams, stats)``, ``stats`` over the frames that entered."""
        import numpy as np
        ins, in_code, in_g = [], 3, 1
        if inputs is not None and in_fmt is None:
            a = np.ascontiguousarray(inputs, dtype=np.float32)
            if a.ndim == 1:
                a = a[None, :]
            ins = [a[i] for i in range(a.shape[0])]
            num_frames = self._frames_for_inputs(a.shape[1], num_frames)
        elif inputs is not None:
            in_code = pcm_format(in_fmt)
            if in_code == 4:
                ins = list(inputs)
                _need_chunks(ins, "elemhip_process_blocks_flac")
                in_g = ins[0].channels if ins else 1
                if num_frames is None and ins:
                    num_frames = ins[0].count
            else:
                ins = [np.ascontiguousarray(a) for a in inputs]
                in_g = int(ins[0].shape[1]) if ins and ins[0].ndim > 1 else 1
                if num_frames is None and ins:
                    num_frames = self._frames_for_inputs(ins[0].shape[0], None)
        if num_frames is None:
            raise ValueError("num_frames is needed without inputs")
        n, S, G = int(num_frames), int(num_streams), int(channels_per_stream)
        b = int(bits) if bits is not None else 0
        nd = self.resample_frames(n)
        cap = int(self._lib.elemhip_flac_bound(nd, max(G, 1), b if b in (16, 24) else 24))
        bufs = [np.empty(cap, dtype=np.uint8) for _ in range(S)]
        sp = (C.c_void_p * max(1, S))(*[C.c_void_p(a.ctypes.data) for a in bufs])
        caps = (C.c_size_t * max(1, S))(*([cap] * S))
        got = (C.c_size_t * max(1, S))()
        if in_code == 4 and in_fmt is not None:
            keep, ip = _flac_in_pointers(ins)
        else:
            ip = (C.c_void_p * max(1, len(ins)))(*[C.c_void_p(a.ctypes.data) for a in ins])
        in_spec = _PcmInSpec(in_code, in_g)
        stats = (_PcmChannelStats * max(1, S * G))()
        spec = _FlacSpec(b, G, 0 if dither_seed is None else 1, 0 if dither_seed is None else int(dither_seed) & 0xFFFFFFFF,
                         int(drop), 0xFFFFFFFFFFFFFFFF if take is None else int(take))
        st = self.sample_time if sample_time is None else int(sample_time)
        rc = self._lib.elemhip_process_blocks_flac(self._h, ip, len(ins), C.byref(in_spec), sp, caps, got, S, C.byref(spec), n, st, stats)
        if rc != 0:
            err = ElemHipError(f"elemhip_process_blocks_flac failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err
        if sample_time is None:
            self.sample_time += ((n + self.block_size - 1) // self.block_size) * self.block_size
        out_stats = {"peak": np.array([stats[c].peak for c in range(S * G)], dtype=np.float32),
                     "over": np.array([stats[c].over for c in range(S * G)], dtype=np.uint64),
                     "nonfinite": np.array([stats[c].nonfinite for c in range(S * G)], dtype=np.uint64)}
        return [bufs[s][:got[s]].tobytes() for s in range(S)], out_stats

    def flac_in_error(self) -> Dict[str, Any]:
        """``elemhip_flac_in_error``: ``{'stream', 'frame', 'reason', 'text'}`` of the last call that answered 106 — the first FLAC
        input frame that did not decode (``frame``: its index in the stream's table as the call was given it)."""
        s, f, r = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
        rc = self._lib.elemhip_flac_in_error(self._h, C.byref(s), C.byref(f), C.byref(r))
        if rc != 0:
            err = ElemHipError(f"elemhip_flac_in_error failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err
        return {"stream": s.value, "frame": f.value, "reason": r.value, "text": FLAC_IN_REASONS.get(r.value, str(r.value))}

    def flac_in_md5(self) -> Dict[str, Any]:
        """``elemhip_flac_in_md5`` (option ``flac_in_md5``): ``{'state': [...], 'md5': [bytes, ...], 'hashed': [...]}``, one entry per
        slot — input stream ``s`` of a call is slot ``s``. state 0 off or never fed, 1 running, 2 complete (``md5`` holds the 16 bytes
        STREAMINFO should announce), 3 broken until ``flac_in_md5_reset`` (a gap, a frame that did not decode, another stream under a
        running slot); ``md5`` is all zero unless the state is 2; ``hashed``: stream samples in the digest. Waits for what is in flight."""
        import numpy as np
        n = C.c_size_t(0)
        rc = self._lib.elemhip_flac_in_md5(self._h, None, None, None, 0, C.byref(n))
        S = int(n.value)
        dig, st, hs = np.zeros((max(S, 1), 16), dtype=np.uint8), np.zeros(max(S, 1), dtype=np.uint32), np.zeros(max(S, 1), dtype=np.uint64)
        if rc == 0 and S:
            rc = self._lib.elemhip_flac_in_md5(self._h, dig.ctypes.data_as(C.POINTER(C.c_uint8)), st.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               hs.ctypes.data_as(C.POINTER(C.c_uint64)), S, C.byref(n))
        if rc != 0:
            err = ElemHipError(f"elemhip_flac_in_md5 failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err
        return {"state": [int(v) for v in st[:S]], "md5": [dig[s].tobytes() for s in range(S)], "hashed": [int(v) for v in hs[:S]]}

    def flac_in_md5_reset(self) -> None:
        """``elemhip_flac_in_md5_reset``: every input slot back to state 0 (a new programme of inputs starts)."""
        rc = self._lib.elemhip_flac_in_md5_reset(self._h)
        if rc != 0:
            err = ElemHipError(f"elemhip_flac_in_md5_reset failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err

    def flac_read(self) -> Dict[str, Any]:
        """``elemhip_flac_read``: the FLAC programme so far — ``{'flac_frame', 'bits', 'channels_per_stream', 'streams', 'sample_rate',
        'flushed', 'frames', 'lpc_order', 'md5_state', 'stream_frames', 'total_samples', 'min_frame_bytes', 'max_frame_bytes',
        'frame_bytes', 'md5'}``: the last six one entry per stream (the STREAMINFO fields; ``frame_bytes`` a uint32 array of every
        frame's byte length); ``lpc_order`` (``elemhip_flac_lpc_order``) the programme's option ``flac_lpc_order``. ``md5_state``
        (``elemhip_flac_md5``, option ``flac_md5``): 0 — the option is off in the programme, or there is none; 1 — the digests are
        running on the GPU, ``md5`` all zero; 2 — final after ``flac_flush``: ``md5`` holds every stream's 16 bytes."""
        import numpy as np
        info = _FlacInfo()
        rc = self._lib.elemhip_flac_read(self._h, C.byref(info), None, 0, None, 0)
        S = int(info.streams)
        per = (_FlacStreamInfo * max(1, S))()
        table = np.zeros((max(1, S), 1), dtype=np.uint32)
        for _ in range(8):
            if rc != 0 or S == 0:
                break
            rc = self._lib.elemhip_flac_read(self._h, C.byref(info), per, S, None, 0)
            if rc != 0:
                break
            cap = max([int(per[s].frames) for s in range(S)] + [1])
            table = np.zeros((S, cap), dtype=np.uint32)
            rc = self._lib.elemhip_flac_read(self._h, C.byref(info), per, S, table.ctypes.data_as(C.POINTER(C.c_uint32)), cap)
            if rc != 6:
                break
            rc = 0          # (another thread rendered in between: size the table again)
        lpc = C.c_uint32(0)
        if rc == 0:
            rc = self._lib.elemhip_flac_lpc_order(self._h, C.byref(lpc))
        md5_state, digests = C.c_uint32(0), np.zeros((max(1, S), 16), dtype=np.uint8)
        if rc == 0:
            rc = self._lib.elemhip_flac_md5(self._h, digests.ctypes.data_as(C.POINTER(C.c_uint8)), S, C.byref(md5_state))
        if rc != 0:
            err = ElemHipError(f"elemhip_flac_read failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err
        return {"flac_frame": int(info.flac_frame), "lpc_order": int(lpc.value), "md5_state": int(md5_state.value),
                "md5": [digests[s].tobytes() for s in range(S)], "bits": int(info.bits), "channels_per_stream": int(info.channels_per_stream), "streams": S,
                "sample_rate": int(info.sample_rate), "flushed": bool(info.flushed), "frames": int(info.frames),
                "stream_frames": [int(per[s].frames) for s in range(S)], "total_samples": [int(per[s].total_samples) for s in range(S)],
                "min_frame_bytes": [int(per[s].min_frame_bytes) for s in range(S)], "max_frame_bytes": [int(per[s].max_frame_bytes) for s in range(S)],
                "frame_bytes": [table[s, :int(per[s].frames)].copy() for s in range(S)]}

    def flac_flush(self):
        """``elemhip_flac_flush``: the open remainder as one final short frame per stream (``b''`` where nothing is open); the programme
        is closed — further FLAC calls fail with code 6 until ``flac_reset``."""
        import numpy as np
        info = _FlacInfo()
        self._lib.elemhip_flac_read(self._h, C.byref(info), None, 0, None, 0)
        S, G, b = int(info.streams), max(1, int(info.channels_per_stream)), int(info.bits)
        cap = int(self._lib.elemhip_flac_bound(0, G, b if b in (16, 24) else 24))
        bufs = [np.empty(cap, dtype=np.uint8) for _ in range(S)]
        sp = (C.c_void_p * max(1, S))(*[C.c_void_p(a.ctypes.data) for a in bufs])
        caps = (C.c_size_t * max(1, S))(*([cap] * S))
        got = (C.c_size_t * max(1, S))()
        rc = self._lib.elemhip_flac_flush(self._h, sp, caps, got, S)
        if rc != 0:
            err = ElemHipError(f"elemhip_flac_flush failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err
        return [bufs[s][:got[s]].tobytes() for s in range(S)]

    def flac_reset(self) -> None:
        """``elemhip_flac_reset``: a new FLAC programme — nothing open, frame number 0."""
        rc = self._lib.elemhip_flac_reset(self._h)
        if rc != 0:
            err = ElemHipError(f"elemhip_flac_reset failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err

    def loudness_read(self) -> Dict[str, Any]:
        """``elemhip_loudness_read`` (option ``loudness_meter``): the programme metered so far — ``{'channels', 'sub_blocks', 'hop',
        'frames', 'mean_squares': float64 [channels, sub_blocks], 'true_peak': float64 [channels] (linear, the zero-padded tail
        included), 'sample_peak': float32 [channels]}``. A read does not disturb a programme that continues."""
        import numpy as np
        info = _LoudnessInfo()
        rc = self._lib.elemhip_loudness_read(self._h, C.byref(info), None, 0, None, None)
        ch = n = 0
        for _ in range(8):
            if rc != 0:
                break
            ch, n = int(info.channels), int(info.sub_blocks)
            ms = np.zeros((ch, n), dtype=np.float64)
            tp, sp = np.zeros(max(1, ch), dtype=np.float64), np.zeros(max(1, ch), dtype=np.float32)
            rc = self._lib.elemhip_loudness_read(self._h, C.byref(info), ms.ctypes.data_as(C.POINTER(C.c_double)), ms.size,
                                                 tp.ctypes.data_as(C.POINTER(C.c_double)), sp.ctypes.data_as(C.POINTER(C.c_float)))
            if rc != 6 or (int(info.channels), int(info.sub_blocks)) == (ch, n):
                break
            rc = 0          # (another thread rendered in between: the info is filled, size the buffers again)
        if rc != 0:
            err = ElemHipError(f"elemhip_loudness_read failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err
        return {"channels": ch, "sub_blocks": n, "hop": int(info.hop), "frames": int(info.frames), "mean_squares": ms,
                "true_peak": tp[:ch], "sample_peak": sp[:ch]}

    def loudness_reset(self) -> None:
        """``elemhip_loudness_reset``: a new programme (time 0, zero filter state, no peaks)."""
        rc = self._lib.elemhip_loudness_reset(self._h)
        if rc != 0:
            err = ElemHipError(f"elemhip_loudness_reset failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err

    def resample_frames(self, num_frames: int) -> int:
        """``elemhip_resample_frames``: the frames the next ``process_blocks_host`` / ``_pcm`` / ``_pcm_io`` call of ``num_frames``
        rendered frames delivers — ``num_frames`` itself while option ``resample_rate`` is off."""
        got = C.c_size_t(0)
        rc = self._lib.elemhip_resample_frames(self._h, int(num_frames), C.byref(got))
        if rc != 0:
            raise ElemHipError(f"elemhip_resample_frames failed: {describe(rc)} (code {rc})")
        return int(got.value)

    def resample_read(self) -> Dict[str, Any]:
        """``elemhip_resample_read`` (option ``resample_rate``): ``{'up', 'down', 'taps', 'latency_frames', 'frames_in',
        'frames_out'}`` — delivery rate / engine rate = up / down in lowest terms, taps per output, the filter's latency in OUTPUT
        frames, and the programme's clock: frames rendered and frames delivered since the option was set or the last reset."""
        info = _ResampleInfo()
        rc = self._lib.elemhip_resample_read(self._h, C.byref(info))
        if rc != 0:
            err = ElemHipError(f"elemhip_resample_read failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err
        return {k: int(getattr(info, k)) for k, _ in _ResampleInfo._fields_}

    def resample_reset(self) -> None:
        """``elemhip_resample_reset``: a new programme (time 0, silence in front of it)."""
        rc = self._lib.elemhip_resample_reset(self._h)
        if rc != 0:
            err = ElemHipError(f"elemhip_resample_reset failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err

    def input_resample_frames(self, num_frames: int) -> int:
        """``elemhip_input_resample_frames``: the input frames the next ``process_blocks_host`` / ``_pcm`` / ``_pcm_io`` call of
        ``num_frames`` engine frames consumes — ``num_frames`` itself while option ``input_rate`` is off."""
        got = C.c_size_t(0)
        rc = self._lib.elemhip_input_resample_frames(self._h, int(num_frames), C.byref(got))
        if rc != 0:
            raise ElemHipError(f"elemhip_input_resample_frames failed: {describe(rc)} (code {rc})")
        return int(got.value)

    def input_resample_read(self) -> Dict[str, Any]:
        """``elemhip_input_resample_read`` (option ``input_rate``): ``{'up', 'down', 'taps', 'latency_frames', 'frames_in',
        'frames_out'}`` — engine rate / input rate = up / down in lowest terms, taps per engine frame, the filter's latency in ENGINE
        frames, and the programme's clock: input frames consumed and engine frames rendered since the option was set or the last reset."""
        info = _ResampleInfo()
        rc = self._lib.elemhip_input_resample_read(self._h, C.byref(info))
        if rc != 0:
            err = ElemHipError(f"elemhip_input_resample_read failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err
        return {k: int(getattr(info, k)) for k, _ in _ResampleInfo._fields_}

    def input_resample_reset(self) -> None:
        """``elemhip_input_resample_reset``: a new input programme (time 0, silence in front of it)."""
        rc = self._lib.elemhip_input_resample_reset(self._h)
        if rc != 0:
            err = ElemHipError(f"elemhip_input_resample_reset failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err

    def _frames_for_inputs(self, have: int, num_frames: Optional[int]) -> int:
        """The engine frames a call with ``have`` input frames renders: ``num_frames`` where it is given (checked against the inputs
        while option ``input_rate`` is on), else the largest count whose need the inputs cover — ``have`` while the option is off."""
        have = int(have)
        if self._lib.elemhip_input_resample_read(self._h, None) != 0:      # off: as ever
            return have if num_frames is None else int(num_frames)
        if num_frames is not None:
            need = self.input_resample_frames(num_frames)
            if have < need:
                raise ValueError(f"the inputs hold {have} frames, {int(num_frames)} engine frames need {need}")
            return int(num_frames)
        lo, hi = 0, 1                       # need(lo) <= have < need(hi); need() grows with the count
        while self.input_resample_frames(hi) <= have:
            lo, hi = hi, hi * 2
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if self.input_resample_frames(mid) <= have else (lo, mid)
        return lo

    def limiter_read(self) -> Dict[str, Any]:
        """``elemhip_limiter_read`` (option ``limiter``): the plan — ``lookahead_frames`` D, ``latency_frames`` D + 6,
        ``release_frames``, ``link`` (channels per linked group; 0: all), ``groups`` (0 before the programme's first call) — the
        programme's ``frames`` and, per group, ``max_reduction`` (float64: the largest reduction behind a delivered gain, 0 .. 1) and
        ``limited_frames`` (uint64: frames delivered with a gain below 1)."""
        import numpy as np
        info = _LimiterInfo()
        rc = self._lib.elemhip_limiter_read(self._h, C.byref(info), None, None, 0)
        groups = int(info.groups)
        red, lim = np.zeros(groups, dtype=np.float64), np.zeros(groups, dtype=np.uint64)
        if rc == 0 and groups:
            rc = self._lib.elemhip_limiter_read(self._h, C.byref(info), red.ctypes.data_as(C.POINTER(C.c_double)), lim.ctypes.data_as(C.POINTER(C.c_uint64)), groups)
        if rc != 0:
            err = ElemHipError(f"elemhip_limiter_read failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err
        got = {k: int(getattr(info, k)) for k, _ in _LimiterInfo._fields_ if k != "reserved"}
        got["max_reduction"], got["limited_frames"] = red, lim
        return got

    def limiter_reset(self) -> None:
        """``elemhip_limiter_reset``: a new programme (frame 0, silence in front of it, statistics zero)."""
        rc = self._lib.elemhip_limiter_reset(self._h)
        if rc != 0:
            err = ElemHipError(f"elemhip_limiter_reset failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err

    def noise_shape(self, coeffs) -> None:
        """``elemhip_noise_shape_set``: the error-feedback coefficients c_1 .. c_K (1 .. 12 of them) of s16 / s24 / FLAC delivery, or
        None / an empty list to turn the shaping off (the default). Starts a new programme. A set the engine refuses (more than 12,
        a non-finite one, too large a sum) raises with ``.code`` 6 and changes nothing."""
        import numpy as np
        c = np.zeros(0, dtype=np.float32) if coeffs is None else np.ascontiguousarray(coeffs, dtype=np.float32).reshape(-1)
        rc = self._lib.elemhip_noise_shape_set(self._h, c.ctypes.data_as(C.POINTER(C.c_float)) if c.size else None, c.size)
        if rc != 0:
            err = ElemHipError(f"elemhip_noise_shape_set failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err

    def noise_shape_read(self) -> Dict[str, Any]:
        """``elemhip_noise_shape_read``: ``taps`` (0: off), ``coeffs_q`` (int32: the coefficients times 2048, rounded), the programme's
        ``channels`` (0 before its first call) and ``frames``, and ``saturated`` (uint64 per channel: the error clamps so far)."""
        import numpy as np
        info = _NoiseShapeInfo()
        rc = self._lib.elemhip_noise_shape_read(self._h, C.byref(info), None, None, 0)
        cq, sat = np.zeros(int(info.taps), dtype=np.int32), np.zeros(int(info.channels), dtype=np.uint64)
        if rc == 0 and info.taps:
            rc = self._lib.elemhip_noise_shape_read(self._h, C.byref(info), cq.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    sat.ctypes.data_as(C.POINTER(C.c_uint64)) if sat.size else None, max(cq.size, sat.size))
        if rc != 0:
            err = ElemHipError(f"elemhip_noise_shape_read failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err
        return {"taps": int(info.taps), "coeffs_q": cq, "channels": int(info.channels), "frames": int(info.frames), "saturated": sat}

    def noise_shape_reset(self) -> None:
        """``elemhip_noise_shape_reset``: a new programme (errors zero, counts zero)."""
        rc = self._lib.elemhip_noise_shape_reset(self._h)
        if rc != 0:
            err = ElemHipError(f"elemhip_noise_shape_reset failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err

    def _spectrum_check(self, what: str, rc: int) -> None:
        if rc != 0:
            err = ElemHipError(f"{what} failed: {describe(rc)} (code {rc})")
            err.code = rc
            raise err

    def spectrum(self, size: Optional[int], hop: Optional[int] = None, window="hann", bands=None, center: bool = False) -> None:
        """``elemhip_spectrum_set``: analyse what the host-buffer render calls deliver as STFT frames of ``size`` (256 .. 4096) every
        ``hop`` (1 .. size; default ``size / 4``) frames — power spectra (``size / 2 + 1`` columns), or with ``bands`` (rows of
        ``(first_bin, weights)``, at most 512; ``elementary_amd.spectrum.mel_bands``) band sums. ``window``: a name
        (``elementary_amd.spectrum.window``) or ``size`` float64 values. ``center``: frame j is centred on programme frame ``j * hop``.
        ``size`` None turns the analyser off (the default). Starts a new programme. A spec the engine refuses raises with ``.code`` 6
        and changes nothing."""
        if size is None:
            return self._spectrum_check("elemhip_spectrum_set", self._lib.elemhip_spectrum_set(self._h, None))
        spec, keep = _spectrum_spec(size, int(size) // 4 if hop is None else hop, window, bands, center)
        rc = self._lib.elemhip_spectrum_set(self._h, C.byref(spec))
        del keep
        self._spectrum_check("elemhip_spectrum_set", rc)

    def spectrum_read(self, sums: bool = True) -> Dict[str, Any]:
        """``elemhip_spectrum_read``: drains the frames emitted since the last read — ``frames`` float32 ``[channels, n, columns]``,
        ``first_frame`` (the programme index of ``frames[:, 0]``), ``sums`` float64 ``[channels, columns]`` (the running sums over every
        frame emitted so far), ``frames_total``, ``delivered`` (programme frames analysed), ``flushed``, and the spec (``size``, ``hop``,
        ``center``, ``bands``). The programme is not disturbed. Raises on an engine whose analyser is off."""
        import numpy as np
        info = _SpectrumInfo()
        self._spectrum_check("elemhip_spectrum_read", self._lib.elemhip_spectrum_read(self._h, C.byref(info), None, 0, None, 0))
        ch, n, cols = int(info.channels), int(info.queued), int(info.columns)
        frames = np.zeros((ch, n, cols), dtype=np.float32)
        acc = np.zeros((ch, cols), dtype=np.float64)
        buf = np.zeros(max(frames.size, 1), dtype=np.float32)
        rc = self._lib.elemhip_spectrum_read(self._h, C.byref(info), buf.ctypes.data_as(C.POINTER(C.c_float)), buf.size,
                                             acc.ctypes.data_as(C.POINTER(C.c_double)) if (sums and acc.size) else None, acc.size)
        self._spectrum_check("elemhip_spectrum_read", rc)
        frames[...] = buf[:frames.size].reshape(frames.shape)
        return {"frames": frames, "first_frame": int(info.first_frame), "sums": acc, "frames_total": int(info.frames),
                "delivered": int(info.delivered), "flushed": bool(info.flushed), "channels": ch, "columns": cols, "size": int(info.size),
                "hop": int(info.hop), "center": bool(info.center), "bands": int(info.bands)}

    def spectrum_flush(self) -> None:
        """``elemhip_spectrum_flush``: pads the programme with zeros, emits the frames that completes and ends it; the next analysed call
        starts a new programme (read first: a new programme drops what was not read)."""
        self._spectrum_check("elemhip_spectrum_flush", self._lib.elemhip_spectrum_flush(self._h))

    def spectrum_reset(self) -> None:
        """``elemhip_spectrum_reset``: a new programme; what was pending is dropped."""
        self._spectrum_check("elemhip_spectrum_reset", self._lib.elemhip_spectrum_reset(self._h))

    def qc(self, spec: Optional[Dict[str, Any]] = None, **params) -> None:
        """``elemhip_qc_set``: inspect what the host-buffer render calls deliver — ``silence_level`` (0), ``clip_level`` (1.0),
        ``clip_run`` (3), ``dropout_frames`` (64), ``bucket`` (0: no overview), ``pairs`` (``(a, b)`` channel pairs, at most 128),
        ``skip`` and ``limit`` (the programme's window in delivered frames; 0: unbounded), as a dict or as keywords. ``qc(None)``
        without keywords turns the inspector off (the default). Starts a new programme. A spec the engine refuses raises with
        ``.code`` 6 and changes nothing."""
        if spec is None and not params:
            return self._spectrum_check("elemhip_qc_set", self._lib.elemhip_qc_set(self._h, None))
        cs, keep = _qc_spec(dict(spec or {}, **params))
        rc = self._lib.elemhip_qc_set(self._h, C.byref(cs))
        if rc == 0:
            self._qc_pairs = keep[0][:2 * int(cs.num_pairs)].reshape(-1, 2).copy()
        del keep
        self._spectrum_check("elemhip_qc_set", rc)

    def qc_read(self, overview: bool = True) -> Dict[str, Any]:
        """``elemhip_qc_read`` (and ``elemhip_qc_overview``): the cumulative results so far, one array entry per channel — ``frames``,
        ``nonfinite``, ``quiet_frames``, ``clipped_frames``, ``min``, ``max``, ``peak_at``, ``head_silence``, ``tail_silence``, ``sum``,
        ``sum_sq``, ``dropouts`` and ``clip_events`` (dicts of ``count``, ``longest``, ``longest_at``, ``first_at``; -1: none),
        ``open_bucket`` (``min``, ``max``, ``frames``), ``pairs`` and ``sum_xy``; with ``overview`` the complete buckets emitted since
        the last such read, float32 ``[channels, n, 2]`` from bucket ``first_bucket`` on (drained). The programme is not disturbed.
        Raises on an engine whose inspector is off."""
        import numpy as np
        info = _QcInfo()
        self._spectrum_check("elemhip_qc_read", self._lib.elemhip_qc_read(self._h, C.byref(info), None, 0, None, 0))
        ch, npairs, queued = int(info.channels), int(info.pairs), int(info.queued)
        recs = (_QcChannel * max(ch, 1))()
        sums = np.zeros(max(npairs, 1), dtype=np.float64)
        self._spectrum_check("elemhip_qc_read", self._lib.elemhip_qc_read(self._h, C.byref(info), recs, ch, sums.ctypes.data_as(C.POINTER(C.c_double)), npairs))
        out = _qc_channels([recs[c] for c in range(ch)], getattr(self, "_qc_pairs", np.zeros((0, 2), dtype=np.uint32))[:npairs], sums[:npairs])
        out.update({"bucket": int(info.bucket), "delivered": int(info.delivered), "programme_frames": int(info.frames), "first_bucket": int(info.first_bucket)})
        if overview:
            buf = np.zeros(max(ch * queued * 2, 1), dtype=np.float32)
            self._spectrum_check("elemhip_qc_overview", self._lib.elemhip_qc_overview(self._h, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.size))
            out["overview"] = buf[:ch * queued * 2].reshape(ch, queued, 2).copy()
        return out

    def qc_reset(self) -> None:
        """``elemhip_qc_reset``: a new programme; buckets nobody read are dropped."""
        self._spectrum_check("elemhip_qc_reset", self._lib.elemhip_qc_reset(self._h))

    def automation(self, channel: int, points) -> None:
        """``elemhip_automation_set``: binds a lane — ``(frame, value[, "hold" | "linear"])`` rows sorted by frame
        (``elementary_amd.automation``: ``ramp``, ``steps`` and the value rule) — to engine input channel ``channel`` (0 .. 31) of the
        host-buffer render calls; frame ``f`` of a call reads the lane's value at ``sample_time + f``, expanded on the GPU. The channel
        must lie at or above the inputs a call supplies. ``points`` empty or None clears the lane. A lane the engine refuses raises with
        ``.code`` 6 and changes nothing."""
        arr, count = _automation_points(points or [])
        self._spectrum_check("elemhip_automation_set", self._lib.elemhip_automation_set(self._h, int(channel), arr if count else None, count))

    def automation_read(self, channel: int) -> Dict[str, Any]:
        """``elemhip_automation_read``: ``{'points': [(frame, value, curve code), ...] of the channel's lane, 'channels': the bound
        channels, 'inputs': highest bound channel + 1}``."""
        info = _AutomationInfo()
        self._spectrum_check("elemhip_automation_read", self._lib.elemhip_automation_read(self._h, int(channel), C.byref(info), None, 0))
        arr = (_AutomationPoint * max(1, int(info.count)))()
        self._spectrum_check("elemhip_automation_read", self._lib.elemhip_automation_read(self._h, int(channel), C.byref(info), arr, len(arr)))
        return {"points": [(int(arr[i].frame), float(arr[i].value), int(arr[i].curve)) for i in range(int(info.count))],
                "channels": [c for c in range(32) if info.lanes >> c & 1], "inputs": int(info.inputs)}

    def automation_reset(self) -> None:
        """``elemhip_automation_reset``: clears every lane."""
        self._spectrum_check("elemhip_automation_reset", self._lib.elemhip_automation_reset(self._h))

    def event_window_blocks(self) -> int:
        """Blocks a ``process_queued_events(blockwise=True)`` window may span and still equal a relay after every block."""
        f = self._lib.elemhip_event_window_blocks
        f.argtypes = [C.c_void_p]
        f.restype = C.c_uint32
        return int(f(self._h))

    def set_stream(self, hip_stream: int) -> None:
        self._lib.elemhip_set_stream(self._h, C.c_void_p(hip_stream))

    def set_option(self, key: str, value: float) -> None:
        rc = self._lib.elemhip_set_option(self._h, key.encode(), float(value))
        if rc != 0:
            err = ElemHipError(f"unknown option {key!r}")
            err.code = rc
            raise err

    def time_launches(self, num_outputs: int, num_blocks: int):
        """Mean HIP-event duration (ms) of each launch level and of the epilogue kernel."""
        buf = (C.c_float * 64)()
        k = self._lib.elemhip_time_launches(self._h, num_outputs, int(num_blocks), buf, 64)
        if k < 0:
            raise ElemHipError(f"elemhip_time_launches failed: {describe(-k)}")
        self.last_event_overhead_ms = float(buf[k])   # empty event pair, already subtracted
        self.last_time_batch = max(1, int(buf[k + 1]))   # blocks per timed launch (option "time_batch")
        self.sample_time += int(num_blocks) * self.block_size * self.last_time_batch
        return [float(buf[i]) for i in range(k)]

    def launch_profile(self):
        """Per-launch-level HIP-event time of the multi-block launches issued since ``set_option('profile_launches', 1)``:
        ``{'level_ms': [...], 'epilogue_ms': x, 'launch_sets': n, 'blocks': b}`` (sums over the profiled launch sets)."""
        buf = (C.c_double * 64)()
        sets, blocks = C.c_uint64(0), C.c_uint64(0)
        f = self._lib.elemhip_get_launch_profile
        f.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        f.restype = C.c_int
        k = f(self._h, buf, 64, C.byref(sets), C.byref(blocks))
        if k <= 0:
            return {"level_ms": [], "epilogue_ms": 0.0, "launch_sets": int(sets.value), "blocks": int(blocks.value)}
        if k > 64:      # more launch levels than the first buffer holds: ask again with room for all of them
            buf = (C.c_double * k)()
            k = min(k, f(self._h, buf, k, C.byref(sets), C.byref(blocks)))
        vals = [float(buf[i]) for i in range(k)]
        return {"level_ms": vals[:-1], "epilogue_ms": vals[-1], "launch_sets": int(sets.value), "blocks": int(blocks.value)}

    def spec_info(self, k: int = 0) -> Dict[str, Any]:
        """The k-th specialised island shape of the newest plan: program text, compiler log, state, islands covered."""
        f = self._lib.elemhip_spec_info
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]
        f.restype = C.c_int
        src, log = C.create_string_buffer(4 << 20), C.create_string_buffer(1 << 20)    # (C2 voice: 170 KB of text)
        state, isl = C.c_int(0), C.c_uint32(0)
        n = f(self._h, k, src, len(src), log, len(log), C.byref(state), C.byref(isl))
        return {"shapes": n, "source": src.value.decode(), "log": log.value.decode(errors="replace"), "state": state.value, "islands": isl.value}

    def describe_plan(self) -> Dict[str, Any]:
        import json
        buf = C.create_string_buffer(1 << 20)
        self._lib.elemhip_describe_plan(self._h, buf, len(buf))
        return json.loads(buf.value)

    def stats(self) -> Dict[str, Any]:
        s = _Stats()
        self._lib.elemhip_get_stats(self._h, C.byref(s))
        return {k: getattr(s, k) for k, _ in _Stats._fields_}
