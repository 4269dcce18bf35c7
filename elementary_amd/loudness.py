"""EBU R 128 gating over the sub-block series the loudness meter returns (``Runtime.loudness_read``), through the C-ABI's
``elemhip_loudness_gate`` — the arithmetic lives once, in elementary_amd/csrc/loudness.h, for hosts with and without Python."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np

from .runtime import ElemHipError, _LoudnessResult, describe, load_library


def gate(ms, weights=None) -> Dict[str, float]:
    """``ms``: mean squares ``[channels, sub_blocks]`` of 100 ms sub-blocks (K-weighted); ``weights``: one per channel (default 1.0;
    BS.1770 gives the surround channels 1.41). Returns ``{'integrated', 'momentary_max', 'short_term_max'}`` in LUFS (``-inf`` where
    no block passes the gates / the programme is shorter than the window) and the block counts ``'blocks'`` / ``'gated_blocks'``."""
    a = np.ascontiguousarray(ms, dtype=np.float64)
    if a.ndim == 1:
        a = a[None, :]
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    if w is not None and w.shape != (a.shape[0],):
        raise ValueError(f"{a.shape[0]} channels, weights of shape {w.shape}")
    out = _LoudnessResult()
    dp = C.POINTER(C.c_double)
    rc = load_library().elemhip_loudness_gate(a.ctypes.data_as(dp), a.shape[0], a.shape[1], None if w is None else w.ctypes.data_as(dp), C.byref(out))
    if rc != 0:
        raise ElemHipError(f"elemhip_loudness_gate failed: {describe(rc)} (code {rc})")
    return {"integrated": float(out.integrated), "momentary_max": float(out.momentary_max), "short_term_max": float(out.short_term_max),
            "blocks": int(out.blocks), "gated_blocks": int(out.gated_blocks)}


def lufs(x) -> float:
    """A mean-square power (channel weights applied, channels summed) as loudness: ``-0.691 + 10 log10 x``; ``-inf`` at 0."""
    x = float(x)
    return float(-0.691 + 10.0 * np.log10(x)) if x > 0.0 else float("-inf")


def dbtp(peak) -> float:
    """A linear true peak in dBTP; ``-inf`` at 0."""
    peak = float(peak)
    return float(20.0 * np.log10(peak)) if peak > 0.0 else float("-inf")
