"""Helpers of the spectrum analyser (``Runtime.spectrum``; elementary_amd/csrc/spectrum.h): analysis windows in float64, mel band
rows, and the decibel scale the device deliberately leaves to the host.

A band row is ``(first_bin, weights)``: ``weights`` float32, one per bin from ``first_bin`` on (it may be empty). The engine sums
``weights[i] * power[first_bin + i]`` in float64 in ascending bin order."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

SIZES = (256, 512, 1024, 2048, 4096)
MAX_BANDS = 512

BandRow = Tuple[int, np.ndarray]


def window(name: str, size: int) -> np.ndarray:
    """``size`` float64 values: ``"hann"`` — periodic, ``0.5 - 0.5 cos(2 pi i / size)``, the STFT window that sums to a constant at
    hops dividing ``size / 2``; ``"blackman-harris"`` — the four-term window of the ``fft`` node (``ffr::make_window``: the argument is
    ``i / (size - 1)``); ``"rect"`` — ones."""
    i = np.arange(int(size), dtype=np.float64)
    if name == "hann":
        return 0.5 - 0.5 * np.cos(2.0 * np.pi * i / float(size))
    if name in ("blackman-harris", "blackman_harris"):
        t = i / float(size - 1)
        return 0.35875 - 0.48829 * np.cos(2.0 * np.pi * t) + 0.14128 * np.cos(4.0 * np.pi * t) - 0.01168 * np.cos(6.0 * np.pi * t)
    if name == "rect":
        return np.ones(int(size), dtype=np.float64)
    raise ValueError(f"unknown window {name!r}: 'hann', 'blackman-harris' or 'rect'")


def hz_to_mel(f):
    """HTK mel scale: ``2595 log10(1 + f / 700)``."""
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_to_hz(m):
    return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)


def mel_bands(sample_rate: float, size: int, n: int, fmin: float = 0.0, fmax: Optional[float] = None) -> List[BandRow]:
    """``n`` unnormalised triangular filters on the HTK mel scale between ``fmin`` and ``fmax`` (default: Nyquist), as band rows over the
    ``size / 2 + 1`` bins of a ``size``-point transform: ``n + 2`` edges equally spaced in mel; filter ``b`` rises from edge ``b`` to 1 at
    edge ``b + 1`` and falls to 0 at edge ``b + 2``. A row holds the bins where its weight is positive (none for a triangle narrower
    than a bin that straddles no bin centre)."""
    fmax = float(sample_rate) / 2.0 if fmax is None else float(fmax)
    if not (0.0 <= fmin < fmax <= float(sample_rate) / 2.0) or n < 1:
        raise ValueError("mel_bands: 0 <= fmin < fmax <= sample_rate / 2 and n >= 1")
    edges = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), int(n) + 2))
    freqs = np.arange(int(size) // 2 + 1, dtype=np.float64) * float(sample_rate) / float(size)
    rows: List[BandRow] = []
    for b in range(int(n)):
        lo, mid, hi = edges[b], edges[b + 1], edges[b + 2]
        w = np.minimum((freqs - lo) / (mid - lo), (hi - freqs) / (hi - mid))
        idx = np.nonzero(w > 0.0)[0]
        if idx.size == 0:
            rows.append((0, np.zeros(0, dtype=np.float32)))
        else:
            rows.append((int(idx[0]), w[idx[0]:idx[-1] + 1].astype(np.float32)))
    return rows


def pack_rows(rows: Sequence[BandRow]):
    """Band rows as the C-ABI takes them: ``(first uint32[B], count uint32[B], weights float32[sum count])``."""
    first = np.array([int(r[0]) for r in rows], dtype=np.uint32)
    ws = [np.ascontiguousarray(r[1], dtype=np.float32).reshape(-1) for r in rows]
    count = np.array([w.size for w in ws], dtype=np.uint32)
    weights = np.concatenate(ws) if ws else np.zeros(0, dtype=np.float32)
    return first, count, np.ascontiguousarray(weights, dtype=np.float32)


def to_db(power, floor_db: float = -200.0, ref: float = 1.0):
    """``10 log10(power / ref)``, not below ``floor_db`` (zero power gives the floor)."""
    p = np.asarray(power, dtype=np.float64) / float(ref)
    with np.errstate(divide="ignore"):
        return np.maximum(10.0 * np.log10(p), float(floor_db))
