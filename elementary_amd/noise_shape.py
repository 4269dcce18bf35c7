"""Noise-shaping filters for s16 / s24 / FLAC delivery (``Runtime.noise_shape``, ``OfflineRenderer.initialize(noise_shape=...)``).

A filter is the list c_1 .. c_K of an error-feedback quantiser: the requantisation error leaves with the spectrum of plain TPDF dither
times the noise transfer function NTF(z) = 1 - sum c_k z^-k, and with 1 + sum c_k^2 times its power. ``first`` and ``second`` are the
plain differentiators and fit any rate; the other presets are psychoacoustic designs for 44.1 kHz — they move the noise out of the
2 - 5 kHz region towards the top of the band — and are accepted at 44100 and 48000 Hz only.
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import numpy as np

PRESETS = {
    "first": [1.0],
    "second": [2.0, -1.0],
    # the 5- and 9-tap designs of Lipshitz, Vanderkooy and Wannamaker, "Minimally audible noise shaping", JAES 39 (1991), as commonly
    # quoted for 44.1 kHz
    "lipshitz5": [2.033, -2.165, 1.959, -1.590, 0.6149],
    "fweighted9": [2.412, -3.370, 3.937, -4.174, 3.353, -2.205, 1.281, -0.569, 0.0847],
    "modified_e9": [1.662, -1.263, 0.4827, -0.2913, 0.1268, -0.1124, 0.03252, -0.01265, -0.03524],
}
PSYCHOACOUSTIC = ("lipshitz5", "fweighted9", "modified_e9")
PSYCHOACOUSTIC_RATES = (44100, 48000)
MAX_TAPS = 12


def ntf_db(coeffs: Sequence[float], freqs, rate: float) -> np.ndarray:
    """|NTF| in dB at ``freqs`` (Hz) for a delivery rate of ``rate``: 20 log10 |1 - sum c_k e^(-j 2 pi f k / rate)|."""
    c = np.asarray(coeffs, dtype=np.float64).reshape(-1)
    w = 2.0 * np.pi * np.asarray(freqs, dtype=np.float64) / float(rate)
    k = np.arange(1, c.size + 1, dtype=np.float64)
    h = 1.0 - np.exp(-1j * np.multiply.outer(w, k)) @ c
    return 20.0 * np.log10(np.maximum(np.abs(h), 1e-300))


def power_gain(coeffs: Sequence[float]) -> float:
    """1 + sum c_k^2: the shaped error's total power over plain dither's."""
    c = np.asarray(coeffs, dtype=np.float64).reshape(-1)
    return float(1.0 + np.sum(c * c))


def resolve(spec: Union[None, str, Sequence[float]], rate: Optional[float] = None) -> Optional[list]:
    """A preset's name or raw coefficients -> the coefficient list (None / empty: off). A psychoacoustic preset at a delivery rate
    other than 44100 or 48000 raises ValueError; raw coefficients are taken at any rate."""
    if spec is None or spec is False:
        return None
    if isinstance(spec, str):
        if spec not in PRESETS:
            raise ValueError(f"unknown noise-shaping preset {spec!r}: one of {sorted(PRESETS)}")
        if spec in PSYCHOACOUSTIC and rate is not None and int(round(float(rate))) not in PSYCHOACOUSTIC_RATES:
            raise ValueError(f"noise-shaping preset {spec!r} is a 44.1 kHz design: the delivery rate is {rate:g}, not 44100 or 48000")
        return list(PRESETS[spec])
    c = [float(v) for v in np.asarray(spec, dtype=np.float64).reshape(-1)]
    if len(c) > MAX_TAPS:
        raise ValueError(f"at most {MAX_TAPS} noise-shaping coefficients, got {len(c)}")
    return c or None
