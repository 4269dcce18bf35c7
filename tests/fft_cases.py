"""The `fft` node's recordings (tests/golden/fft_wasm.{json,f32}, written by tests/golden/make_fft_golden.js from the reference's
wasm engine) as the tests see them: scenarios, inputs, graphs, recorded spectra, and the tolerance the recording itself sets."""
from __future__ import annotations

import json
import os

import numpy as np

from helpers import lcg_noise_fast

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = (256, 512, 1024, 2048, 4096)


def manifest():
    with open(os.path.join(GOLDEN, "fft_wasm.json")) as f:
        return json.load(f)


def recording():
    return np.fromfile(os.path.join(GOLDEN, "fft_wasm.f32"), dtype="<f4")


def e_ref(man, size) -> float:
    """max |recorded bin - float64 DFT bin| over every event of that size the reference produced (measured by the recording script)."""
    return float(man["E_ref"][str(size)])


def scenario_input(man, sc) -> np.ndarray:
    return lcg_noise_fast(sc["block"] * sc["blocks"], int(man["input_seed"]), float(man["input_amp"]))


def window(size: int) -> np.ndarray:
    """wasm/FFT.h:51-65 evaluated in double (the recorded engine is Runtime<double>)."""
    t = np.arange(size, dtype=np.float64) / (size - 1)
    return 0.35875 - 0.48829 * np.cos(2.0 * np.pi * t) + 0.14128 * np.cos(4.0 * np.pi * t) - 0.01168 * np.cos(6.0 * np.pi * t)


def raw_frame(x: np.ndarray, ev) -> np.ndarray:
    """The `size` input frames an event transformed (frames before the start of the input are the ring's initial zeros)."""
    at, size = int(ev["frame"]), int(ev["size"])
    out = np.zeros(size, np.float32)
    lo = max(0, -at)
    out[lo:] = x[at + lo:at + size]
    return out


def windowed_frame(x: np.ndarray, ev) -> np.ndarray:
    return (raw_frame(x, ev).astype(np.float64) * window(int(ev["size"]))).astype(np.float32)


def recorded_spectrum(rec: np.ndarray, ev):
    """(real, imag) of a stored event, None for one whose spectrum the fixture leaves out."""
    if ev.get("offset") is None:
        return None
    bins, at = int(ev["size"]) // 2 + 1, int(ev["offset"])
    return rec[at:at + bins], rec[at + bins:at + 2 * bins]


def fft_events(sc):
    return [e for e in sc["events"] if e["type"] == "fft"]


def roots(sc, with_fft=True, overrides=None):
    """The scenario's graph through the public interface; `with_fft=False`: every fft node replaced by its child."""
    from elementary_amd import el
    x = el.in_({"channel": 0})

    def fft(k):
        props = dict(sc["ffts"][k]["props"])
        props.update((overrides or {}).get(k, {}))
        return el.fft(props, x) if with_fft else x
    if sc["graph"] == "single":
        return [fft(0)]
    return [fft(0), el.meter(dict(sc["meter"]["props"]), fft(1))]
