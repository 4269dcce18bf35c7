"""``master_wav`` — a RIFF/WAVE or FLAC file brought to a delivery spec ("-14 LUFS, -1 dBTP") on the GPU, in two passes over a pass-through
graph: the first meters the input (BS.1770 integrated loudness and true peak), the second applies ``target - measured`` dB of static
gain and the look-ahead true-peak limiter and meters what it writes. No sample is scaled or limited on the host."""
from __future__ import annotations

from typing import Any, Callable, Dict

import numpy as np

from . import el
from .offline import OfflineRenderer
from .flac import FlacReader
from .wav import WavReader


def _reader(path):
    """The input's reader: ``FlacReader`` for a file that starts with ``fLaC`` (its frames are decoded on the GPU), else ``WavReader``."""
    with open(path, "rb") as f:
        flac = f.read(4) == b"fLaC"
    return FlacReader(path) if flac else WavReader(path)


def master_wav(engine_factory: Callable[[float, int], Any], in_path, out_path, target_lufs: float = -14.0, ceiling_dbtp: float = -1.0,
               fmt: str = "s24", block_size: int = 512, oversample: int = 1, noise_shape=None, verify_input: bool = False, qc=None, **limiter) -> Dict[str, Any]:
    """``in_path`` -> ``out_path`` (format ``fmt`` — 's16', 's24', 'f32', or 'flac16' / 'flac24' for a FLAC file encoded on the GPU —
    the input's rate and channel count) at ``target_lufs`` integrated loudness under a
    true-peak ceiling of ``ceiling_dbtp``. ``limiter``: further limiter parameters (``lookahead_ms``, ``release_ms``, ``link``).
    ``qc``: an inspector spec (``Runtime.qc``; None: off) — the second pass is inspected on the GPU and the read-out of the file it wrote
    comes back under ``'qc'`` (``elementary_amd.qc.report`` / ``findings`` derive the figures and the verdicts).
    Returns ``{'input_lufs', 'input_true_peak_dbtp', 'output_lufs', 'output_true_peak_dbtp', 'gain_db', 'max_reduction_db',
    'limited_frames', 'over', 'nonfinite'}``. Where the limiter worked the output is quieter than the target by what it took away; the
    output's metered true peak may exceed the ceiling slightly (``OfflineRenderer.initialize``). An input that passes no loudness
    gate (silence) raises ``ValueError``: there is no gain that brings it to a target.

    ``verify_input`` (a FLAC input): the metering pass also hashes the decoded samples on the GPU (option ``flac_in_md5``) and compares
    the digest with what the file's STREAMINFO announces; the result carries ``input_md5`` (['ok'], ['absent'], ...), and a mismatch
    raises ``FlacMd5Mismatch`` BEFORE the second pass opens the output: a damaged source does not become a deliverable.

    Both passes meter on the same grid: the limiter delays its output by ``latency_frames``, so the first pass puts as many frames of
    silence in front of the input — the second pass's figures then differ from the first's by the gain and the limiter alone.

    ``oversample`` = k > 1: the engine runs at k times the file's rate with ``input_sample_rate`` and ``output_sample_rate`` both the
    file's, in both passes — the file is converted up on the GPU in front of the graph and down again behind it. Nothing else
    changes: the limiter and the meter still work on what is delivered, at the file's rate, and the output has the input's rate and
    length. The first pass renders the converters' latencies out behind the file, so both passes still meter on one grid."""
    k = int(oversample)
    if k < 1:
        raise ValueError("oversample is a whole factor of 1 or more")
    unknown = set(limiter) - {"lookahead_ms", "release_ms", "link"}
    if unknown:
        raise ValueError(f"unknown limiter parameters: {sorted(unknown)}")
    with _reader(str(in_path)) as r:
        rate, channels, frames, in_fmt = float(r.sample_rate), int(r.channels), int(r.frames), r.fmt
    from .noise_shape import resolve
    shape = None if fmt == "f32" else resolve(noise_shape, rate)      # (refused here, before anything is rendered)
    sil_fmt = "s16" if in_fmt == "flac" else in_fmt      # (silence is fed as PCM: a FLAC input is decoded to PCM on the GPU anyway)

    def renderer(**kw):
        core = OfflineRenderer(engine_factory)
        if k > 1:
            kw = dict(kw, input_sample_rate=rate, output_sample_rate=rate)
        core.initialize(num_input_channels=channels, num_output_channels=channels, sample_rate=rate * k, block_size=int(block_size),
                        loudness_meter=True, **kw)
        core.render(*[el.in_({"channel": c}) for c in range(channels)])
        # the roots fade in over 20 ms of engine time: let that pass on silence, then start the meter's programme
        warm = -(-int(0.05 * rate * k) // int(block_size)) * int(block_size)
        core.process_pcm_io([silence(warm)], sil_fmt, warm)
        core.loudness_reset()
        if k > 1:                                  # the converters' programmes start with the meter's
            core.input_resample_reset()
            core.resample_reset()
        return core

    def silence(n):
        shape, dtype = {"s16": ((n, channels), np.int16), "s24": ((n, channels, 3), np.uint8)}.get(sil_fmt, ((n, channels), np.float32))
        return np.zeros(shape, dtype=dtype)

    params = dict(limiter, ceiling_dbtp=float(ceiling_dbtp))
    # the limiter's latency at this rate, from a plan of the same parameters
    probe = renderer(limiter=dict(params, gain_db=0.0))
    latency = probe.limiter()["latency_frames"]
    del probe
    first = renderer()
    first.process_pcm_io([silence(latency)], sil_fmt, latency * k)      # (every call renders a multiple of k engine frames: it consumes its frames / k)
    verify = bool(verify_input) and in_fmt == "flac"
    verdicts = {}
    with _reader(str(in_path)) as r:
        if verify:
            first.verify_begin()
        done = 0
        while done < frames:
            m = min(1 << 20, frames - done)
            first.process_pcm_io([r.read(m)], in_fmt, m * k)
            done += m
        if verify:
            verdicts = {"input_md5": first.verify_end([r.md5])}
    if k > 1:
        # what the second pass renders behind the file to take the converters' latencies out (OfflineRenderer._file_span)
        tail = first.resample()["latency_frames"] + (2 * first.input_resample()["latency_frames"] + k) // (2 * k)
        first.process_pcm_io([silence(1)], sil_fmt, tail * k)
    measured = first.loudness()
    if not np.isfinite(measured["integrated_lufs"]):
        raise ValueError("the input passes no loudness gate: no gain brings it to a target")
    gain_db = float(target_lufs) - float(measured["integrated_lufs"])
    second = renderer(limiter=dict(params, gain_db=gain_db), noise_shape=shape, **({} if qc is None else {"qc": dict(qc)}))
    stats = second.process_wav(str(in_path), str(out_path), fmt)
    lim = second.limiter()
    shaped = {"saturated": int(np.sum(second.noise_shape()["saturated"]))} if shape else {}
    if qc is not None:        # the inspector's report of the file the second pass wrote (elementary_amd.qc.report derives the figures)
        verdicts = dict(verdicts, qc=stats["qc"])
    return {**shaped, **verdicts, "input_lufs": float(measured["integrated_lufs"]), "input_true_peak_dbtp": float(measured["true_peak_dbtp"]),
            "output_lufs": float(stats["integrated_lufs"]), "output_true_peak_dbtp": float(stats["true_peak_dbtp"]), "gain_db": gain_db,
            "max_reduction_db": float(lim["max_reduction_db"]), "max_reduction": float(np.max(lim["max_reduction"], initial=0.0)),
            "limited_frames": int(np.sum(lim["limited_frames"])), "over": int(np.sum(stats["over"])), "nonfinite": int(np.sum(stats["nonfinite"]))}
