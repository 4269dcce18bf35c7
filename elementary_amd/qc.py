"""Helpers of the inspector (``Runtime.qc``; elementary_amd/csrc/qc.h): the figures derived from a read and the verdicts against a
caller's limits. ``read`` is what ``Runtime.qc_read``, ``OfflineRenderer.qc`` or ``runtime.qc_host`` return."""
import math
from typing import Any, Dict, List, Optional

import numpy as np


def report(read: Dict[str, Any], sample_rate: float) -> Dict[str, Any]:
    """Per channel: ``dc`` (sum / frames), ``rms_dbfs`` (-inf for silence), ``head_silence_s`` and ``tail_silence_s``; per pair
    ``correlation`` = sum_xy / sqrt(sum_sq_a * sum_sq_b), ``nan`` where a side is silent. A programme of no frames gives zeros."""
    frames = np.asarray(read["frames"], dtype=np.float64)
    n = np.maximum(frames, 1.0)
    mean_sq = np.asarray(read["sum_sq"], dtype=np.float64) / n
    with np.errstate(divide="ignore"):
        rms = np.where(mean_sq > 0, 10.0 * np.log10(np.where(mean_sq > 0, mean_sq, 1.0)), -np.inf)
    corr = []
    for k, (a, b) in enumerate(read["pairs"]):
        den = math.sqrt(float(read["sum_sq"][a]) * float(read["sum_sq"][b]))
        corr.append(float(read["sum_xy"][k]) / den if den > 0 else float("nan"))
    return {"dc": np.asarray(read["sum"], dtype=np.float64) / n, "rms_dbfs": rms,
            "head_silence_s": np.asarray(read["head_silence"], dtype=np.float64) / float(sample_rate),
            "tail_silence_s": np.asarray(read["tail_silence"], dtype=np.float64) / float(sample_rate),
            "correlation": np.array(corr, dtype=np.float64), "pairs": list(read["pairs"])}


def findings(read: Dict[str, Any], sample_rate: float, max_head_s: Optional[float] = None, max_tail_s: Optional[float] = None,
             max_dc: Optional[float] = None, min_correlation: Optional[float] = None) -> List[Dict[str, Any]]:
    """Plain records ``{'kind', 'channel', 'at', 'length', 'value'}`` for whatever exceeds the caller's limits — kinds 'head_silence',
    'tail_silence', 'dropout', 'clip', 'nonfinite', 'dc' and 'correlation' (``channel``: the pair's index there). ``at`` and ``length``
    are programme frames (-1: not applicable). Dropouts, clip events and non-finite samples are always findings; a limit of None
    is not checked. Raises nothing."""
    rep = report(read, sample_rate)
    out: List[Dict[str, Any]] = []

    def add(kind, channel, at, length, value):
        out.append({"kind": kind, "channel": int(channel), "at": int(at), "length": int(length), "value": float(value)})

    for c in range(len(read["frames"])):
        frames = int(read["frames"][c])
        if max_head_s is not None and rep["head_silence_s"][c] > max_head_s:
            add("head_silence", c, 0, read["head_silence"][c], rep["head_silence_s"][c])
        if max_tail_s is not None and rep["tail_silence_s"][c] > max_tail_s:
            add("tail_silence", c, frames - int(read["tail_silence"][c]), read["tail_silence"][c], rep["tail_silence_s"][c])
        if read["dropouts"]["count"][c] > 0:
            add("dropout", c, read["dropouts"]["longest_at"][c], read["dropouts"]["longest"][c], read["dropouts"]["count"][c])
        if read["clip_events"]["count"][c] > 0:
            add("clip", c, read["clip_events"]["longest_at"][c], read["clip_events"]["longest"][c], read["clip_events"]["count"][c])
        if read["nonfinite"][c] > 0:
            add("nonfinite", c, -1, -1, read["nonfinite"][c])
        if max_dc is not None and abs(rep["dc"][c]) > max_dc:
            add("dc", c, -1, -1, rep["dc"][c])
    if min_correlation is not None:
        for k, r in enumerate(rep["correlation"]):
            if not math.isnan(r) and r < min_correlation:
                add("correlation", k, -1, -1, r)
    return out
