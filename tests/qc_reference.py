"""The inspector's definitions restated in numpy (not a transcription of elementary_amd/csrc/qc.h): flags per frame, runs by run-length
encoding from np.diff, the sums with math.fsum. ``inspect(x, ...)`` returns what ``Runtime.qc_read`` returns for the programme ``x``
float32 [channels, frames]; ``compare(got, want)`` holds every exact field with == and the float64 sums to the bound for an arbitrary
summation order of n terms, |got - fsum| <= gamma * sum|t| with gamma = (n - 1) u / (1 - (n - 1) u), u = 2^-53 (the terms x, x^2 and
x_a x_b of float32 operands are exact in double, so the additions are the only roundings)."""
import math

import numpy as np

U = 2.0 ** -53
EXACT = ("frames", "nonfinite", "quiet_frames", "clipped_frames", "peak_at", "head_silence", "tail_silence")
RUNS = ("count", "longest", "longest_at", "first_at")


def clean(x):
    x = np.asarray(x, dtype=np.float32)
    return np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float32)


def runs_of(flags):
    """(starts, lengths) of the maximal runs of True."""
    f = np.concatenate([[0], np.asarray(flags, dtype=np.int8), [0]])
    d = np.diff(f)
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    return starts, ends - starts


def _findings(starts, lengths):
    if not len(starts):
        return {"count": 0, "longest": 0, "longest_at": -1, "first_at": -1}
    k = int(np.argmax(lengths))            # (the first of equals)
    return {"count": int(len(starts)), "longest": int(lengths[k]), "longest_at": int(starts[k]), "first_at": int(starts[0])}


def gamma(n):
    return (n - 1) * U / (1.0 - (n - 1) * U) if n > 1 else 0.0


def inspect(x, silence_level=0.0, clip_level=1.0, clip_run=3, dropout_frames=64, bucket=0, pairs=(), skip=0, limit=0):
    x = np.asarray(x, dtype=np.float32)
    x = x[:, skip:]
    if limit:
        x = x[:, :limit]
    ch, n = x.shape
    c = clean(x)
    keys = EXACT + ("min", "max", "sum", "sum_sq", "sum_bound", "sum_sq_bound")
    out = {k: [] for k in keys}
    out["dropouts"] = {k: [] for k in RUNS}
    out["clip_events"] = {k: [] for k in RUNS}
    for i in range(ch):
        a = np.abs(c[i])
        quiet, clipped = a <= np.float32(silence_level), a >= np.float32(clip_level)
        out["frames"].append(n)
        out["nonfinite"].append(int((~np.isfinite(x[i])).sum()))
        out["quiet_frames"].append(int(quiet.sum()))
        out["clipped_frames"].append(int(clipped.sum()))
        out["min"].append(np.float32(c[i].min()) if n else np.float32(0))
        out["max"].append(np.float32(c[i].max()) if n else np.float32(0))
        out["peak_at"].append(int(np.argmax(a)) if n else -1)
        qs, ql = runs_of(quiet)
        head = int(ql[0]) if len(qs) and qs[0] == 0 else 0
        tail = int(ql[-1]) if len(qs) and qs[-1] + ql[-1] == n else 0
        out["head_silence"].append(head)
        out["tail_silence"].append(tail)
        inner = (qs > 0) & (qs + ql < n) & (ql >= dropout_frames)
        cs, cl = runs_of(clipped)
        long_enough = cl >= clip_run
        for name, f in (("dropouts", _findings(qs[inner], ql[inner])), ("clip_events", _findings(cs[long_enough], cl[long_enough]))):
            for k in RUNS:
                out[name][k].append(f[k])
        d = c[i].astype(np.float64)
        out["sum"].append(math.fsum(d))
        out["sum_sq"].append(math.fsum(d * d))
        out["sum_bound"].append(gamma(n) * math.fsum(np.abs(d)))
        out["sum_sq_bound"].append(gamma(n) * math.fsum(d * d))
    for k in EXACT:
        out[k] = np.array(out[k], dtype=np.int64)
    for name in ("dropouts", "clip_events"):
        for k in RUNS:
            out[name][k] = np.array(out[name][k], dtype=np.int64)
    for k in ("min", "max"):
        out[k] = np.array(out[k], dtype=np.float32)
    for k in ("sum", "sum_sq", "sum_bound", "sum_sq_bound"):
        out[k] = np.array(out[k], dtype=np.float64)
    out["pairs"] = [tuple(p) for p in pairs]
    xy = [c[a].astype(np.float64) * c[b].astype(np.float64) for a, b in pairs]
    out["sum_xy"] = np.array([math.fsum(t) for t in xy], dtype=np.float64)
    out["sum_xy_bound"] = np.array([gamma(n) * math.fsum(np.abs(t)) for t in xy], dtype=np.float64)
    if bucket:
        k = n // bucket
        body = c[:, :k * bucket].reshape(ch, k, bucket)
        out["overview"] = np.stack([body.min(axis=2), body.max(axis=2)], axis=2).astype(np.float32) if k else np.zeros((ch, 0, 2), dtype=np.float32)
        rest = c[:, k * bucket:]
        out["open_bucket"] = {"frames": np.full(ch, n - k * bucket, dtype=np.int64),
                              "min": rest.min(axis=1) if rest.shape[1] else np.zeros(ch, dtype=np.float32),
                              "max": rest.max(axis=1) if rest.shape[1] else np.zeros(ch, dtype=np.float32)}
    else:
        out["overview"] = np.zeros((ch, 0, 2), dtype=np.float32)
        out["open_bucket"] = {"frames": np.zeros(ch, dtype=np.int64), "min": np.zeros(ch, dtype=np.float32), "max": np.zeros(ch, dtype=np.float32)}
    return out


def compare(got, want, what="", overview=None):
    """Asserts `got` (a read) against `want` (inspect): == on the exact fields, the derived bound on the three kinds of sums.
    `overview`: every complete bucket of the programme so far (reads drain them: the caller concatenates)."""
    for k in EXACT:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for name in ("dropouts", "clip_events"):
        for k in RUNS:
            assert np.array_equal(got[name][k], want[name][k]), (what, name, k, got[name][k], want[name][k])
    for k in ("min", "max"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in ("sum", "sum_sq", "sum_xy"):
        err = np.abs(got[k] - want[k])
        assert got[k].shape == want[k].shape and np.all(err <= want[k + "_bound"]), (what, k, got[k], want[k], err, want[k + "_bound"])
    assert list(got["pairs"]) == list(want["pairs"]), (what, got["pairs"])
    for k in ("frames", "min", "max"):
        assert np.array_equal(got["open_bucket"][k], want["open_bucket"][k]), (what, "open bucket", k, got["open_bucket"][k], want["open_bucket"][k])
    if overview is not None:
        assert overview.shape == want["overview"].shape and np.array_equal(overview, want["overview"]), (what, "overview", overview.shape, want["overview"].shape)


def correlation(read, k):
    a, b = read["pairs"][k]
    den = math.sqrt(read["sum_sq"][a] * read["sum_sq"][b])
    return read["sum_xy"][k] / den if den > 0 else float("nan")


def exact_bytes(read):
    """Everything a read returns per channel and pair, as bytes: what must not depend on how the render was cut (sums included)."""
    parts = [np.asarray(read[k]).tobytes() for k in EXACT + ("min", "max", "sum", "sum_sq", "sum_xy")]
    parts += [np.asarray(read[n][k]).tobytes() for n in ("dropouts", "clip_events") for k in RUNS]
    parts += [np.asarray(read["open_bucket"][k]).tobytes() for k in ("frames", "min", "max")]
    return b"".join(parts)
