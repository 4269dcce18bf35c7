"""ITU-R BS.1770-4 / EBU R 128 in numpy, serial and in float64: the K-weighting (the two analog prototypes, bilinear-transformed at
the signal's sample rate), mean squares over 100 ms sub-blocks, the gated integrated loudness, and the true peak by 4x oversampling
with a 49-tap windowed-sinc interpolator. Written from the standard and the filter formulas of the meter's specification, not from
elementary_amd/csrc/loudness.h: direct form I recurrences sample by sample, the interpolator as one convolution of the zero-stuffed
signal."""
import math

import numpy as np

ABS_GATE = -70.0
REL_GATE = -10.0


def shelf(fs):
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]
    a = [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return b, a


def highpass(fs):
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    return [1.0, -2.0, 1.0], [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]


def hop(fs):
    return int(math.floor(fs / 10.0 + 0.5))


def _biquad(b, a, x):
    """y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2], zero initial conditions."""
    n = len(x)
    v = b[0] * x
    v[1:] += b[1] * x[:-1]
    v[2:] += b[2] * x[:-2]
    a1, a2 = a[1], a[2]
    y1 = y2 = 0.0
    out = []
    push = out.append
    for t in v.tolist():
        y = t - a1 * y1 - a2 * y2
        y2 = y1
        y1 = y
        push(y)
    return np.array(out, dtype=np.float64) if n else np.zeros(0)


def clean(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isfinite(x), x, 0.0)


def kweight(x, fs):
    """One channel, float64 out."""
    return _biquad(*highpass(fs), _biquad(*shelf(fs), clean(x)))


def mean_squares(x, fs):
    """x [channels, frames] -> [channels, frames // hop]: the mean square of the K-weighted signal over each whole sub-block."""
    x = np.atleast_2d(np.asarray(x))
    h = hop(fs)
    n = x.shape[1] // h
    out = np.zeros((x.shape[0], n), dtype=np.float64)
    seen = {}
    for c in range(x.shape[0]):
        key = x[c].tobytes()
        if key not in seen:
            y = kweight(x[c], fs)[:n * h]
            seen[key] = (y * y).reshape(n, h).sum(axis=1) / h if n else np.zeros(0)
        out[c] = seen[key]
    return out


def interpolator():
    j = np.arange(49, dtype=np.float64)
    h = np.sinc((j - 24.0) / 4.0) * 0.5 * (1.0 - np.cos(2.0 * np.pi * j / 48.0))
    for p in range(4):
        h[p::4] /= h[p::4].sum()
    return h


def true_peak(x):
    """x [channels, frames] -> per channel max(|x|, |4x zero-stuffed x convolved ("full") with the interpolator|), linear."""
    x = np.atleast_2d(np.asarray(x))
    h = interpolator()
    out = np.zeros(x.shape[0], dtype=np.float64)
    for c in range(x.shape[0]):
        xc = clean(x[c])
        if len(xc) == 0:
            continue
        up = np.zeros(4 * len(xc), dtype=np.float64)
        up[::4] = xc
        out[c] = max(float(np.abs(xc).max()), float(np.abs(np.convolve(up, h)).max()))
    return out


def sample_peak(x):
    x = np.atleast_2d(np.asarray(x))
    return np.abs(clean(x)).max(axis=1).astype(np.float32) if x.shape[1] else np.zeros(x.shape[0], np.float32)


def _lufs(p):
    return -0.691 + 10.0 * math.log10(p) if p > 0.0 else -math.inf


def gate(ms, weights=None):
    """ms [channels, sub-blocks] -> integrated / momentary max / short-term max loudness (LUFS)."""
    ms = np.atleast_2d(np.asarray(ms, dtype=np.float64))
    w = np.ones(ms.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64)
    n = ms.shape[1]

    def powers(length):
        return [float(np.dot(w, ms[:, i:i + length].sum(axis=1) / length)) for i in range(0, n - length + 1)]

    short = [_lufs(p) for p in powers(30)]
    res = {"integrated": -math.inf, "momentary_max": -math.inf, "short_term_max": max(short) if short else -math.inf}
    blocks = powers(4)
    if not blocks:
        return res
    loud = [_lufs(p) for p in blocks]
    res["momentary_max"] = max(loud)
    kept = [p for p, l in zip(blocks, loud) if l > ABS_GATE]
    if not kept:
        return res
    rel = _lufs(sum(kept) / len(kept)) + REL_GATE
    kept = [p for p, l in zip(blocks, loud) if l > ABS_GATE and l > rel]
    if kept:
        res["integrated"] = _lufs(sum(kept) / len(kept))
    return res


def dbtp(peak):
    return 20.0 * math.log10(peak) if peak > 0.0 else -math.inf


BOUND_REL, BOUND_ABS = 1e-9, 1e-24


def close(got, want):
    """|got - want| <= 1e-9 * want + 1e-24, elementwise (want >= 0); returns (ok, index of the first miss or None)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False, ("shape", got.shape, want.shape)
    bad = np.argwhere(~(np.abs(got - want) <= BOUND_REL * np.abs(want) + BOUND_ABS))
    return (len(bad) == 0), (tuple(int(i) for i in bad[0]) if len(bad) else None)
