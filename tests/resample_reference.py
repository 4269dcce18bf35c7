"""The yardstick of delivery-rate conversion: a numpy restatement, in float64, of the polyphase Kaiser-windowed sinc the engine's
option ``resample_rate`` applies — written from the formulas, NOT from elementary_amd/csrc/resample.h.

Plan: g = gcd(fin, fout), L = fout / g, M = fin / g, s = min(1, L / M), W = 32 / s, Wc = ceil(W), T = 2 Wc, Do = ceil(Wc L / M).
Prototype: g(t) = s sinc(s t) I0(beta sqrt(1 - (t / W)^2)) / I0(beta) for |t| < W, else 0; beta = 0.1102 (100 - 8.7).
Output n: a = (n - Do) M, i0 = floor(a / L), p = a - i0 L, y[n] = sum_k g(p / L + Wc - 1 - k) x[i0 - Wc + 1 + k], x[j] = 0 for j < 0.
After t input frames exactly ceil(t L / M) outputs exist.

``resample`` also returns, per output sample, the bound a float32 evaluation (float32 coefficients, k ascending, one or two roundings
per tap) is held to:  B[n] = (T + 4) 2^-24 sum_k |g_k x_k| + T 2^-126  — 1 for the coefficient's rounding, 1 for the product, T - 1
additions, 2 for a host I0 series that differs from numpy's in the last place; the second term covers denormal products."""
import math

import numpy as np

Z = 32
BETA = 0.1102 * (100.0 - 8.7)


def plan(fin, fout):
    fin, fout = int(fin), int(fout)
    g = math.gcd(fin, fout)
    L, M = fout // g, fin // g
    Wc = Z if L >= M else -((-Z * M) // L)
    return {"L": L, "M": M, "s": min(1.0, L / M), "W": Z / min(1.0, L / M), "Wc": Wc, "T": 2 * Wc, "Do": -((-Wc * L) // M)}


def frames_out(t, pl):
    """Outputs that exist after ``t`` input frames: ceil(t L / M)."""
    return -((-int(t) * pl["L"]) // pl["M"])


def prototype(t, pl):
    t = np.asarray(t, dtype=np.float64)
    s, W = pl["s"], pl["W"]
    inside = np.abs(t) < W
    u = np.where(inside, t / W, 0.0)
    return np.where(inside, s * np.sinc(s * t) * np.i0(BETA * np.sqrt(1.0 - u * u)) / np.i0(BETA), 0.0)


def phases(pl):
    """h[p][k] = g(p / L + Wc - 1 - k), float64 [L, T]."""
    p = np.arange(pl["L"], dtype=np.float64)[:, None]
    k = np.arange(pl["T"], dtype=np.float64)[None, :]
    return prototype(p / pl["L"] + pl["Wc"] - 1.0 - k, pl)


def resample(x, fin, fout):
    """x float [channels, t] (or [t]) -> (y, B), float64 [channels, ceil(t L / M)] each: the whole programme from time 0."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    pl = plan(fin, fout)
    L, M, Wc, T, Do = pl["L"], pl["M"], pl["Wc"], pl["T"], pl["Do"]
    t = x.shape[1]
    n = np.arange(frames_out(t, pl), dtype=np.int64)
    a = (n - Do) * M
    i0 = a // L                                   # (numpy floors)
    p = a - i0 * L
    h = phases(pl)
    pad = T + M // L + 2 + Do * M // L + 2        # every index in front of the programme that an output can reach
    xp = np.concatenate([np.zeros((x.shape[0], pad)), x, np.zeros((x.shape[0], 1))], axis=1)
    first = i0 - Wc + 1 + pad
    assert first.min(initial=0) >= 0 and (i0 + Wc).max(initial=0) < t
    y = np.zeros((x.shape[0], len(n)))
    mag = np.zeros_like(y)
    for k in range(T):
        term = h[p, k][None, :] * xp[:, first + k]
        y += term
        mag += np.abs(term)
    return y, (T + 4) * 2.0 ** -24 * mag + T * 2.0 ** -126


def response_db(proto, L, fin, nfft=1 << 19):
    """(freqs in Hz, gain in dB) of the interleaved prototype — sampled at fin * L, gain / L — on a grid of nfft / 2 + 1 points up
    to fin * L / 2."""
    proto = np.asarray(proto, dtype=np.float64)
    H = np.abs(np.fft.rfft(proto, nfft)) / L
    return np.arange(len(H)) * (fin * L / nfft), 20.0 * np.log10(np.maximum(H, 1e-30))
