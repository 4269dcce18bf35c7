"""The resource loader's semantics in numpy and float64, written from the specification (a source of G interleaved channels at one
rate becomes planar rows at the engine's rate), not from elementary_amd/csrc/resource_load.h.

Same rate: row g, frame f = the decoded sample (f, g). Other rate: g = gcd(fin, fout), L = fout / g, M = fin / g, s = min(1, L / M),
W = 32 / s, Wc = ceil(W), T = 2 Wc; the prototype g(t) = s sinc(s t) I0(beta sqrt(1 - (t / W)^2)) / I0(beta) for |t| < W, beta = 0.1102
(100 - 8.7); resource frame n, 0 <= n < ceil(N L / M): a = n M, i0 = floor(a / L), p = a - i0 L, y[n] = sum_k g(p / L + Wc - 1 - k)
x[i0 - Wc + 1 + k] with x = 0 outside the file. ``bound`` is the float32 evaluation's error bound per output, (T + 1) 2^-24 sum_k
|h_k| |x_k|: T roundings of the fused multiply-add chain and one of each coefficient."""
import math

import numpy as np

import pcm_unpack_reference as uref


def plan(fin, fout):
    g = math.gcd(int(fin), int(fout))
    L, M = int(fout) // g, int(fin) // g
    Wc = 32 if L >= M else -(-32 * M // L)
    return {"L": L, "M": M, "Wc": Wc, "T": 2 * Wc}


def prototype(t, L, M):
    t = np.asarray(t, dtype=np.float64)
    s = 1.0 if L >= M else L / M
    W = 32.0 / s
    beta = 0.1102 * (100.0 - 8.7)
    inside = np.abs(t) < W
    u = np.where(inside, t / W, 0.0)
    return np.where(inside, s * np.sinc(s * t) * np.i0(beta * np.sqrt(1.0 - u * u)) / np.i0(beta), 0.0)


def out_frames(n, fin, fout):
    p = plan(fin, fout)
    return -(-n * p["L"] // p["M"])


def decode(stream, fmt):
    """One stream in the layout ``add_shared_resource_pcm`` takes -> float32 ``[G, frames]``."""
    return np.ascontiguousarray(uref.decode_stream(stream, fmt).T)


def convert(x, fin, fout):
    """``x`` float ``[G, N]`` at ``fin`` -> ``(y, bound)``, float64 ``[G, ceil(N L / M)]`` each."""
    x = np.asarray(x, dtype=np.float64)
    G, N = x.shape
    p = plan(fin, fout)
    L, M, Wc, T = p["L"], p["M"], p["Wc"], p["T"]
    n_out = -(-N * L // M)
    y, bound = np.zeros((G, n_out)), np.zeros((G, n_out))
    k = np.arange(T)
    for n in range(n_out):
        a = n * M
        i0 = a // L
        ph = a - i0 * L
        h = prototype(ph / L + Wc - 1.0 - k, L, M)
        idx = i0 - Wc + 1 + k
        ok = (idx >= 0) & (idx < N)
        xs = x[:, idx[ok]]
        y[:, n] = xs @ h[ok]
        bound[:, n] = (T + 1) * 2.0 ** -24 * (np.abs(xs) @ np.abs(h[ok]))
    return y, bound
