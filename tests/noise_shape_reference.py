"""Noise-shaped requantisation restated from its specification, independently of elementary_amd/csrc/noise_shape.h: integers per
frame (numpy int64 vectors over the channels, a Python loop over the frames), float32 only where the sample is split, the dither's
hashes from tests/pcm_reference.py."""
import math

import numpy as np

from pcm_reference import h32

F, Q, MAX_TAPS, E, SUM_MAX = 8, 11, 12, 1 << 14, 131071


def quantise_coeffs(coeffs):
    """cq_k = floor(float32(c_k) * 2048 + 0.5) in double; None for a set that is refused."""
    c = [float(np.float32(v)) for v in coeffs]
    if not 1 <= len(c) <= MAX_TAPS or not all(math.isfinite(v) for v in c):
        return None
    cq = [math.floor(v * 2048.0 + 0.5) for v in c]
    return cq if sum(abs(v) for v in cq) <= SUM_MAX else None


def dither_q8(seed, channel, t):
    """(r1 >> 24) - (r2 >> 24) for int64 times t: the two hashes of pcm_pack's dither for the key (seed, channel, t)."""
    t = np.asarray(t, dtype=np.int64)
    lo = (t & 0xffffffff).astype(np.uint32); hi = ((t >> 32) & 0xffffffff).astype(np.uint32)
    k0 = h32(np.array([(seed ^ (channel * 0x9E3779B9)) & 0xffffffff], dtype=np.uint32))
    k = h32(lo ^ h32(hi ^ k0)); r1 = h32(k); r2 = h32(k ^ np.uint32(0x85EBCA6B))
    return (r1 >> np.uint32(24)).astype(np.int64) - (r2 >> np.uint32(24)).astype(np.int64)


def split(x, bits):
    """float32 [..] -> (xi, xf): floor(x S) and the fraction in 1 / 256, 0 .. 256."""
    S = np.float32(2.0 ** (bits - 1))
    x = np.asarray(x, dtype=np.float32)
    x = np.where(np.isfinite(x), x, np.float32(0)).astype(np.float32)
    x = np.clip(x, np.float32(-2), np.float32(2)).astype(np.float32)
    w = (x * S).astype(np.float32)
    fl = np.floor(w).astype(np.float32)
    frac = (w - fl).astype(np.float32)
    xf = np.floor(((frac * np.float32(256)).astype(np.float32) + np.float32(0.5)).astype(np.float32))
    return fl.astype(np.int64), xf.astype(np.int64)


def new_state(channels):
    return {"e": np.zeros((channels, MAX_TAPS), dtype=np.int64), "saturated": np.zeros(channels, dtype=np.int64)}


def shape(coeffs, x, bits=16, seed=None, channel0=0, time0=0, state=None):
    """x float32 [channels, frames] at absolute frame time0 -> (codes int64 [channels, frames], state). `state` (new_state, or what a
    former call returned) is not modified."""
    cq = quantise_coeffs(coeffs)
    assert cq is not None
    K = len(cq)
    x = np.asarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[None, :]
    ch, n = x.shape
    S = 1 << (bits - 1)
    xi, xf = split(x, bits)
    t = time0 + np.arange(n, dtype=np.int64)
    dq = np.stack([dither_q8(seed, channel0 + c, t) for c in range(ch)]) if seed is not None else np.zeros((ch, n), dtype=np.int64)
    st = new_state(ch) if state is None else {"e": state["e"].copy(), "saturated": state["saturated"].copy()}
    e, sat = st["e"], st["saturated"]
    cqv = np.array(cq, dtype=np.int64)
    codes = np.zeros((ch, n), dtype=np.int64)
    for f in range(n):
        acc = e[:, :K] @ cqv
        assert np.all(np.abs(acc) < 2 ** 31 - 1024)
        fb = (acc + 1024) >> Q
        r = xf[:, f] + dq[:, f] - fb
        y = np.clip(xi[:, f] + ((r + 128) >> F), -S, S - 1)
        d = np.clip(y - xi[:, f], -128, 128)
        en = (d << F) - (xf[:, f] - fb)
        sat += np.abs(en) > E
        en = np.clip(en, -E, E)
        e[:, 1:] = e[:, :-1].copy()
        e[:, 0] = en
        e[:, K:] = 0
        codes[:, f] = y
    return codes, st


def state_bytes(st):
    """The reference's state as the engine lays it out: per channel int32 e[12], uint64 saturated, 8 bytes zero."""
    ch = st["e"].shape[0]
    out = np.zeros((ch, 64), dtype=np.uint8)
    out[:, :48] = st["e"].astype("<i4").view(np.uint8).reshape(ch, 48)
    out[:, 48:56] = st["saturated"].astype("<u8").view(np.uint8).reshape(ch, 8)
    return out


def pack(codes, G, fmt):
    """int codes [nOut, frames] -> the streams process_blocks_pcm returns: int16 [frames, G] or uint8 [frames, G, 3]."""
    codes = np.asarray(codes, dtype=np.int64)
    out = []
    for s in range(codes.shape[0] // G):
        a = np.ascontiguousarray(codes[s * G:(s + 1) * G].T)
        if fmt == "s16":
            out.append(a.astype(np.int16))
        else:
            out.append(np.ascontiguousarray(a.astype("<i4").view(np.uint8).reshape(a.shape[0], G, 4)[:, :, :3]))
    return out
