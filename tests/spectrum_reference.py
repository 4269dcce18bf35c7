"""Reference and tolerance of the spectrum analyser's tests: numpy float64, a restatement of the DEFINITION (include/elemhip.h at
elemhip_spectrum_set), not of elementary_amd/csrc/spectrum.h. Frames are gathered by index with zero fill, multiplied by the window,
transformed with np.fft.rfft, |X|^2 taken, and band sums formed in float64 from the float32 weights.

Per bin:   |P - P_ref| <= 2^-23 P_ref + 2 |X_ref| d + d^2 + 2^-126,   d = K eps64 log2(S) sqrt(S) ||frame * window||_2
  2^-23 P_ref   float rounding of a correctly computed double, with one ulp of slack for ties
  d             the disagreement of two double transforms of the same frame
  2^-126        flushed float subnormals
Per band:  the |w|-weighted sum of its bins' 2 |X_ref| d + d^2, plus 2^-126, plus 2^-23 of the band value, plus
           count eps64 sum |w| P_ref (the order of the float64 sum).

K. The largest |X_twin - X_numpy| / (eps64 log2(S) sqrt(S) ||frame * window||_2) of the host emulation of the kernel
(tests/native/spectrum_host.cpp, whose powers are the twin's bits) over the inputs of tests/test_spectrum_host.py measured
K_MEASURED below, at sizes 256 .. 4096 alike; a recursive radix-2 transform in float64 measures 0.13 - 0.16 against numpy. The bound
uses four times the measured value: both sides carry independent errors of that order, and the device may contract differently. A K
far above 1 would mean a bug, not a tolerance."""
import numpy as np

EPS64 = float(np.finfo(np.float64).eps)
K_MEASURED = 0.061         # 0.039 .. 0.061 over the five sizes: test_native_emulation_prints_the_twins_bits prints it and holds it below K
K = 4.0 * K_MEASURED
SIZES = (256, 512, 1024, 2048, 4096)


def pad_of(size, center):
    return size // 2 if center else 0


def frames_complete(n, size, hop, center):
    """Frames whose last sample lies among the first n delivered."""
    p = pad_of(size, center)
    return (n + p - size) // hop + 1 if n + p >= size else 0


def frames_total(n, size, hop, center):
    """... and after a flush: centred 1 + n div hop, else the least count that covers every sample; nothing for n = 0."""
    if n == 0:
        return 0
    if center:
        return 1 + n // hop
    return -(-max(n - size, 0) // hop) + 1


def gather(x, size, hop, center, count, first=0):
    """float64 [channels, count, size]: frame first + j covers programme frames [(first + j) hop - P, ... + size), zeros outside."""
    x = np.asarray(x, dtype=np.float32)
    ch, n = x.shape
    idx = (np.arange(first, first + count)[:, None] * hop - pad_of(size, center)) + np.arange(size)[None, :]
    ok = (idx >= 0) & (idx < n)
    out = np.zeros((ch, count, size), dtype=np.float64)
    if n:
        out[:, ok] = x[:, idx[ok]].astype(np.float64)
    return out


def analyse(x, size, hop, window, bands=None, center=False, count=None, first=0):
    """(want, bound): float64 [channels, count, columns] each — the reference's columns and the tolerance around them."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[None, :]
    if count is None:
        count = frames_total(x.shape[1], size, hop, center) - first
    w = np.asarray(window, dtype=np.float64)
    fw = gather(x, size, hop, center, count, first) * w
    X = np.fft.rfft(fw, axis=-1)
    P = X.real * X.real + X.imag * X.imag
    d = K * EPS64 * np.log2(size) * np.sqrt(size) * np.sqrt((fw * fw).sum(axis=-1))[..., None]
    a = 2.0 * np.abs(X) * d + d * d                      # the bins' absolute terms
    if bands is None:
        return P, 2.0 ** -23 * P + a + 2.0 ** -126
    want = np.zeros(P.shape[:2] + (len(bands),), dtype=np.float64)
    bound = np.zeros_like(want)
    for b, (f0, wts) in enumerate(bands):
        wt = np.asarray(wts, dtype=np.float32).astype(np.float64)
        sl = slice(int(f0), int(f0) + wt.size)
        want[..., b] = (P[..., sl] * wt).sum(axis=-1)
        mag = (P[..., sl] * np.abs(wt)).sum(axis=-1)
        bound[..., b] = (a[..., sl] * np.abs(wt)).sum(axis=-1) + 2.0 ** -126 + 2.0 ** -23 * np.abs(want[..., b]) + wt.size * EPS64 * mag
    return want, bound


def close(got, want, bound):
    """(ok, where): every |got - want| <= bound, and exact zeros wherever the reference frame is silent."""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != want.shape:
        return False, ("shape", got.shape, want.shape)
    silent = (want == 0.0) & (bound <= 2.0 ** -126)      # (a silent frame, or an empty band row: nothing but the subnormal term is left)
    bad = ~(np.abs(got - want) <= bound) | (silent & (got != 0.0))
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        return False, (i, float(got[i]), float(want[i]), float(bound[i]))
    return True, None


def running_sums(frames):
    """float64 [channels, columns]: the columns of float32 `frames` [channels, n, columns] summed in frame order."""
    acc = np.zeros((frames.shape[0], frames.shape[2]), dtype=np.float64)
    for j in range(frames.shape[1]):
        acc += frames[:, j, :].astype(np.float64)
    return acc
