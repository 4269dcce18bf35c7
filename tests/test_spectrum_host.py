"""The spectrum analyser without a GPU: the scalar twin (elemhip_spectrum_host) against tests/spectrum_reference.py, band rows, the mel
helper, the kernel's phases emulated thread by thread (tests/native/spectrum_host.cpp) and validation on a dry engine handle."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import spectrum_reference as ref
from elementary_amd import spectrum as sp
from elementary_amd.runtime import ElemHipError, Runtime, spectrum_frames, spectrum_host
from test_fft_host import ROOT, _clangxx


def programme(n, channels=1, seed=1, silent=0):
    """float32 [channels, n]: noise plus two tones, peaks near 0.9; the first `silent` frames zero."""
    rng = np.random.default_rng(seed * 7919 + n)
    t = np.arange(n, dtype=np.float64)
    x = np.stack([0.25 * rng.standard_normal(n) + 0.4 * np.sin(2 * np.pi * (0.013 + 0.05 * c) * t) + 0.2 * np.sin(2 * np.pi * 0.31 * t + c)
                  for c in range(channels)]) if n else np.zeros((channels, 0))
    x = x.astype(np.float32)
    x[:, :silent] = 0.0
    return x


def band_rows(size):
    """Twelve band rows over the bins of `size`: overlapping, of odd widths, one empty, one over every bin, negative weights too."""
    bins = size // 2 + 1
    rng = np.random.default_rng(size)
    rows = [(0, np.ones(bins, dtype=np.float32)), (5, np.zeros(0, dtype=np.float32)), (bins - 1, np.array([0.5], dtype=np.float32)), (bins, np.zeros(0, dtype=np.float32))]
    for k in range(8):
        first = int(rng.integers(0, bins - 1))
        count = int(rng.integers(1, min(bins - first, 97) + 1))
        rows.append((first, (rng.standard_normal(count) if k % 2 else rng.random(count)).astype(np.float32)))
    return rows


@pytest.mark.parametrize("size", ref.SIZES)
def test_twin_equals_the_reference(size):
    """All five sizes; hops S, S / 4, 96 and 7; power and bands; centred and not; programmes of 0, 1, S / 2 - 1, S and 3 S + 37 frames
    (the longest with a silent head: exact zeros). The counts are elemhip_spectrum_frames' and the formulas'; the running sums are the
    emitted floats summed in frame order; two calls with the state handed on return the bits of one."""
    win = sp.window("hann", size)
    rows = band_rows(size)
    for hop in (size, size // 4, 96, 7):
        for n in (0, 1, size // 2 - 1, size, 3 * size + 37):
            x = programme(n, 2, seed=hop, silent=size + size // 4 if n > 3 * size else 0)
            for center in (False, True):
                total = ref.frames_total(n, size, hop, center)
                assert spectrum_frames(size, hop, center, n, True) == total and spectrum_frames(size, hop, center, n) == ref.frames_complete(n, size, hop, center)
                assert total == (0 if n == 0 else 1 + n // hop if center else -(-max(n - size, 0) // hop) + 1)
                for bands in (None, rows):
                    got, sums, state = spectrum_host(x, size, hop, win, bands, center)
                    assert state is None and got.dtype == np.float32 and got.shape == (2, total, len(rows) if bands else size // 2 + 1)
                    want, bound = ref.analyse(x, size, hop, win, bands, center)
                    ok, where = ref.close(got, want, bound)
                    assert ok, (size, hop, n, center, bands is not None, where)
                    assert sums.tobytes() == ref.running_sums(got).tobytes()
                    if n > 3 * size and bands is None:
                        assert total > 2 and not got[:, 0].any() and got[:, -1].any()
                    if n > size and hop in (96, size):
                        cut = n // 3 + 5
                        g1, _, st = spectrum_host(x[:, :cut], size, hop, win, bands, center, flush=False)
                        assert g1.shape[1] == ref.frames_complete(cut, size, hop, center) and st["delivered"] == cut
                        g2, s2, _ = spectrum_host(x[:, cut:], size, hop, win, bands, center, state=st)
                        assert np.concatenate([g1, g2], axis=1).tobytes() == got.tobytes() and s2.tobytes() == sums.tobytes()


@pytest.mark.parametrize("size", [256, 512])
def test_identity_band_rows_are_power_mode(size):
    """S / 2 + 1 rows, each one bin wide with weight 1: the bytes of power mode. An empty row gives 0."""
    x = programme(3 * size + 37, 2, seed=3)
    win = sp.window("blackman-harris", size)
    power, psums, _ = spectrum_host(x, size, size // 4, win, None, True)
    rows = [(k, np.ones(1, dtype=np.float32)) for k in range(size // 2 + 1)]
    bands, bsums, _ = spectrum_host(x, size, size // 4, win, rows, True)
    assert bands.tobytes() == power.tobytes() and bsums.tobytes() == psums.tobytes()
    got, _, _ = spectrum_host(x, size, size // 4, win, [(3, np.zeros(0, dtype=np.float32)), (0, np.ones(1, dtype=np.float32))], True)
    assert not got[:, :, 0].any() and got[:, :, 1].tobytes() == power[:, :, 0].tobytes()


def test_window_and_db_helpers():
    for size in (256, 4096):
        i = np.arange(size)
        assert np.array_equal(sp.window("hann", size), 0.5 - 0.5 * np.cos(2.0 * np.pi * i / size))
        t = i / (size - 1.0)
        bh = 0.35875 - 0.48829 * np.cos(2 * np.pi * t) + 0.14128 * np.cos(4 * np.pi * t) - 0.01168 * np.cos(6 * np.pi * t)
        assert np.abs(sp.window("blackman-harris", size) - bh).max() <= 1e-15
        assert sp.window("hann", size).dtype == np.float64 and sp.window("hann", size)[0] == 0.0
    assert sp.to_db(np.array([1.0, 10.0, 0.0])).tolist() == [0.0, 10.0, -200.0]
    with pytest.raises(ValueError):
        sp.window("kaiser", 256)


@pytest.mark.parametrize("sr,size,n,fmin,fmax", [(44100.0, 1024, 40, 0.0, None), (48000.0, 4096, 128, 20.0, 20000.0), (8000.0, 256, 64, 0.0, None),
                                                 (16000.0, 512, 80, 50.0, 7600.0)])
def test_mel_bands_are_the_formula(sr, size, n, fmin, fmax):
    """HTK mel 2595 log10(1 + f / 700), n + 2 edges equally spaced in mel, unnormalised triangles: evaluated here bin by bin in plain
    Python and compared with the rows; every row lies within the bins."""
    import math
    rows = sp.mel_bands(sr, size, n, fmin, fmax)
    assert len(rows) == n
    top = sr / 2.0 if fmax is None else fmax
    mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)
    m0, m1 = mel(fmin), mel(top)
    edges = [700.0 * (10.0 ** ((m0 + (m1 - m0) * k / (n + 1)) / 2595.0) - 1.0) for k in range(n + 2)]
    bins = size // 2 + 1
    for b, (first, w) in enumerate(rows):
        assert w.dtype == np.float32 and 0 <= first and first + w.size <= bins
        dense = np.zeros(bins)
        dense[first:first + w.size] = w
        lo, mid, hi = edges[b], edges[b + 1], edges[b + 2]
        for k in range(bins):
            f = k * sr / size
            tri = max(0.0, min((f - lo) / (mid - lo), (hi - f) / (hi - mid)))
            assert abs(dense[k] - tri) <= 1e-6, (b, k, dense[k], tri)
        if w.size:
            assert w[0] > 0 and w[-1] > 0 and w.max() <= 1.0
    with pytest.raises(ValueError):
        sp.mel_bands(sr, size, n, 100.0, sr)


def test_native_emulation_prints_the_twins_bits():
    """tests/native/spectrum_host.cpp, built with the ROCm toolchain's clang++ as test_fft_host.py builds its program: 128 emulated
    threads per frame, phase by phase, in a loop of the program's own. Its power columns are the twin's bytes. Its bins measure the
    tolerance constant: the largest |X - X_numpy| / (eps64 log2(S) sqrt(S) ||frame * window||_2) is printed and must not exceed K."""
    cxx = _clangxx()
    assert cxx, "the ROCm toolchain's clang++ builds the host emulation (ext_vector_type)"
    worst = 0.0
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "spectrum_host")
        subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "elementary_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "spectrum_host.cpp"), "-o", exe], check=True)
        for size in ref.SIZES:
            for hop, center, wname in ((size // 4, True, "hann"), (96, False, "blackman-harris")):
                n = 3 * size + 37
                x = programme(n, 1, seed=hop)
                win = sp.window(wname, size)
                fx, fw, fp, fb = (os.path.join(d, f"{size}_{hop}.{e}") for e in ("x", "w", "p", "b"))
                x[0].astype("<f4").tofile(fx)
                win.astype("<f8").tofile(fw)
                subprocess.run([exe, str(size), str(hop), "1" if center else "0", fx, fw, fp, fb], check=True, capture_output=True)
                total = ref.frames_total(n, size, hop, center)
                power = np.fromfile(fp, dtype="<f4").reshape(total, size // 2 + 1)
                bins = np.fromfile(fb, dtype="<f8").reshape(total, size // 2 + 1, 2)
                twin, _, _ = spectrum_host(x, size, hop, win, None, center)
                assert power.tobytes() == twin[0].tobytes(), (size, hop)
                frames = ref.gather(x, size, hop, center, total)[0] * win
                X = np.fft.rfft(frames, axis=-1)
                err = np.abs((bins[..., 0] + 1j * bins[..., 1]) - X).max(axis=-1)
                unit = ref.EPS64 * np.log2(size) * np.sqrt(size) * np.sqrt((frames * frames).sum(axis=-1))
                k = float((err / unit).max())
                print(f"size {size} hop {hop}: {total} frames, K measured {k:.3f}")
                worst = max(worst, k)
    print(f"largest K measured {worst:.3f} (recorded {ref.K_MEASURED}, the bound uses {ref.K})")
    assert worst <= ref.K


def test_validation_on_a_dry_handle():
    """Size 300, hop 0 and hop above the size, 513 bands and a band row past the last bin are refused with code 6 on a handle without a
    device; a good spec is accepted there, and so is turning the analyser off."""
    rt = Runtime(48000.0, 512, device=-1)
    one = np.ones(1, dtype=np.float32)
    bad = [dict(size=300, hop=64), dict(size=1024, hop=0), dict(size=1024, hop=1025), dict(size=1024, hop=256, bands=[(0, one)] * 513),
           dict(size=1024, hop=256, bands=[(512, np.ones(2, dtype=np.float32))]), dict(size=1024, hop=256, bands=[(514, np.zeros(0, dtype=np.float32))])]
    for kw in bad:
        with pytest.raises(ElemHipError) as e:
            rt.spectrum(**kw)
        assert e.value.code == 6, kw
        with pytest.raises(ElemHipError) as e:
            spectrum_host(np.zeros((1, 8), dtype=np.float32), kw["size"], kw["hop"], "hann", kw.get("bands"))
        assert e.value.code == 6, kw
    rt.spectrum(1024, 256, bands=[(0, one)] * 512)
    rt.spectrum(256, 256, bands=[(128, one), (129, np.zeros(0, dtype=np.float32))], center=True)
    rt.spectrum(None)
    assert spectrum_frames(300, 64, False, 1000) == 0
