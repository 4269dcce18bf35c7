"""The spectrum analyser on the GPU (Runtime.spectrum; elementary_amd/csrc/spectrum.hip): every launch set of the host-buffer render
calls framed, windowed and transformed behind its last level, the overlap carried from set to set, half to half and call to call.
Every comparison is against tests/spectrum_reference.py — numpy float64, a restatement of the definition, not of the header — applied
to the planar floats the SAME calls returned, within the bound that file derives."""
import numpy as np
import pytest

import spectrum_reference as ref
from elementary_amd import el
from elementary_amd import spectrum as sp
from elementary_amd.runtime import ElemHipError, spectrum_launches
from test_gpu_noise_shape import _roots as _gain_roots
from test_gpu_pcm import _hip, _inputs, _roots

pytestmark = pytest.mark.gpu

SR = 44100.0


def _check(rt, planar, size, hop, window, bands=None, center=False, flush=True, what="", before=None):
    """Reads (after a flush, if asked) and holds everything emitted so far — `before` (the frames of earlier reads) included — to the
    reference over `planar` [channels, frames], the whole programme so far. Returns the read-out with all frames in front."""
    if flush:
        rt.spectrum_flush()
    got = rt.spectrum_read()
    n = planar.shape[1]
    count = ref.frames_total(n, size, hop, center) if flush else ref.frames_complete(n, size, hop, center)
    have = 0 if before is None else before.shape[1]
    assert got["first_frame"] == have and got["frames_total"] == count and got["delivered"] == n and got["flushed"] == flush, \
        (what, got["first_frame"], got["frames_total"], count, got["delivered"])
    frames = got["frames"] if before is None else np.concatenate([before, got["frames"]], axis=1)
    want, bound = ref.analyse(planar, size, hop, window, bands, center, count=count)
    ok, where = ref.close(frames, want, bound)
    if not ok:
        print(what, "first miss (channel, frame, column), got, want, bound:", where)
    assert ok, (what, where)
    assert got["sums"].tobytes() == ref.running_sums(frames).tobytes(), what
    got["frames"] = frames
    return got


@pytest.mark.parametrize("size", ref.SIZES)
@pytest.mark.parametrize("bs", [64, 512])
def test_sizes_blocks_and_hops(gpu_required, bs, size):
    """75 blocks + 37 frames in sets of 8 blocks: ten sets, both halves, a cut last block. Hop S / 4, and 96 at S = 256; 2 channels as
    planar floats and 3 as one s16 stream; power mode, and 40 mel bands at S = 1024. At block 64 a set is 512 frames: a frame of 4096
    spans nine sets and the carried tail is longer than what a set adds."""
    frames = 75 * bs + 37
    x = _inputs(frames)
    cases = [(size // 4, None)] + ([(96, None)] if size == 256 else []) + ([(256, sp.mel_bands(SR, 1024, 40))] if size == 1024 else [])
    for n_out in (2, 3):
        a = _hip(SR, bs, batch_blocks=8)
        assert a.render(*_roots(n_out))["result"] == 0
        a.process_blocks_host(x[:, :32 * bs], n_out, 32 * bs)          # (the root fades settle: launch sets from here on)
        for hop, bands in cases:
            win = sp.window("hann", size)
            a.spectrum(size, hop, win, bands)
            sets = a.stats()["batch_launches"]
            if n_out == 2:
                planar = a.process_blocks_host(x, n_out, frames)
            else:
                planar = a.process_blocks_pcm(x, 1, 3, frames, "s16", dither_seed=5, want_float=True)[2]
            part = _check(a, planar, size, hop, win, bands, flush=False, what=(bs, size, hop, n_out, "complete"))
            _check(a, planar, size, hop, win, bands, flush=True, what=(bs, size, hop, n_out, "flushed"), before=part["frames"])
            assert a.stats()["batch_launches"] - sets >= 10            # (at block 64 and S = 4096: a frame spans nine of them)


def test_the_cut_into_calls_and_sets_changes_no_bit(gpu_required):
    """One call; after a reset three calls of 9 blocks + 5 frames, 41 blocks and the rest, with a read between them; once more in sets
    of 1024 blocks; and a second engine: the same bytes, frames and running sums. (A graph of gains: the floats do not depend on the cut.)"""
    bs, n_out, size, hop = 512, 3, 2048, 96
    frames = 75 * bs + 37
    cuts = [0, 9 * bs + 5, 9 * bs + 5 + 41 * bs, frames]
    x = _inputs(frames)
    win = sp.window("blackman-harris", size)
    seen = []
    for batch in (8, 8, 1024):
        a = _hip(SR, bs, batch_blocks=batch)
        assert a.render(*_gain_roots(n_out))["result"] == 0
        a.process_blocks_host(x[:, :8 * bs], n_out, 8 * bs)            # (the root fades settle: from here on the floats are gain * input)
        a.spectrum(size, hop, win, center=True)
        one = a.process_blocks_host(x, n_out, frames)
        r1 = _check(a, one, size, hop, win, None, True, flush=False, what=("one call", batch))
        a.spectrum_reset()
        empty = a.spectrum_read()
        assert empty["delivered"] == 0 and empty["frames_total"] == 0 and empty["frames"].shape[1] == 0 and not empty["sums"].any()
        parts, part = [], None
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            parts.append(a.process_blocks_host(x[:, lo:hi], n_out, hi - lo))
            part = _check(a, np.concatenate(parts, axis=1), size, hop, win, None, True, flush=False, what=("call ending at", hi, batch),
                          before=None if part is None else part["frames"])            # (a read does not disturb the programme)
        assert np.concatenate(parts, axis=1).tobytes() == one.tobytes()
        r3 = _check(a, one, size, hop, win, None, True, flush=True, what=("three calls, flushed", batch), before=part["frames"])
        assert r3["frames"][:, :r1["frames"].shape[1]].tobytes() == r1["frames"].tobytes()
        seen.append((r1["frames"].tobytes(), r1["sums"].tobytes(), r3["frames"].tobytes(), r3["sums"].tobytes()))
    assert seen[0] == seen[1] == seen[2]


def test_centred_with_flush(gpu_required):
    """A centred programme whose length is no multiple of the hop, then — the call after a flush starts at frame 0 — one shorter than
    S / 2, then an empty flush."""
    bs, n_out, size, hop = 64, 2, 1024, 200
    win = sp.window("hann", size)
    a = _hip(SR, bs, batch_blocks=8)
    assert a.render(*_roots(n_out))["result"] == 0
    a.spectrum(size, hop, win, center=True)
    for frames in (31 * bs + 17, 300, 1):
        assert frames % hop != 0
        planar = a.process_blocks_host(_inputs(frames), n_out, frames)
        got = _check(a, planar, size, hop, win, None, True, flush=True, what=("centred", frames))
        assert got["frames"].shape[1] == 1 + frames // hop
    a.spectrum_reset()
    a.spectrum_flush()
    assert a.spectrum_read()["frames"].shape[1] == 0


def test_behind_the_converter_and_the_limiter_and_before_the_quantiser(gpu_required):
    """resample_rate 48000 from 44100, the limiter on, s16 delivery with second-order noise shaping: the spectrum is that of the floats
    the call returns — latencies included, quantisation not — and the PCM bytes are those of an engine without the analyser."""
    from elementary_amd.noise_shape import PRESETS
    bs, n_out, size, hop = 350, 4, 512, 128
    win = sp.window("hann", size)
    bands = sp.mel_bands(48000.0, size, 24)
    out = []
    for on in (True, False):
        a = _hip(SR, bs, batch_blocks=3, resample_rate=48000, limiter_gain_db=6.0, limiter=1)
        assert a.render(*_roots(n_out))["result"] == 0
        a.noise_shape(PRESETS["second"])
        if on:
            a.spectrum(size, hop, win, bands)
        streams, planars = [], []
        for frames in (17 * bs + 99, 700):
            s, _, p = a.process_blocks_pcm(_inputs(frames), 2, 2, frames, "s16", dither_seed=7, want_float=True)
            assert p.shape[1] == s[0].shape[0] != frames
            streams.append([np.ascontiguousarray(v).tobytes() for v in s]); planars.append(p)
        if on:
            _check(a, np.concatenate(planars, axis=1), size, hop, win, bands, flush=True, what="converter, limiter, shaped s16")
        out.append((streams, [p.tobytes() for p in planars]))
    assert out[0] == out[1]


def test_the_tap_slice_path(gpu_required):
    """Block 700 renders as two slices of 350 frames; a tap graph there goes host block by host block through the scalar twin, on the
    same carried state: the programme a launch-set call began goes on through it, and back."""
    bs, size, hop, frames = 700, 1024, 256, 9 * 700 + 211
    win = sp.window("hann", size)
    taps = [el.tapOut({"name": "fb"}, el.add(el.mul(1.5, el.in_({"channel": 0})), el.mul(0.5, el.tapIn({"name": "fb"})))),
            el.mul(0.9, el.in_({"channel": 1}))]
    a = _hip(SR, bs, batch_blocks=8)
    assert a.render(*_roots(2))["result"] == 0                   # no taps yet: launch sets
    a.spectrum(size, hop, win)
    x = _inputs(frames)
    p0 = a.process_blocks_host(x, 2, frames)
    part = _check(a, p0, size, hop, win, flush=False, what="launch sets")
    sets, launched = a.stats()["batch_launches"], spectrum_launches()
    assert sets >= 1
    assert a.render(*taps)["result"] == 0
    p1 = a.process_blocks_pcm(x, 1, 2, frames, "s16", want_float=True)[2]
    part = _check(a, np.concatenate([p0, p1], axis=1), size, hop, win, flush=False, what="then taps", before=part["frames"])
    assert a.stats()["batch_launches"] == sets and spectrum_launches() == launched       # (the block-by-block path, the twin)
    assert a.render(*_roots(2))["result"] == 0
    p2 = a.process_blocks_host(x, 2, frames)
    _check(a, np.concatenate([p0, p1, p2], axis=1), size, hop, win, flush=True, what="then launch sets again", before=part["frames"])
    assert spectrum_launches() > launched


def test_off_adds_nothing(gpu_required):
    """An engine never given a spec, and one whose analyser was turned off again: spectrum_read raises, the launch counters of a render
    are those of an engine with the analyser on (its kernels run behind the levels, not among them), no analyser kernel is launched,
    and the samples are the same bits in all three."""
    bs, n_out, frames = 512, 4, 40 * 512 + 11
    x = _inputs(frames)
    keys = ("batch_launches", "spec_launches", "blocks_rendered", "graph_replays", "graph_captures", "resident_launches", "fft_launches",
            "num_levels", "num_islands")
    seen = []
    for mode in ("never", "off again", "on"):
        a = _hip(SR, bs, batch_blocks=8, specialize=2)
        assert a.render(*_roots(n_out))["result"] == 0
        if mode != "never":
            a.spectrum(1024, 256)
        if mode == "off again":
            a.spectrum(None)
        before = spectrum_launches()
        streams, stats, planar = a.process_blocks_pcm(x, 2, 2, frames, "s16", dither_seed=3, want_float=True)
        host = a.process_blocks_host(x, n_out, frames)
        seen.append(({k: a.stats()[k] for k in keys}, [s.tobytes() for s in streams], planar.tobytes(), host.tobytes(), {k: v.tobytes() for k, v in stats.items()}))
        if mode == "on":
            assert spectrum_launches() > before
        else:
            assert spectrum_launches() == before
            with pytest.raises(ElemHipError):
                a.spectrum_read()
            with pytest.raises(ElemHipError):
                a.spectrum_flush()
    assert seen[0] == seen[1] == seen[2], [s[0] for s in seen]
    assert seen[0][0]["batch_launches"] >= 10


def test_offline_renderer_spectrogram(gpu_required):
    from elementary_amd.offline import OfflineRenderer
    bs, n_out, frames = 512, 2, 20 * 512 + 123
    core = OfflineRenderer(lambda s, n: _hip(s, n, batch_blocks=8))
    core.initialize(num_input_channels=2, num_output_channels=n_out, sample_rate=SR, block_size=bs, spectrum={"size": 1024, "hop": 256, "mel": 40, "center": True})
    core.render(*_roots(n_out))
    x = _inputs(frames)
    streams, _, planar = core.process_pcm(list(x), 1, 2, frames, "s16", want_float=True)
    first = core.spectrogram()
    got = core.spectrogram(flush=True)
    want, bound = ref.analyse(planar, 1024, 256, sp.window("hann", 1024), sp.mel_bands(SR, 1024, 40), True)
    assert got["frames"][:, :first["frames"].shape[1]].tobytes() == first["frames"].tobytes()
    ok, where = ref.close(got["frames"], want, bound)
    assert ok, where
    assert np.isfinite(sp.to_db(got["sums"] / got["frames_total"])).all()
    plain = OfflineRenderer(lambda s, n: _hip(s, n, batch_blocks=8))
    plain.initialize(num_input_channels=2, num_output_channels=n_out, sample_rate=SR, block_size=bs)
    with pytest.raises(RuntimeError):
        plain.spectrogram()
