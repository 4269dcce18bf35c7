"""The loudness meter on the GPU (option "loudness_meter"; elementary_amd/csrc/loudness.hip): every launch set of the host-buffer
render calls metered behind its last level, the state carried from set to set, half to half and call to call. Every comparison is
against tests/loudness_reference.py — a numpy restatement of BS.1770-4, not of the header — applied to the planar floats the SAME
calls returned, within |got - want| <= 1e-9 * want + 1e-24: both sides compute in float64, they differ in summation order and in the
hand-off of the filter state only."""
import wave

import numpy as np
import pytest

import loudness_reference as ref
from elementary_amd import el
from elementary_amd.offline import OfflineRenderer
from test_gpu_events import TOL
from test_gpu_pcm import _checker, _hip, _inputs, _ref_planar, _roots

pytestmark = pytest.mark.gpu


def _metered(sr, bs, **opts):
    return _hip(sr, bs, loudness_meter=1, **opts)


def _check(rt, planar, sr, set_frames=None, what=""):
    """The meter's read-out against the reference over `planar` [channels, frames], the whole programme so far."""
    got = rt.loudness_read()
    ms, tp, sp = ref.mean_squares(planar, sr), ref.true_peak(planar), ref.sample_peak(planar)
    assert got["channels"] == planar.shape[0] and got["frames"] == planar.shape[1] and got["hop"] == ref.hop(sr), (what, got["frames"])
    assert got["sub_blocks"] == planar.shape[1] // ref.hop(sr) and got["mean_squares"].shape == ms.shape, (what, got["sub_blocks"])
    ok, where = ref.close(got["mean_squares"], ms)
    if not ok:
        c, j = where
        print(what, "first differing (channel, sub-block, set):", c, j, None if set_frames is None else (j * got["hop"]) // set_frames,
              got["mean_squares"][c, j], ms[c, j])
    assert ok, (what, "series", where)
    ok, where = ref.close(got["true_peak"], tp)
    assert ok, (what, "true peak", where, got["true_peak"].tolist(), tp.tolist())
    assert np.array_equal(got["sample_peak"], sp), (what, got["sample_peak"].tolist(), sp.tolist())
    return got


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("bs", [128, 512])
@pytest.mark.parametrize("sr", [8000.0, 44100.0])
def test_series_and_peaks_equal_the_reference(gpu_required, sr, bs, G):
    """75 blocks + 37 frames in sets of 8 blocks: ten sets, both halves, a cut last block, sub-blocks (hop 800 / 4410) and 96-frame
    segments that straddle set boundaries; two streams of G channels delivered as s16, as f32 and as planar floats, one programme each."""
    n_out, frames = 2 * G, 75 * bs + 37
    a, c = _metered(sr, bs, batch_blocks=8), _checker(sr, bs)
    assert a.render(*_roots(n_out))["result"] == 0 and c.render(*_roots(n_out))["result"] == 0
    for k, fmt in enumerate(("s16", "f32", None)):
        x = _inputs(frames) if k == 0 else np.roll(_inputs(frames), 1000 * k, axis=1)
        a.loudness_reset()
        if fmt is None:
            planar = a.process_blocks_host(x, n_out, frames)
        else:
            _, stats, planar = a.process_blocks_pcm(x, 2, G, frames, fmt, dither_seed=5 if G == 1 else None, want_float=True)
        got = _check(a, planar, sr, 8 * bs, (sr, bs, G, fmt))
        if fmt is not None:
            assert np.array_equal(got["sample_peak"].view(np.uint32), stats["peak"].view(np.uint32))
        if k == 0:
            want = _ref_planar(c, x, n_out, bs, frames)
            assert float(np.abs(planar - want).max()) <= TOL * max(1.0, float(np.abs(want).max()))
    assert a.stats()["batch_launches"] >= 10


def test_one_call_and_three_calls_and_identical_runs(gpu_required):
    """The programme delivered as one call and — after a reset — as three calls of 9 blocks + 5 frames, 41 blocks and the rest: the
    state crosses the calls. Each is held to the reference over its own floats; a second engine doing the same returns the same bits."""
    sr, bs, n_out = 44100.0, 512, 4
    frames = 75 * bs + 37
    cuts = [0, 9 * bs + 5, 9 * bs + 5 + 41 * bs, frames]
    x = _inputs(frames)
    reads = []
    for _ in range(2):
        a = _metered(sr, bs, batch_blocks=8)
        assert a.render(*_roots(n_out))["result"] == 0
        _, _, one = a.process_blocks_pcm(x, 2, 2, frames, "s24", want_float=True)
        r1 = _check(a, one, sr, 8 * bs, "one call")
        a.loudness_reset()
        assert a.loudness_read()["frames"] == 0 and a.loudness_read()["sub_blocks"] == 0
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            parts.append(a.process_blocks_pcm(x[:, lo:hi], 2, 2, hi - lo, "s24", want_float=True)[2])
            _check(a, np.concatenate(parts, axis=1), sr, None, f"after the call that ends at {hi}")       # (a read does not disturb it)
        r3 = a.loudness_read()
        reads.append((r1, r3))
    for r_a, r_b in zip(reads[0], reads[1]):
        for key in ("mean_squares", "true_peak", "sample_peak"):
            assert r_a[key].tobytes() == r_b[key].tobytes(), key


def test_set_size_does_not_matter(gpu_required):
    sr, bs, n_out = 44100.0, 512, 2
    frames = 75 * bs + 37
    x = _inputs(frames)
    got = []
    for batch in (8, 1024):
        a = _metered(sr, bs, batch_blocks=batch)
        assert a.render(*_roots(n_out))["result"] == 0
        planar = a.process_blocks_host(x, n_out, frames)
        got.append((planar, _check(a, planar, sr, batch * bs, f"batch_blocks {batch}")))
    assert np.array_equal(got[0][0], got[1][0])
    m8, m1024 = got[0][1]["mean_squares"], got[1][1]["mean_squares"]
    assert (np.abs(m8 - m1024) <= 2 * (ref.BOUND_REL * m1024 + ref.BOUND_ABS)).all()


def test_sliced_host_block_700_s24_three_channels(gpu_required):
    """Block 700 renders as two slices of 350 frames: every other row starts 8 bytes off a 16-byte line."""
    sr, bs, G, n_out = 44100.0, 700, 3, 6
    frames = 37 * bs + 37
    a = _metered(sr, bs, batch_blocks=8)
    assert a.render(*_roots(n_out))["result"] == 0
    _, stats, planar = a.process_blocks_pcm(_inputs(frames), 2, G, frames, "s24", dither_seed=99, want_float=True)
    got = _check(a, planar, sr, 8 * 350, "block 700")
    assert np.array_equal(got["sample_peak"].view(np.uint32), stats["peak"].view(np.uint32))
    assert a.stats()["batch_launches"] >= 1


def test_host_fallback_for_taps_under_a_sliced_block(gpu_required):
    """A tap graph at host block 700 renders host block by host block through process(): the floats are on the host and go through
    the header's scalar loop — the same meter, the same state: the programme a launch-set call began goes on through it."""
    sr, bs, frames = 44100.0, 700, 9 * 700 + 211
    taps = [el.tapOut({"name": "fb"}, el.add(el.mul(1.5, el.in_({"channel": 0})), el.mul(0.5, el.tapIn({"name": "fb"})))),
            el.mul(0.9, el.in_({"channel": 1}))]
    a = _metered(sr, bs, batch_blocks=8)
    assert a.render(*_roots(2))["result"] == 0                   # no taps yet: launch sets
    x = _inputs(frames)
    p0 = a.process_blocks_host(x, 2, frames)
    _check(a, p0, sr, 8 * 350, "launch sets")
    sets = a.stats()["batch_launches"]
    assert sets >= 1
    assert a.render(*taps)["result"] == 0
    _, stats, p1 = a.process_blocks_pcm(x, 1, 2, frames, "s16", want_float=True)
    _check(a, np.concatenate([p0, p1], axis=1), sr, None, "then taps, pcm")
    p2 = a.process_blocks_host(x, 2, frames)
    _check(a, np.concatenate([p0, p1, p2], axis=1), sr, None, "then taps, floats")
    assert a.stats()["batch_launches"] == sets                   # (those two did take the block-by-block path)
    a.loudness_reset()
    _, stats, p3 = a.process_blocks_pcm(x, 1, 2, frames, "s24", want_float=True)
    got = _check(a, p3, sr, None, "taps alone")
    assert np.array_equal(got["sample_peak"].view(np.uint32), stats["peak"].view(np.uint32))


def test_pcm_input(gpu_required):
    sr, bs, n_out = 8000.0, 128, 4
    frames = 75 * bs + 37
    codes = np.round(_inputs(frames).T * 32767.0).astype(np.int16)                 # one s16 stream of two channels
    a = _metered(sr, bs, batch_blocks=8)
    assert a.render(*_roots(n_out))["result"] == 0
    _, stats, planar = a.process_blocks_pcm_io([codes], "s16", num_frames=frames, out_fmt="s16", num_streams=2, channels_per_stream=2, want_float=True)
    got = _check(a, planar, sr, 8 * bs, "s16 in, s16 out")
    assert np.array_equal(got["sample_peak"].view(np.uint32), stats["peak"].view(np.uint32))
    more = a.process_blocks_pcm_io([codes], "s16", num_outputs=n_out, num_frames=frames)
    _check(a, np.concatenate([planar, more], axis=1), sr, None, "s16 in, floats out")


def _renderer(n_out, sr, bs, meter):
    core = OfflineRenderer(lambda s, n: _hip(s, n, batch_blocks=8))
    kw = {"loudness_meter": True} if meter else {}
    core.initialize(num_input_channels=2, num_output_channels=n_out, sample_rate=sr, block_size=bs, **kw)
    core.render(*_roots(n_out))
    return core


def test_wav_files_carry_loudness_and_the_same_bytes(gpu_required, tmp_path):
    sr, bs, n_out, frames = 44100.0, 512, 4, 40 * 512 + 123
    x = _inputs(frames)
    codes = np.round(x.T * 32767.0).astype(np.int16)
    with wave.open(str(tmp_path / "in.wav"), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(int(sr)); w.writeframes(codes.tobytes())
    stats = {}
    for meter in (False, True):
        core = _renderer(n_out, sr, bs, meter)
        tag = "on" if meter else "off"
        stats["write", meter] = core.write_wav(str(tmp_path / (tag + "_w{}.wav")), list(x), frames, "s24", channels_per_stream=2, dither_seed=11, chunk_frames=7 * 512)
        if meter:
            got = core.loudness()
            assert stats["write", True]["integrated_lufs"] == got["integrated_lufs"] and stats["write", True]["true_peak_dbtp"] == got["true_peak_dbtp"]
            assert got["frames"] == frames and np.isfinite(got["integrated_lufs"]) and np.isfinite(got["true_peak_dbtp"])
            per = core.loudness(programmes=[[0, 1], [2, 3]])
            assert len(per) == 2 and max(p["true_peak_dbtp"] for p in per) == got["true_peak_dbtp"]
        if meter:
            core.loudness_reset()                                   # (the second file as a programme of its own)
        stats["wav", meter] = core.process_wav(str(tmp_path / "in.wav"), str(tmp_path / (tag + "_p{}.wav")), "s16", channels_per_stream=2, chunk_frames=9 * 512)
        if meter:
            got = core.loudness()
            assert stats["wav", True]["integrated_lufs"] == got["integrated_lufs"] and stats["wav", True]["true_peak_dbtp"] == got["true_peak_dbtp"]
            assert got["frames"] == frames
            # ... and the figures are the reference's over the floats of such a render
            twin = _renderer(n_out, sr, bs, True)
            twin.write_wav(str(tmp_path / "twin_w{}.wav"), list(x), frames, "s24", channels_per_stream=2, dither_seed=11, chunk_frames=7 * 512)
            twin.loudness_reset()
            planar = twin.process_pcm_io([codes], "s16", frames, "s16", 2, 2, want_float=True)[2]
            _check(twin.runtime, planar, sr, None, "process_wav's twin")
            want = ref.gate(ref.mean_squares(planar, sr))["integrated"]
            assert abs(got["integrated_lufs"] - want) <= 1e-7 and abs(got["true_peak_dbtp"] - ref.dbtp(ref.true_peak(planar).max())) <= 1e-7
    for kind in ("write", "wav"):
        assert set(stats[kind, False]) == {"peak", "over", "nonfinite"}
        assert set(stats[kind, True]) == {"peak", "over", "nonfinite", "integrated_lufs", "true_peak_dbtp"}
        for key in ("peak", "over", "nonfinite"):
            assert np.array_equal(stats[kind, False][key], stats[kind, True][key])
    for name in ("w0", "w1", "p0", "p1"):
        assert (tmp_path / f"on_{name}.wav").read_bytes() == (tmp_path / f"off_{name}.wav").read_bytes(), name
    with pytest.raises(RuntimeError):
        _renderer(n_out, sr, bs, False).loudness()


def test_the_option_adds_no_launch_to_the_render(gpu_required):
    """Off (never set, or set to 0) the launch counters of a render are those of an engine that never heard of the option, and on the
    render levels launch as often: the meter's kernels run behind them, not among them. The samples are the same bits in all three."""
    sr, bs, n_out, frames = 44100.0, 512, 4, 40 * 512 + 11
    x = _inputs(frames)
    keys = ("batch_launches", "spec_launches", "blocks_rendered", "graph_replays", "graph_captures", "resident_launches", "fft_launches",
            "num_levels", "num_islands")
    seen = []
    for opts in ({}, {"loudness_meter": 0}, {"loudness_meter": 1}):
        a = _hip(sr, bs, batch_blocks=8, specialize=2, **opts)      # (the commit waits for its kernels: the same launches in all three)
        assert a.render(*_roots(n_out))["result"] == 0
        streams, stats, planar = a.process_blocks_pcm(x, 2, 2, frames, "s16", dither_seed=3, want_float=True)
        host = a.process_blocks_host(x, n_out, frames)
        seen.append(({k: a.stats()[k] for k in keys}, [s.tobytes() for s in streams], planar.tobytes(), host.tobytes(), {k: v.tobytes() for k, v in stats.items()}))
        if not opts.get("loudness_meter"):
            from elementary_amd.runtime import ElemHipError
            with pytest.raises(ElemHipError):
                a.loudness_read()
    assert seen[0] == seen[1] == seen[2], [s[0] for s in seen]
    assert seen[0][0]["batch_launches"] >= 10
