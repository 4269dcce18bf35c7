"""The true-peak limiter on the GPU (options "limiter", "limiter_*"; elementary_amd/csrc/limiter.hip): every launch set of the
host-buffer render calls limited behind the converter, the carried state crossing sets, halves and calls. The yardstick is
tests/limiter_reference.py — a float64 numpy restatement of the formulas, not of the header — applied to the floats a TWIN engine
without the option rendered from the same input, within one float32 ulp; the packed streams against tests/pcm_reference.py over the
limited floats; bit-for-bit claims against the header's scalar loop compiled for the host (tests/native/limiter_host.cpp)."""
import numpy as np
import pytest

import limiter_reference as ref
import loudness_reference as lref
import resample_reference as rref
from elementary_amd import el
from elementary_amd.offline import OfflineRenderer
from elementary_amd.runtime import ElemHipError
from test_gpu_loudness import _check as _check_meter
from test_gpu_pcm import _check_call, _hip, _inputs, _roots
from test_limiter_host import host_loop

pytestmark = pytest.mark.gpu

RATE = 12000.0
CEILING = np.float32(10.0 ** (-1.0 / 20.0))


def _params(D, link=0, rate=RATE, **more):
    return dict(ceiling_dbtp=-1.0, release_ms=50.0, lookahead_ms=D * 1000.0 / rate, link=link, **more)


def _limited(rate, bs, params, **opts):
    """An engine with the limiter on (the parameters first, then the switch)."""
    rt = _hip(float(rate), bs, **opts)
    for k, v in params.items():
        rt.set_option("limiter_" + k, v)
    rt.set_option("limiter", 1)
    return rt


def _through(n):
    return [el.in_({"channel": c}) for c in range(n)]


def _pair(rate, bs, params, roots, **opts):
    """(the engine with the limiter, its twin without), the same graph rendered on both."""
    a, twin = _limited(rate, bs, params, **opts), _hip(float(rate), bs, **opts)
    assert a.render(*roots)["result"] == 0 and twin.render(*roots)["result"] == 0
    return a, twin


_REFS = {}


def _reference(floats, rate, params):
    key = (floats.tobytes(), floats.shape, rate, tuple(sorted(params.items())))
    if key not in _REFS:
        _REFS[key] = ref.limit(floats, rate, **params)
    return _REFS[key]


def _within(got, floats, rate, params, what):
    """`got` against the reference over the twin's `floats`: one float32 ulp; the sample peak under the ceiling; where the
    reference's gain is exactly 1 (and the static gain 0 dB) the twin's bits, delayed by the latency."""
    want, g, stats = _reference(floats, rate, params)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = ref.within(got, want)
    err = np.abs(got.astype(np.float64) - want)
    fin = np.isfinite(want)
    print(what, "frames", got.shape[1], "limited share", (g < 1.0).mean(axis=1).tolist(), "idle share", (g == 1.0).mean(axis=1).tolist(),
          "worst error / ulp", float((err[fin] / np.spacing(np.abs(want[fin]).astype(np.float32))).max()))
    assert ok.all(), (what, int((~ok).sum()), np.argwhere(~ok)[:4].tolist())
    ceiling = np.float32(10.0 ** (params["ceiling_dbtp"] / 20.0))
    assert float(np.abs(got[np.isfinite(got)]).max()) <= ceiling + np.spacing(ceiling), what
    if params.get("gain_db", 0.0) == 0.0:
        lat = ref.plan(rate, **params)["latency"]
        delayed = np.concatenate([np.zeros((floats.shape[0], lat), dtype=np.float32), floats], axis=1)[:, :floats.shape[1]]
        width = params["link"] or floats.shape[0]
        idle = np.repeat(g == 1.0, width, axis=0)
        assert np.array_equal(got.view(np.uint32)[idle], delayed.view(np.uint32)[idle]), what
    return want, g, stats


def _check_read(rt, stats, frames, params, rate=RATE):
    got = rt.limiter_read()
    pl = ref.plan(rate, **params)
    assert (got["lookahead_frames"], got["latency_frames"], got["release_frames"], got["link"]) == (pl["D"], pl["D"] + 6, pl["R"], pl["link"])
    assert got["groups"] == len(stats["max_reduction"]) and got["frames"] == frames
    ref.check_stats(got["max_reduction"], got["limited_frames"], stats)
    return got


@pytest.mark.parametrize("link", [0, 1])
@pytest.mark.parametrize("D", [1, 66, 300])
@pytest.mark.parametrize("bs", [128, 512])
def test_floats_and_streams_equal_the_reference(gpu_required, bs, D, link):
    """20 blocks + 37 frames in sets of 8 blocks: three sets, both halves, a cut last block, a latency that crosses set boundaries (306
    frames against blocks of 128); planar floats, f32, and s16 with dither — a programme each. Neither branch goes untested: the
    reference limits between half and 0.95 of the frames and leaves at least 0.05 of them alone."""
    params, frames = _params(D, link), 20 * bs + 37
    a, twin = _pair(RATE, bs, params, _through(2), batch_blocks=8)
    x = ref.signal(bs)
    assert x.shape == (2, frames)
    for fmt in (None, "f32", "s16"):
        a.limiter_reset()
        floats = twin.process_blocks_host(x, 2, frames)
        if fmt is None:
            planar = a.process_blocks_host(x, 2, frames)
        else:
            seed = 5 if fmt == "s16" else None
            streams, stats, planar = a.process_blocks_pcm(x, 1, 2, frames, fmt, dither_seed=seed, want_float=True, sample_time=0)
            _check_call(streams, stats, planar, 2, fmt, seed, 0)
            assert int(stats["over"].sum()) == 0
        want, g, st = _within(planar, floats, RATE, params, (bs, D, link, fmt))
        assert ((g < 1.0).mean(axis=1) >= 0.5).all() and ((g < 1.0).mean(axis=1) <= 0.95).all() and ((g == 1.0).mean(axis=1) >= 0.05).all()
        _check_read(a, st, frames, params)
    assert a.stats()["batch_launches"] >= 3


def test_cuts_set_sizes_and_engines_leave_the_same_bits(gpu_required):
    """One call against three calls (9 blocks + 5 frames, 41 blocks, the rest), launch sets of 8 blocks against one set, a second
    engine, and the programme once more after a reset: the same bytes, packed and planar, and the same statistics."""
    bs, D = 128, 66
    params = _params(D, 1)
    frames = 60 * bs + 37
    cuts = [0, 9 * bs + 5, 9 * bs + 5 + 41 * bs, frames]
    x = np.tile(ref.signal(bs), (1, 3))[:, :frames]

    def read(rt):
        got = rt.limiter_read()
        return got["frames"], got["max_reduction"].tobytes(), got["limited_frames"].tobytes()

    def one(rt):
        streams, _, planar = rt.process_blocks_pcm(x, 1, 2, frames, "s24", dither_seed=21, want_float=True, sample_time=0)
        return [s.tobytes() for s in streams], planar.tobytes(), read(rt)

    def three(rt):
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            parts.append(rt.process_blocks_pcm(x[:, lo:hi], 1, 2, hi - lo, "s24", dither_seed=21, want_float=True, sample_time=lo))
            assert rt.limiter_read()["frames"] == hi
        return [np.concatenate([p[0][0] for p in parts]).tobytes()], np.concatenate([p[2] for p in parts], axis=1).tobytes(), read(rt)

    seen = []
    for batch in (8, 1024, 8):
        rt = _limited(RATE, bs, params, batch_blocks=batch)
        assert rt.render(*_through(2))["result"] == 0
        rt.process_blocks_host(x[:, :40 * bs], 2, 40 * bs)                 # (the roots' fade-in: 20 ms)
        rt.limiter_reset()
        assert rt.limiter_read()["frames"] == 0 and rt.limiter_read()["groups"] == 0
        seen.append(one(rt))
        rt.limiter_reset()
        seen.append(three(rt))
        rt.limiter_reset()
        seen.append(one(rt))                                               # the programme repeats
    for other in seen[1:]:
        assert other == seen[0]
    planar = np.frombuffer(seen[0][1], dtype=np.float32).reshape(2, -1)
    _, _, st = _within(planar, x, RATE, params, "cuts")
    assert st["limited_frames"].min() > 1000


def test_host_loop_for_taps_under_a_sliced_block_continues_the_programme(gpu_required, tmp_path):
    """A tap graph at host block 700 (two slices of 350) renders host block by host block through process(): the floats are on the
    host and go through the header's scalar loop with the carried state brought over for the call. A programme begun by launch sets
    goes on through it, and back: the bits and the statistics are limiter_host() over the twin's concatenated floats."""
    bs, frames, D = 700, 9 * 700 + 211, 66
    params = _params(D, 0)
    taps = [el.tapOut({"name": "fb"}, el.add(el.mul(0.8, el.in_({"channel": 0})), el.mul(0.3, el.tapIn({"name": "fb"})))), el.in_({"channel": 1})]
    a, twin = _pair(RATE, bs, params, _through(2), batch_blocks=8)
    x = np.tile(ref.signal(512), (1, 2))[:, :frames]
    f0, p0 = twin.process_blocks_host(x, 2, frames), a.process_blocks_host(x, 2, frames)
    sets = a.stats()["batch_launches"]
    assert sets >= 1
    assert a.render(*taps)["result"] == 0 and twin.render(*taps)["result"] == 0
    f1 = twin.process_blocks_host(x, 2, frames)
    streams, stats, p1 = a.process_blocks_pcm(x, 1, 2, frames, "s24", dither_seed=4, want_float=True, sample_time=frames)
    _check_call(streams, stats, p1, 2, "s24", 4, frames)
    f2, p2 = twin.process_blocks_host(x, 2, frames), a.process_blocks_host(x, 2, frames)
    assert a.stats()["batch_launches"] == sets                   # (those two did take the block-by-block path)
    assert a.render(*_through(2))["result"] == 0 and twin.render(*_through(2))["result"] == 0
    f3, p3 = twin.process_blocks_host(x, 2, frames), a.process_blocks_host(x, 2, frames)
    floats, got = np.concatenate([f0, f1, f2, f3], axis=1), np.concatenate([p0, p1, p2, p3], axis=1)
    want, st = host_loop(tmp_path, floats, RATE, **params)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    read = a.limiter_read()
    assert read["frames"] == 4 * frames and read["max_reduction"].tolist() == st["max_reduction"] and read["limited_frames"].tolist() == st["limited_frames"]
    _within(got, floats, RATE, params, "launch sets, taps, taps, launch sets")


def test_behind_the_converter_and_in_front_of_the_meter(gpu_required):
    """48000 -> 44100 at block size 128: the result is the reference over the twin's CONVERTED floats at the delivery rate (D = 66
    frames of 44100), and the meter reads what the loudness reference reads over the limited floats — it meters what is delivered, so
    its true peak is the limited output's, whatever that is."""
    fin, fout, bs, frames = 48000, 44100, 128, 60 * 128 + 37
    params = dict(ceiling_dbtp=-1.0, release_ms=50.0, lookahead_ms=1.5, link=0)
    a = _limited(fin, bs, params, batch_blocks=8, resample_rate=fout, loudness_meter=1)
    twin = _hip(float(fin), bs, batch_blocks=8, resample_rate=fout)
    assert a.render(*_through(2))["result"] == 0 and twin.render(*_through(2))["result"] == 0
    x = np.tile(ref.signal(128, fin), (1, 4))[:, :frames]
    floats = twin.process_blocks_host(x, 2, frames)
    assert floats.shape[1] == rref.frames_out(frames, rref.plan(fin, fout))
    streams, stats, planar = a.process_blocks_pcm(x, 1, 2, frames, "s16", dither_seed=9, want_float=True)
    _check_call(streams, stats, planar, 2, "s16", 9, 0)                      # (output-frame time: the programme began with the option)
    want, g, st = _within(planar, floats, float(fout), params, "converted")
    assert (g < 1.0).mean() > 0.2 and (g == 1.0).mean() > 0.02
    got = _check_read(a, st, floats.shape[1], params, float(fout))
    assert got["lookahead_frames"] == 66
    meter = _check_meter(a, planar, float(fout), None, "limited")
    print("metered true peak of the output, dBTP:", [lref.dbtp(float(v)) for v in meter["true_peak"]])
    # whichever option is set first
    b = _hip(float(fin), bs, batch_blocks=8, loudness_meter=1)
    for k, v in params.items():
        b.set_option("limiter_" + k, v)
    b.set_option("limiter", 1)
    b.set_option("resample_rate", fout)
    assert b.render(*_through(2))["result"] == 0
    assert b.limiter_read()["lookahead_frames"] == 66
    again = b.process_blocks_host(x, 2, frames)
    assert np.array_equal(again.view(np.uint32), planar.view(np.uint32))


def test_nonfinite_samples_pass_and_detect_as_silence(gpu_required):
    """A NaN and an inf reach the pack kernel's count, delayed by the latency, and leave every other frame's gain as it was: the
    other frames are those of the same programme with zeros in their place."""
    bs, D, frames = 128, 18, 12 * 128 + 37
    params = _params(D, 0)
    a, twin = _pair(RATE, bs, params, _through(2), batch_blocks=8)
    x = ref.signal(128)[:, :frames].copy()
    for rt in (a, twin):
        rt.process_blocks_host(x[:, :4 * bs], 2, 4 * bs)                   # (the roots' fade-in: 20 ms)
    a.limiter_reset()
    clean = x.copy()
    x[0, 700], x[1, 900] = np.nan, np.inf
    clean[0, 700] = clean[1, 900] = 0.0
    streams, stats, planar = a.process_blocks_pcm(x, 1, 2, frames, "s16", want_float=True, sample_time=0)
    assert stats["nonfinite"].tolist() == [1, 1]
    lat = D + 6
    assert np.isnan(planar[0, 700 + lat]) and np.isinf(planar[1, 900 + lat])
    a.limiter_reset()
    other = a.process_blocks_host(clean, 2, frames)
    keep = np.ones(planar.shape, dtype=bool)
    keep[0, 700 + lat] = keep[1, 900 + lat] = False
    differ = (planar.view(np.uint32) != other.view(np.uint32)) & keep
    assert not differ.any(), (int(differ.sum()), np.argwhere(differ)[:6].tolist(), planar[differ][:6].tolist(), other[differ][:6].tolist())
    _within(other, twin.process_blocks_host(clean, 2, frames), RATE, params, "zeros in their place")


def _renderer(n, fin, bs, fout, params, meter=False):
    core = OfflineRenderer(lambda s, k: _hip(s, k, batch_blocks=8))
    kw = {} if fout is None else {"output_sample_rate": fout}
    core.initialize(num_input_channels=n, num_output_channels=n, sample_rate=fin, block_size=bs, limiter=params, loudness_meter=meter, **kw)
    core.render(*_through(n))
    return core


def _read_wav(path):
    from elementary_amd.wav import WavReader
    with WavReader(str(path)) as r:
        return r.sample_rate, r.read(r.frames)


@pytest.mark.parametrize("fout", [None, 44100])
def test_wav_files_have_the_latency_taken_out(gpu_required, tmp_path, fout):
    """write_wav / process_wav: frame n of the file is the limited render at n — output n + Do + D + 6 of the plain call — with and
    without the converter; the bytes do not depend on chunk_frames; the statistics carry the limiter's deepest reduction."""
    from elementary_amd.wav import WavWriter
    fin, bs, frames = 48000, 512, 14 * 512 + 123
    params = dict(ceiling_dbtp=-1.0, release_ms=50.0, lookahead_ms=1.5, link=0)
    x = np.tile(ref.signal(128, fin), (1, 3))[:, :frames]
    w = WavWriter(str(tmp_path / "in.wav"), "f32", 2, fin)
    w.write(np.ascontiguousarray(x.T))
    w.close()
    files = {}
    for chunk in (5 * 512, 1 << 20):
        core = _renderer(2, fin, bs, fout, params)
        st_w = core.write_wav(str(tmp_path / f"w{chunk}.wav"), list(x), frames, "s24", dither_seed=11, chunk_frames=chunk)
        st_p = core.process_wav(str(tmp_path / "in.wav"), str(tmp_path / f"p{chunk}.wav"), "f32", chunk_frames=chunk)
        assert set(st_w) == set(st_p) == {"peak", "over", "nonfinite", "limiter_max_reduction_db"}
        assert st_w["limiter_max_reduction_db"] > 3.0 and st_p["limiter_max_reduction_db"] > 3.0
        for name in ("w", "p"):
            files[name, chunk] = (tmp_path / f"{name}{chunk}.wav").read_bytes()
    for name in ("w", "p"):
        assert files[name, 5 * 512] == files[name, 1 << 20], name
    up, down, Do = 1, 1, 0
    if fout is not None:
        pl = rref.plan(fin, fout)
        up, down, Do = pl["L"], pl["M"], pl["Do"]
    lat = Do + ref.plan(float(fout or fin), **params)["latency"]
    keep, extra = -((-frames * up) // down), -((-lat * down) // up)
    plain = _limited(fin, bs, params, batch_blocks=8, **({} if fout is None else {"resample_rate": fout}))
    assert plain.render(*_through(2))["result"] == 0
    xp = np.concatenate([x, np.zeros((2, extra), dtype=np.float32)], axis=1)
    streams_w, _, _ = plain.process_blocks_pcm(xp, 1, 2, frames + extra, "s24", dither_seed=11, sample_time=0)
    assert st_w["limiter_max_reduction_db"] == -20.0 * float(np.log10(1.0 - plain.limiter_read()["max_reduction"].max()))
    plain.limiter_reset()
    if fout is not None:
        plain.resample_reset()
    streams_p, _, _ = plain.process_blocks_pcm(xp, 1, 2, frames + extra, "f32", sample_time=0)
    assert st_p["limiter_max_reduction_db"] == -20.0 * float(np.log10(1.0 - plain.limiter_read()["max_reduction"].max()))
    rate, got = _read_wav(tmp_path / f"w{1 << 20}.wav")
    assert rate == (fout or fin) and got.shape[0] == keep and np.array_equal(got, streams_w[0][lat:lat + keep])
    rate, got = _read_wav(tmp_path / f"p{1 << 20}.wav")
    assert rate == (fout or fin) and got.shape[0] == keep and np.array_equal(got.view(np.uint32), streams_p[0][lat:lat + keep].view(np.uint32))
    with pytest.raises(RuntimeError):
        OfflineRenderer(lambda s, k: _hip(s, k)).limiter()


def _tone_file(path, amp, seconds=3.0, rate=48000):
    from elementary_amd.wav import WavWriter
    n = int(seconds * rate)
    t = np.arange(n)
    env = np.clip(np.minimum(t, n - 1 - t) / (0.25 * rate), 0.0, 1.0)           # silence-to-level fades of 250 ms at either end
    x = np.stack([amp * env * np.sin(2.0 * np.pi * 1000.0 * t / rate), 0.8 * amp * env * np.sin(2.0 * np.pi * 440.0 * t / rate + 1.0)]).astype(np.float32)
    w = WavWriter(str(path), "f32", 2, rate)
    w.write(np.ascontiguousarray(x.T))
    w.close()
    return x


def test_master_wav_reaches_the_target_where_the_limiter_is_idle(gpu_required, tmp_path):
    """A 3 s programme that stays under the ceiling after the gain: the output's integrated loudness is the target within 1e-5 LU
    (float rounding of the outputs moves a level by at most 20 log10(1 + 2^-24), about 5e-7 dB) and no frame is limited."""
    from elementary_amd.master import master_wav
    x = _tone_file(tmp_path / "in.wav", 0.1)
    got = master_wav(lambda s, k: _hip(s, k, batch_blocks=64), tmp_path / "in.wav", tmp_path / "out.wav", target_lufs=-14.0, ceiling_dbtp=-1.0, fmt="f32")
    print(got)
    assert abs(got["input_lufs"] - lref.gate(lref.mean_squares(x, 48000.0))["integrated"]) < 0.01          # (the meter's own grid: latency frames of silence first)
    assert got["gain_db"] == -14.0 - got["input_lufs"] and 3.0 < got["gain_db"] < 12.0
    assert got["limited_frames"] == 0 and got["max_reduction"] == 0.0 and got["max_reduction_db"] == 0.0
    assert abs(got["output_lufs"] - (-14.0)) <= 1e-5, got["output_lufs"]
    rate, y = _read_wav(tmp_path / "out.wav")
    assert rate == 48000 and y.shape == (x.shape[1], 2)
    assert ref.within(y.T, 10.0 ** (got["gain_db"] / 20.0) * x.astype(np.float64)).all()                   # frame n of the file is G x[n]
    assert abs(got["output_true_peak_dbtp"] - (got["input_true_peak_dbtp"] + got["gain_db"])) < 1e-4


def test_master_wav_limits_what_does_not_fit(gpu_required, tmp_path):
    """A target that would put the peaks over the ceiling: the limiter works, and the s16 file has no sample over full scale."""
    from elementary_amd.master import master_wav
    _tone_file(tmp_path / "in.wav", 0.1)
    got = master_wav(lambda s, k: _hip(s, k, batch_blocks=64), tmp_path / "in.wav", tmp_path / "out.wav", target_lufs=-1.0, ceiling_dbtp=-1.0, fmt="s16",
                     release_ms=100.0)
    print(got)
    assert got["max_reduction"] > 0.0 and got["max_reduction_db"] > 0.0 and got["limited_frames"] > 48000 and got["over"] == 0 and got["nonfinite"] == 0
    assert got["output_lufs"] < -1.0
    rate, y = _read_wav(tmp_path / "out.wav")
    assert int(np.abs(y.astype(np.int32)).max()) <= int(np.ceil(float(CEILING) * 32767.0)) + 1
    silent = tmp_path / "silent.wav"
    _tone_file(silent, 0.0, seconds=1.0)
    with pytest.raises(ValueError):
        master_wav(lambda s, k: _hip(s, k), silent, tmp_path / "never.wav")


def test_off_means_absent(gpu_required):
    """Never set, set to 0, or only its parameters set: the launch counters of PCM, metered and converted renders are those of an
    engine that never heard of the option and every delivered byte is the same; there is nothing to read. On, the render levels
    launch as often: the limiter runs behind them."""
    sr, bs, n_out, frames = 48000.0, 512, 4, 40 * 512 + 11
    x = _inputs(frames)
    keys = ("batch_launches", "spec_launches", "blocks_rendered", "graph_replays", "graph_captures", "resident_launches", "fft_launches",
            "num_levels", "num_islands")
    seen = []
    for opts in ({}, {"limiter": 0}, {"limiter_gain_db": 6, "limiter_lookahead_ms": 3.0}, {"limiter_gain_db": 6, "limiter": 1}):
        a = _hip(sr, bs, batch_blocks=8, specialize=2, **opts)      # (the commit waits for its kernels: the same launches in all of them)
        assert a.render(*_roots(n_out))["result"] == 0
        streams, stats, planar = a.process_blocks_pcm(x, 2, 2, frames, "s16", dither_seed=3, want_float=True)
        host = a.process_blocks_host(x, n_out, frames)
        a.set_option("loudness_meter", 1)
        metered = a.process_blocks_host(x, n_out, frames)
        loud = a.loudness_read()
        a.set_option("resample_rate", 44100)
        converted = a.process_blocks_host(x, n_out, frames)
        seen.append(({k: a.stats()[k] for k in keys}, [s.tobytes() for s in streams], planar.tobytes(), host.tobytes(), {k: v.tobytes() for k, v in stats.items()},
                     metered.tobytes(), loud["mean_squares"].tobytes(), loud["true_peak"].tobytes(), converted.tobytes()))
        if opts.get("limiter") != 1:
            for call in (a.limiter_read, a.limiter_reset):
                with pytest.raises(ElemHipError):
                    call()
        else:
            assert a.limiter_read()["frames"] == converted.shape[1]          # (setting the rate began a new programme)
    assert seen[0] == seen[1] == seen[2], [s[0] for s in seen]
    assert seen[3][0] == seen[0][0] and seen[3][1] != seen[0][1]
    assert seen[0][0]["batch_launches"] >= 10


def test_channel_counts_are_held_to_the_programme(gpu_required):
    """A channel count that is no multiple of `link`, or another count than the programme's, is refused; a reset admits it."""
    a = _limited(RATE, 128, _params(18, 2), batch_blocks=8)
    assert a.render(*_through(2)[:1] * 3)["result"] == 0
    x = ref.signal(128)
    with pytest.raises(ElemHipError):
        a.process_blocks_host(x, 3, 1024)
    a.set_option("limiter_link", 0)
    assert a.process_blocks_host(x, 3, 1024).shape == (3, 1024)
    assert a.render(*_through(2))["result"] == 0
    with pytest.raises(ElemHipError):
        a.process_blocks_host(x, 2, 1024)
    a.limiter_reset()
    assert a.process_blocks_host(x, 2, 1024).shape == (2, 1024)
