"""Delivery at another sample rate on the GPU (option "resample_rate"; elementary_amd/csrc/resample.hip): every launch set of the
host-buffer render calls converted behind its last level, the carried frames crossing sets, halves and calls. The yardstick is
tests/resample_reference.py — a float64 numpy restatement of the formulas, not of the header — applied to the floats a TWIN engine
without the option rendered from the same input, within the reference's own bound B; the packed streams against
tests/pcm_reference.py over the converted floats at output-frame time; bit-for-bit claims against the header's scalar loop compiled
for the host (tests/native/resample_host.cpp)."""
import os
import subprocess
import wave

import numpy as np
import pytest

import loudness_reference as lref
import resample_reference as ref
from elementary_amd import el
from elementary_amd.offline import OfflineRenderer
from elementary_amd.runtime import ElemHipError
from test_gpu_loudness import _check as _check_meter
from test_gpu_pcm import _check_call, _hip, _inputs, _roots
from test_resample_host import CSRC, ROOT, _cxx

pytestmark = pytest.mark.gpu

RATIOS = [(12000, 8000), (8000, 12000), (48000, 44100), (176400, 44100)]


def _plain_roots(n_out, n_in=2):
    """Channel c = in[c % n_in] scaled: no state and no clock, so the floats do not depend on how a render is cut into calls."""
    gains = (1.7, 0.9, -1.3, 0.5, 1.1, -0.7)
    return [el.mul(gains[c % len(gains)], el.in_({"channel": c % n_in})) for c in range(n_out)]


def _pair(fin, fout, bs, roots, **opts):
    """(the engine with the option, its twin without), the same graph rendered on both."""
    a, twin = _hip(float(fin), bs, resample_rate=fout, **opts), _hip(float(fin), bs, **opts)
    assert a.render(*roots)["result"] == 0 and twin.render(*roots)["result"] == 0
    return a, twin


def _within_bound(got, floats, fin, fout, what):
    """`got` [channels, outputs] against the reference over `floats` [channels, frames]: the count exactly, the samples within B."""
    want, bound = ref.resample(floats, fin, fout)
    assert got.shape == want.shape and got.shape[1] == ref.frames_out(floats.shape[1], ref.plan(fin, fout)), (what, got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want)
    print(what, "outputs", got.shape[1], "worst error / bound", float((err / bound).max()), "peak", float(np.abs(want).max()))
    assert (err <= bound).all(), (what, int((err > bound).sum()), np.argwhere(err > bound)[:4].tolist())
    assert float(np.abs(want).max()) > 0.1, what


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("bs", [128, 512])
@pytest.mark.parametrize("fin,fout", RATIOS)
def test_floats_and_streams_equal_the_references(gpu_required, fin, fout, bs, G):
    """20 blocks + 37 frames in sets of 8 blocks: three sets, both halves, a cut last block, carried frames that cross set boundaries
    (at 176400 -> 44100 with block size 128 they span two blocks); two streams of G channels delivered as s16 with dither, as f32
    and as planar floats — a programme each."""
    n_out, frames = 2 * G, 20 * bs + 37
    a, twin = _pair(fin, fout, bs, _roots(n_out), batch_blocks=8)
    pl = ref.plan(fin, fout)
    for k, fmt in enumerate(("s16", "f32", None)):
        x = _inputs(frames) if k == 0 else np.roll(_inputs(frames), 1000 * k, axis=1)
        a.resample_reset()
        floats = twin.process_blocks_host(x, n_out, frames)
        if fmt is None:
            planar = a.process_blocks_host(x, n_out, frames)
        else:
            seed = 5 if fmt == "s16" else None
            streams, stats, planar = a.process_blocks_pcm(x, 2, G, frames, fmt, dither_seed=seed, want_float=True)
            _check_call(streams, stats, planar, G, fmt, seed, 0)           # (output-frame time: the programme began at the reset)
        _within_bound(planar, floats, fin, fout, (fin, fout, bs, G, fmt))
        got = a.resample_read()
        assert (got["up"], got["down"], got["taps"], got["latency_frames"]) == (pl["L"], pl["M"], pl["T"], pl["Do"])
        assert got["frames_in"] == frames and got["frames_out"] == planar.shape[1] == ref.frames_out(frames, pl)
    assert a.stats()["batch_launches"] >= 3


def test_cuts_set_sizes_and_engines_leave_the_same_bits(gpu_required):
    """One call against three calls (9 blocks + 5 frames, 41 blocks, the rest), launch sets of 8 blocks against one set, a second
    engine, and the programme once more after a reset: the same bytes, packed and planar. (A stateless graph whose root fades have
    settled: the call that ends inside a block renders the same floats as the call that does not.)"""
    fin, fout, bs, n_out = 48000, 44100, 128, 4
    frames = 60 * bs + 37
    cuts = [0, 9 * bs + 5, 9 * bs + 5 + 41 * bs, frames]
    x = _inputs(frames)
    pl = ref.plan(fin, fout)

    def one(rt):
        streams, _, planar = rt.process_blocks_pcm(x, 2, 2, frames, "s24", dither_seed=21, want_float=True)
        return [s.tobytes() for s in streams], planar.tobytes()

    def three(rt):
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            parts.append(rt.process_blocks_pcm(x[:, lo:hi], 2, 2, hi - lo, "s24", dither_seed=21, want_float=True))
            got = rt.resample_read()
            assert got["frames_in"] == hi and got["frames_out"] == ref.frames_out(hi, pl) == sum(p[2].shape[1] for p in parts)
        return [np.concatenate([p[0][s] for p in parts]).tobytes() for s in range(2)], np.concatenate([p[2] for p in parts], axis=1).tobytes()

    seen = []
    for batch in (8, 1024, 8):
        rt = _hip(float(fin), bs, resample_rate=fout, batch_blocks=batch)
        assert rt.render(*_plain_roots(n_out))["result"] == 0
        rt.process_blocks_host(x[:, :40 * bs], n_out, 40 * bs)              # (the roots' fade-in: 20 ms)
        rt.resample_reset()
        seen.append(one(rt))
        rt.resample_reset()
        got = rt.resample_read()
        assert got["frames_in"] == 0 and got["frames_out"] == 0
        seen.append(three(rt))
        rt.resample_reset()
        seen.append(one(rt))                                               # the programme repeats
    for other in seen[1:]:
        assert other == seen[0]
    planar = np.frombuffer(seen[0][1], dtype=np.float32).reshape(n_out, -1)
    gains = np.array([1.7, 0.9, -1.3, 0.5], dtype=np.float32)[:, None]
    _within_bound(planar, gains * x[[0, 1, 0, 1]], fin, fout, "cuts")


def _host_loop(tmp_path, floats, fin, fout):
    """resample_host() of the header over `floats` [channels, frames], one programme from time 0."""
    exe = os.path.join(str(tmp_path), "resample_host")
    if not os.path.exists(exe):
        subprocess.run([_cxx(), "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "native", "resample_host.cpp"), "-o", exe], check=True)
    np.ascontiguousarray(floats, dtype=np.float32).tofile(os.path.join(str(tmp_path), "apply_in.f32"))
    subprocess.run([exe, str(tmp_path), "apply", str(fin), str(fout), str(floats.shape[0])], check=True, capture_output=True, timeout=120)
    return np.fromfile(os.path.join(str(tmp_path), "apply_out.f32"), dtype=np.float32).reshape(floats.shape[0], -1)


def test_sliced_host_block_700_s24_three_channels(gpu_required, tmp_path):
    """Block 700 renders as two slices of 350 frames; launch sets hold whole host blocks. Within B of the reference, the bits of
    the header's scalar loop, the streams packed at output-frame time."""
    fin, fout, bs, G, n_out = 48000, 44100, 700, 3, 6
    frames = 21 * bs + 37
    a, twin = _pair(fin, fout, bs, _roots(n_out), batch_blocks=8)
    x = _inputs(frames)
    floats = twin.process_blocks_host(x, n_out, frames)
    streams, stats, planar = a.process_blocks_pcm(x, 2, G, frames, "s24", dither_seed=99, want_float=True)
    _check_call(streams, stats, planar, G, "s24", 99, 0)
    _within_bound(planar, floats, fin, fout, "block 700")
    assert np.array_equal(planar.view(np.uint32), _host_loop(tmp_path, floats, fin, fout).view(np.uint32))
    assert a.stats()["batch_launches"] >= 1


def test_host_loop_for_taps_under_a_sliced_block_continues_the_programme(gpu_required, tmp_path):
    """A tap graph at host block 700 renders host block by host block through process(): the floats are on the host and go through
    the header's scalar loop with the carried frames brought over for the call. A programme begun by launch sets goes on through it,
    and back: the bits are resample_host() over the concatenated floats."""
    fin, fout, bs, frames = 48000, 44100, 700, 9 * 700 + 211
    taps = [el.tapOut({"name": "fb"}, el.add(el.mul(1.5, el.in_({"channel": 0})), el.mul(0.5, el.tapIn({"name": "fb"})))),
            el.mul(0.9, el.in_({"channel": 1}))]
    a, twin = _pair(fin, fout, bs, _roots(2), batch_blocks=8)
    x = _inputs(frames)
    pl = ref.plan(fin, fout)
    f0, p0 = twin.process_blocks_host(x, 2, frames), a.process_blocks_host(x, 2, frames)
    sets = a.stats()["batch_launches"]
    assert sets >= 1
    assert a.render(*taps)["result"] == 0 and twin.render(*taps)["result"] == 0
    t1 = a.resample_read()["frames_out"]
    f1 = twin.process_blocks_host(x, 2, frames)
    streams, stats, p1 = a.process_blocks_pcm(x, 1, 2, frames, "s24", dither_seed=4, want_float=True)
    _check_call(streams, stats, p1, 2, "s24", 4, t1)
    f2, p2 = twin.process_blocks_host(x, 2, frames), a.process_blocks_host(x, 2, frames)
    assert a.stats()["batch_launches"] == sets                   # (those two did take the block-by-block path)
    assert a.render(*_roots(2))["result"] == 0 and twin.render(*_roots(2))["result"] == 0
    f3, p3 = twin.process_blocks_host(x, 2, frames), a.process_blocks_host(x, 2, frames)
    floats, got = np.concatenate([f0, f1, f2, f3], axis=1), np.concatenate([p0, p1, p2, p3], axis=1)
    assert got.shape[1] == ref.frames_out(4 * frames, pl) == a.resample_read()["frames_out"]
    want = _host_loop(tmp_path, floats, fin, fout)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    _within_bound(got, floats, fin, fout, "launch sets, taps, taps, launch sets")


@pytest.mark.parametrize("meter_first", [True, False])
def test_the_meter_meters_what_is_delivered(gpu_required, meter_first):
    """With `loudness_meter`, whichever option is set first: the read-out is the loudness reference's over the converted floats at the
    DELIVERY rate, within that module's own bound; hop = round(fout / 10)."""
    fin, fout, bs, n_out = 48000, 44100, 512, 4
    frames = 40 * bs + 37
    opts = [("loudness_meter", 1), ("resample_rate", fout)]
    a = _hip(float(fin), bs, batch_blocks=8, **dict(opts if meter_first else opts[::-1]))
    assert a.render(*_roots(n_out))["result"] == 0
    x = _inputs(frames)
    _, _, planar = a.process_blocks_pcm(x, 2, 2, frames, "s16", want_float=True)
    got = _check_meter(a, planar, float(fout), None, ("meter first", meter_first))
    assert got["hop"] == round(fout / 10) == lref.hop(float(fout)) and got["frames"] == planar.shape[1] == ref.frames_out(frames, ref.plan(fin, fout))
    more = a.process_blocks_host(x, n_out, frames)
    _check_meter(a, np.concatenate([planar, more], axis=1), float(fout), None, "a second call")


def _renderer(n_in, n_out, fin, bs, fout, roots):
    core = OfflineRenderer(lambda s, n: _hip(s, n, batch_blocks=8))
    kw = {} if fout is None else {"output_sample_rate": fout}
    core.initialize(num_input_channels=n_in, num_output_channels=n_out, sample_rate=fin, block_size=bs, **kw)
    core.render(*roots)
    return core


def _read_wav(path):
    from elementary_amd.wav import WavReader
    with WavReader(str(path)) as r:
        return r.sample_rate, r.read(r.frames)


def test_wav_files_at_the_delivery_rate(gpu_required, tmp_path):
    """write_wav / process_wav with output_sample_rate: the header carries the delivery rate, the file holds ceil(num_frames L / M)
    frames, frame n of it is output n + Do of the plain call, and the bytes do not depend on chunk_frames."""
    fin, fout, bs, n_out, frames = 48000, 44100, 512, 4, 30 * 512 + 123
    pl = ref.plan(fin, fout)
    L, M, Do = pl["L"], pl["M"], pl["Do"]
    x = _inputs(frames)
    codes = np.round(x.T * 32767.0).astype(np.int16)
    with wave.open(str(tmp_path / "in.wav"), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(fin); w.writeframes(codes.tobytes())
    roots = _plain_roots(n_out)
    files = {}
    for chunk in (7 * 512, 1 << 20):
        core = _renderer(2, n_out, fin, bs, fout, roots)
        st_w = core.write_wav(str(tmp_path / f"w{chunk}_{{}}.wav"), list(x), frames, "s24", channels_per_stream=2, dither_seed=11, chunk_frames=chunk)
        st_p = core.process_wav(str(tmp_path / "in.wav"), str(tmp_path / f"p{chunk}_{{}}.wav"), "s16", channels_per_stream=2, chunk_frames=chunk)
        assert set(st_w) == set(st_p) == {"peak", "over", "nonfinite"}
        for name in ("w", "p"):
            for s in range(2):
                files[name, s, chunk] = (tmp_path / f"{name}{chunk}_{s}.wav").read_bytes()
    for name in ("w", "p"):
        for s in range(2):
            assert files[name, s, 7 * 512] == files[name, s, 1 << 20], (name, s)
    keep, extra = -((-frames * L) // M), -((-Do * M) // L)
    # the plain calls: a fresh programme of frames + extra rendered frames
    plain = _hip(float(fin), bs, batch_blocks=8, resample_rate=fout)
    assert plain.render(*roots)["result"] == 0
    xp = np.concatenate([x, np.zeros((2, extra), dtype=np.float32)], axis=1)
    streams_w, _, _ = plain.process_blocks_pcm(xp, 2, 2, frames + extra, "s24", dither_seed=11)
    plain.resample_reset()
    cp = np.concatenate([codes, np.zeros((extra, 2), dtype=np.int16)])
    streams_p, _, _ = plain.process_blocks_pcm_io([cp], "s16", num_frames=frames + extra, out_fmt="s16", num_streams=2, channels_per_stream=2)
    for s in range(2):
        rate, got = _read_wav(tmp_path / f"w{1 << 20}_{s}.wav")
        assert rate == fout and got.shape[0] == keep and np.array_equal(got, streams_w[s][Do:Do + keep])
        rate, got = _read_wav(tmp_path / f"p{1 << 20}_{s}.wav")
        assert rate == fout and got.shape[0] == keep and np.array_equal(got, streams_p[s][Do:Do + keep])
    with pytest.raises(RuntimeError):
        _renderer(2, n_out, fin, bs, None, roots).resample()


def test_a_sine_lands_on_the_delivery_rate_s_grid(gpu_required, tmp_path):
    """A 1 kHz sine through a pass-through graph, 48000 -> 44100, written as a float file: frame n is sin(2 pi 1000 n / 44100)
    within 2e-5 in the steady state (the float32 input plus the 0.001 dB ripple; numpy gives 1e-6)."""
    fin, fout, bs, frames = 48000, 44100, 512, 12 * 512 + 77
    x = np.sin(2.0 * np.pi * 1000.0 * np.arange(frames + 200) / fin).astype(np.float32)[None, :]
    core = _renderer(1, 1, fin, bs, fout, [el.in_({"channel": 0})])
    core.write_wav(str(tmp_path / "sine.wav"), list(x), frames, "f32")
    rate, got = _read_wav(tmp_path / "sine.wav")
    assert rate == fout and got.shape == (ref.frames_out(frames, ref.plan(fin, fout)), 1)
    n = np.arange(got.shape[0])
    err = np.abs(got[:, 0] - np.sin(2.0 * np.pi * 1000.0 * n / fout))
    steady = slice(2000, got.shape[0] - 80)          # (clear of the root's fade-in, 20 ms, and of the programme's edges: T = 70 taps)
    print("worst steady-state error", float(err[steady].max()))
    assert float(err[steady].max()) <= 2e-5
    # the renderer's own buffers: process() delivers ceil(rendered L / M) frames
    core.resample_reset()
    out = [np.zeros(ref.frames_out(frames, ref.plan(fin, fout)), dtype=np.float32)]
    core.process([x[0, :frames]], out)
    lat = core.resample()["latency_frames"]
    assert core.resample()["frames_in"] == frames and float(np.abs(out[0][lat + 2000:] - got[2000:got.shape[0] - lat, 0]).max()) == 0.0


def test_off_means_absent(gpu_required):
    """Never set, or set to 0, the launch counters of a render are those of an engine that never heard of the option and every
    delivered byte is the same; there is nothing to read. On, the render levels launch as often: the converter runs behind them."""
    sr, bs, n_out, frames = 44100.0, 512, 4, 40 * 512 + 11
    x = _inputs(frames)
    keys = ("batch_launches", "spec_launches", "blocks_rendered", "graph_replays", "graph_captures", "resident_launches", "fft_launches",
            "num_levels", "num_islands")
    seen = []
    for opts in ({}, {"resample_rate": 0}, {"resample_rate": sr}, {"resample_rate": 48000}):
        a = _hip(sr, bs, batch_blocks=8, specialize=2, **opts)      # (the commit waits for its kernels: the same launches in all of them)
        assert a.render(*_roots(n_out))["result"] == 0
        streams, stats, planar = a.process_blocks_pcm(x, 2, 2, frames, "s16", dither_seed=3, want_float=True)
        host = a.process_blocks_host(x, n_out, frames)
        seen.append(({k: a.stats()[k] for k in keys}, [s.tobytes() for s in streams], planar.tobytes(), host.tobytes(), {k: v.tobytes() for k, v in stats.items()}))
        if opts.get("resample_rate") != 48000:
            assert a.resample_frames(frames) == frames
            for call in (a.resample_read, a.resample_reset):
                with pytest.raises(ElemHipError):
                    call()
        else:
            assert a.resample_read()["frames_in"] == 2 * frames
    assert seen[0] == seen[1] == seen[2], [s[0] for s in seen]
    assert seen[3][0] == seen[0][0] and seen[3][1] != seen[0][1]
    assert seen[0][0]["batch_launches"] >= 10
