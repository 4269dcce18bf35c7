"""Inputs at another sample rate on the GPU (option "input_rate"; elementary_amd/csrc/resample_in.hip): every launch set's stretch of
the input decoded and converted to the engine's rate in front of its first level, the carried frames crossing sets, halves and
calls. Bit-for-bit claims are made against a TWIN engine without the option that is fed, as planar floats, what the header's scalar
pull loop (resample_in_host, compiled for the host: tests/native/resample_in_host.cpp) makes of the decoded input; the filter itself
is held to tests/resample_reference.py — a float64 numpy restatement of the formulas, not of the header — within that reference's
own bound B."""
import os
import subprocess

import numpy as np
import pytest

import resample_reference as ref
from elementary_amd import el
from elementary_amd.offline import OfflineRenderer
from elementary_amd.runtime import ElemHipError
from test_gpu_pcm import _hip, _inputs, _roots
from test_gpu_resample import _plain_roots, _read_wav
from test_resample_in_host import build_host_program, need

pytestmark = pytest.mark.gpu

RATIOS = [(8000, 12000), (12000, 8000), (44100, 48000), (44100, 176400)]          # (input rate, engine rate)
GAINS = np.array([1.7, 0.9, -1.3, 0.5, 1.1, -0.7], dtype=np.float32)


@pytest.fixture(scope="module")
def host_loop(tmp_path_factory):
    """resample_in_host() of the header over `floats` [channels, input frames], one programme from time 0: `frames` engine frames."""
    work = tmp_path_factory.mktemp("resample_in_apply")
    exe = build_host_program(work)

    def apply(floats, fin, fout, frames):
        floats = np.ascontiguousarray(floats, dtype=np.float32)
        floats.tofile(os.path.join(str(work), "apply_in.f32"))
        subprocess.run([exe, str(work), "apply", str(fin), str(fout), str(floats.shape[0]), str(frames)], check=True, capture_output=True, timeout=120)
        return np.fromfile(os.path.join(str(work), "apply_out.f32"), dtype=np.float32).reshape(floats.shape[0], frames)
    return apply


def _encode(x, fmt, G):
    """x float32 [channels, frames] -> (streams of G channels in `fmt`, the floats those streams decode to)."""
    if fmt == "s16":
        codes = np.round(x * 32767.0).astype(np.int16)
        dec = codes.astype(np.float32) * np.float32(2.0 ** -15)
        streams = [np.ascontiguousarray(codes[s:s + G].T) for s in range(0, x.shape[0], G)]
    elif fmt == "s24":
        codes = np.round(x.astype(np.float64) * 8388607.0).astype(np.int32)
        dec = codes.astype(np.float32) * np.float32(2.0 ** -23)
        u = codes.astype(np.uint32)
        b = np.stack([(u >> (8 * k)) & 0xFF for k in range(3)], axis=-1).astype(np.uint8)          # [channels, frames, 3]
        streams = [np.ascontiguousarray(b[s:s + G].transpose(1, 0, 2)) for s in range(0, x.shape[0], G)]
    else:
        dec = x
        streams = [np.ascontiguousarray(x[s:s + G].T) for s in range(0, x.shape[0], G)]
    return streams, dec


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("bs", [128, 512])
@pytest.mark.parametrize("fin,fout", RATIOS)
def test_render_equals_the_twin_fed_by_the_scalar_loop(gpu_required, host_loop, fin, fout, bs, G):
    """20 blocks + 37 engine frames in sets of 8 blocks: three sets, both halves, a cut last block, carried frames that cross set
    boundaries; two streams of G channels as s16, s24 and f32, and the same channels as planar floats — a programme each."""
    n_in, n_out, frames = 2 * G, 2 * G, 20 * bs + 37
    a, twin = _hip(float(fout), bs, input_rate=fin, batch_blocks=8), _hip(float(fout), bs, batch_blocks=8)
    roots = _roots(n_out, n_in)
    assert a.render(*roots)["result"] == 0 and twin.render(*roots)["result"] == 0
    pl = ref.plan(fin, fout)
    ni = need(frames, pl["L"], pl["M"])
    for k, fmt in enumerate(("s16", "s24", "f32", None)):
        x = np.roll(_inputs(ni, n_in), 1000 * k, axis=1)
        a.input_resample_reset()
        assert a.input_resample_frames(frames) == ni
        if fmt is None:
            dec = x
            got = a.process_blocks_host(x, n_out, frames)
        else:
            streams, dec = _encode(x, fmt, G)
            got = a.process_blocks_pcm_io(streams, fmt, num_outputs=n_out, num_frames=frames)
        want = twin.process_blocks_host(host_loop(dec, fin, fout, frames), n_out, frames)
        assert _same_bits(got, want), (fmt, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        assert float(np.abs(want).max()) > 0.1
        info = a.input_resample_read()
        assert (info["up"], info["down"], info["taps"], info["latency_frames"]) == (pl["L"], pl["M"], pl["T"], pl["Do"])
        assert info["frames_in"] == ni and info["frames_out"] == frames
    assert a.stats()["batch_launches"] >= 3


def _settled(fin, fout, bs, n_out, **opts):
    """A pass-through engine whose root fades have settled, at the start of a programme."""
    rt = _hip(float(fout), bs, input_rate=fin, **opts)
    assert rt.render(*_plain_roots(n_out))["result"] == 0
    rt.process_blocks_host(np.zeros((2, rt.input_resample_frames(40 * bs)), dtype=np.float32), n_out, 40 * bs)      # (the roots' fade-in: 20 ms)
    rt.input_resample_reset()
    if "resample_rate" in opts:
        rt.resample_reset()
    return rt


@pytest.mark.parametrize("fin,fout", [(44100, 48000), (12000, 8000)])
def test_pass_through_is_within_the_bound_of_the_reference(gpu_required, fin, fout):
    bs, n_out, frames = 128, 4, 20 * 128 + 37
    pl = ref.plan(fin, fout)
    rt = _settled(fin, fout, bs, n_out, batch_blocks=8)
    streams, x = _encode(_inputs(need(frames, pl["L"], pl["M"])), "s16", 2)
    got = rt.process_blocks_pcm_io(streams, "s16", num_outputs=n_out, num_frames=frames)
    y, bound = ref.resample(x, fin, fout)
    gain = GAINS[:n_out, None].astype(np.float64)
    want, B = gain * y[[0, 1, 0, 1], :frames], np.abs(gain) * bound[[0, 1, 0, 1], :frames]
    err = np.abs(got.astype(np.float64) - want)
    tol = B + 2.0 ** -24 * np.abs(want)               # the reference's own bound, and one rounding of the gain
    print(fin, fout, "worst error / tolerance", float((err / tol).max()), "peak", float(np.abs(want).max()))
    assert got.shape == want.shape and (err <= tol).all(), (int((err > tol).sum()), np.argwhere(err > tol)[:4].tolist())
    assert float(np.abs(want).max()) > 0.1


def test_cuts_set_sizes_and_engines_leave_the_same_bits(gpu_required):
    """One call against three calls (9 blocks + 5 frames, 41 blocks, the rest), launch sets of 8 blocks against one set, a second
    engine, and the programme once more after a reset: the same bytes, packed and planar."""
    fin, fout, bs, n_out = 44100, 48000, 128, 4
    frames = 60 * bs + 37
    cuts = [0, 9 * bs + 5, 9 * bs + 5 + 41 * bs, frames]
    pl = ref.plan(fin, fout)
    L, M = pl["L"], pl["M"]
    streams, _ = _encode(_inputs(need(frames, L, M)), "s24", 2)

    def one(rt):
        s, _, planar = rt.process_blocks_pcm_io(streams, "s24", num_frames=frames, out_fmt="s24", num_streams=2, channels_per_stream=2, dither_seed=21,
                                                want_float=True, sample_time=0)
        return [a.tobytes() for a in s], planar.tobytes()

    def three(rt):
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            ni = rt.input_resample_frames(hi - lo)
            assert ni == need(hi, L, M) - need(lo, L, M)
            parts.append(rt.process_blocks_pcm_io([streams[0][need(lo, L, M):need(hi, L, M)]], "s24", num_frames=hi - lo, out_fmt="s24", num_streams=2,
                                                  channels_per_stream=2, dither_seed=21, want_float=True, sample_time=lo))
            got = rt.input_resample_read()
            assert got["frames_in"] == need(hi, L, M) and got["frames_out"] == hi
        return [np.concatenate([p[0][s] for p in parts]).tobytes() for s in range(2)], np.concatenate([p[2] for p in parts], axis=1).tobytes()

    seen = []
    for batch in (8, 1024, 8):
        rt = _settled(fin, fout, bs, n_out, batch_blocks=batch)
        seen.append(one(rt))
        rt.input_resample_reset()
        got = rt.input_resample_read()
        assert got["frames_in"] == 0 and got["frames_out"] == 0
        seen.append(three(rt))
        rt.input_resample_reset()
        seen.append(one(rt))                                               # the programme repeats
    for other in seen[1:]:
        assert other == seen[0]
    assert np.abs(np.frombuffer(seen[0][1], dtype=np.float32)).max() > 0.1


def test_host_loop_for_taps_under_a_sliced_block_leaves_the_launch_sets_bits(gpu_required):
    """A tap graph at host block 700 renders host block by host block through process(): the inputs are decoded and converted on the
    host by the header's scalar loops, with the carried frames brought over for the call. Its stateless channel carries the bits the
    launch sets left for the same programme, and a programme begun by one path goes on through the other."""
    fin, fout, bs, frames = 44100, 48000, 700, 9 * 700 + 211
    pl = ref.plan(fin, fout)
    ni = need(frames, pl["L"], pl["M"])
    taps = [el.tapOut({"name": "fb"}, el.add(el.mul(1.5, el.in_({"channel": 0})), el.mul(0.5, el.tapIn({"name": "fb"})))),
            el.mul(0.9, el.in_({"channel": 1}))]
    streams, _ = _encode(_inputs(2 * ni), "s16", 2)
    settle = [np.zeros((ni + 8, 2), dtype=np.int16)]          # (a stretch's length depends on where the programme stands: a frame or two to spare)
    a = _hip(float(fout), bs, input_rate=fin, batch_blocks=8)
    seen = {}
    for name, roots in (("sets", _plain_roots(2)), ("taps", taps)):
        assert a.render(*roots)["result"] == 0
        a.process_blocks_pcm_io(settle, "s16", num_outputs=2, num_frames=frames)          # (the roots' fade: 20 ms)
        a.input_resample_reset()
        sets = a.stats()["batch_launches"]
        first = a.process_blocks_pcm_io([streams[0][:ni]], "s16", num_outputs=2, num_frames=frames)
        took = a.input_resample_frames(frames)
        second = a.process_blocks_pcm_io([streams[0][ni:ni + took]], "s16", num_outputs=2, num_frames=frames)
        assert (a.stats()["batch_launches"] > sets) == (name == "sets")                   # (the tap graph did take the block-by-block path)
        info = a.input_resample_read()
        assert info["frames_out"] == 2 * frames and info["frames_in"] == need(2 * frames, pl["L"], pl["M"]) == ni + took
        seen[name] = np.concatenate([first, second], axis=1)
    assert _same_bits(seen["taps"][1], seen["sets"][1]), int((seen["taps"][1].view(np.uint32) != seen["sets"][1].view(np.uint32)).sum())
    assert float(np.abs(seen["sets"][1]).max()) > 0.1
    # ... and across the paths: launch sets first, the host loop second
    assert a.render(*_plain_roots(2))["result"] == 0
    a.process_blocks_pcm_io(settle, "s16", num_outputs=2, num_frames=frames)
    a.input_resample_reset()
    first = a.process_blocks_pcm_io([streams[0][:ni]], "s16", num_outputs=2, num_frames=frames)
    assert a.render(*taps)["result"] == 0
    took = a.input_resample_frames(frames)
    second = a.process_blocks_pcm_io([streams[0][ni:ni + took]], "s16", num_outputs=2, num_frames=frames)
    tail = slice(frames + 2000, 2 * frames)               # (clear of the new roots' fade)
    assert _same_bits(second[1][2000:], seen["sets"][1][tail])


def _renderer(n_in, n_out, sr, bs, roots, **kw):
    core = OfflineRenderer(lambda s, n: _hip(s, n, batch_blocks=8))
    core.initialize(num_input_channels=n_in, num_output_channels=n_out, sample_rate=sr, block_size=bs, **kw)
    core.render(*roots)
    return core


def _write_wav(path, fmt, rate, stream):
    from elementary_amd.wav import WavWriter
    with WavWriter(str(path), fmt, stream.shape[1], rate) as w:
        w.write(stream)


def test_both_converters_on_a_file_up_and_down_again(gpu_required, tmp_path):
    """A 44100 Hz float file into a 176400 Hz engine and out at 44100 Hz through process_wav with a pass-through graph: as many
    frames as the input, all latencies taken out, and clear of the edges the reference applied twice — up, then down — within the
    sum of its two bounds, the first carried through the second filter (its absolute coefficient sum)."""
    fin, sr, bs, F = 44100, 176400, 512, 5000
    x = (0.5 * np.sin(2.0 * np.pi * 997.0 * np.arange(F) / fin) + 0.4 * _inputs(F, 1)[0]).astype(np.float32)
    _write_wav(tmp_path / "in.wav", "f32", fin, x[:, None])
    core = _renderer(1, 1, sr, bs, [el.in_({"channel": 0})], input_sample_rate=fin, output_sample_rate=fin)
    core.process_pcm_io([np.zeros((1, 1), dtype=np.float32)], "f32", 40 * bs)          # (the root's fade-in)
    core.process_wav(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), "f32")
    rate, got = _read_wav(tmp_path / "out.wav")
    assert rate == fin and got.shape == (F, 1)
    up, down = ref.plan(fin, sr), ref.plan(sr, fin)
    assert core.input_resample()["latency_frames"] == up["Do"] and core.resample()["latency_frames"] == down["Do"]
    xp = np.concatenate([x, np.zeros(200, dtype=np.float32)])
    u, bu = ref.resample(xp, fin, sr)
    u, bu = u[:, up["Do"]:], bu[:, up["Do"]:]
    d, bd = ref.resample(u, sr, fin)
    d, bd = d[0, down["Do"]:], bd[0, down["Do"]:]
    carried = float(np.abs(ref.phases(down)).sum(axis=1).max())
    tol = bd[:F] + float(bu.max()) * carried
    err = np.abs(got[:, 0].astype(np.float64) - d[:F])
    mid = slice(256, F - 256)
    print("worst error / tolerance", float((err[mid] / tol[mid]).max()), "peak", float(np.abs(d[:F]).max()))
    assert (err[mid] <= tol[mid]).all() and float(np.abs(d[:F][mid]).max()) > 0.3


def test_a_48000_s16_file_through_a_44100_engine_with_the_meter(gpu_required, tmp_path):
    fin, sr, bs, F = 48000, 44100, 512, 40000          # (0.83 s: the meter's gate wants 400 ms and more)
    codes = np.round(_inputs(F).T * 32767.0).astype(np.int16)
    _write_wav(tmp_path / "in.wav", "s16", fin, codes)
    core = _renderer(2, 2, sr, bs, _plain_roots(2), input_sample_rate=fin, loudness_meter=True)
    stats = core.process_wav(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), "s24")
    rate, got = _read_wav(tmp_path / "out.wav")
    keep = -((-F * 147) // 160)
    assert rate == sr and got.shape[0] == keep
    info = core.input_resample()
    assert (info["up"], info["down"]) == (147, 160) and info["frames_out"] == keep + info["latency_frames"]
    assert info["frames_in"] == need(info["frames_out"], 147, 160)
    assert np.isfinite(stats["integrated_lufs"]) and np.isfinite(stats["true_peak_dbtp"]) and stats["peak"].max() > 0.1
    # a file at any other rate is still refused
    _write_wav(tmp_path / "odd.wav", "s16", 32000, codes)
    with pytest.raises(ValueError, match="sample rate 32000 of an input file"):
        core.process_wav(str(tmp_path / "odd.wav"), str(tmp_path / "never.wav"), "s24")


def test_master_wav_oversampled(gpu_required, tmp_path):
    from elementary_amd.master import master_wav
    rate, F = 44100, 3 * 44100 // 2
    t = np.arange(F) / rate
    x = np.stack([0.25 * np.sin(2 * np.pi * 440.0 * t), 0.2 * np.sin(2 * np.pi * 660.0 * t)], axis=1)
    _write_wav(tmp_path / "in.wav", "s16", rate, np.round(x * 32767.0).astype(np.int16))
    got = master_wav(lambda s, n: _hip(s, n, batch_blocks=64), tmp_path / "in.wav", tmp_path / "out.wav", target_lufs=-16.0, oversample=4)
    out_rate, y = _read_wav(tmp_path / "out.wav")
    assert out_rate == rate and y.shape[0] == F
    for key in ("input_lufs", "input_true_peak_dbtp", "output_lufs", "output_true_peak_dbtp", "gain_db"):
        assert np.isfinite(got[key]), (key, got)
    print(got)
    assert abs(got["output_lufs"] - (-16.0)) < 0.5 and abs(got["gain_db"] - (-16.0 - got["input_lufs"])) < 1e-9


def test_non_finite_float_input_arrives_non_finite(gpu_required):
    fin, fout, bs, frames = 44100, 48000, 128, 16 * 128
    rt = _settled(fin, fout, bs, 2, batch_blocks=8)
    x = _inputs(rt.input_resample_frames(frames))
    x[0, 700], x[1, 900] = np.inf, np.nan
    got = rt.process_blocks_pcm_io([np.ascontiguousarray(x.T)], "f32", num_outputs=2, num_frames=frames)
    for c, at in ((0, 700), (1, 900)):
        bad = np.flatnonzero(~np.isfinite(got[c]))
        centre = at * 160 // 147 + 35
        assert 32 <= len(bad) <= 80 and abs(int(bad.mean()) - centre) <= 2, (c, len(bad), bad[:3], centre)
    assert np.isfinite(got[:, :600]).all() and np.isfinite(got[:, 1200:]).all()


def test_short_inputs_and_refused_rates(gpu_required):
    fin, fout, bs, frames = 44100, 48000, 128, 16 * 128
    rt = _settled(fin, fout, bs, 2, batch_blocks=8)
    ni = rt.input_resample_frames(frames)
    x = _inputs(ni)
    with pytest.raises(ValueError):
        rt.process_blocks_host(x[:, :ni - 1], 2, frames)
    with pytest.raises(ValueError):
        rt.process_blocks_pcm_io([np.ascontiguousarray(x[:, :ni - 1].T)], "f32", num_outputs=2, num_frames=frames)
    assert rt.input_resample_read()["frames_out"] == 0          # (refused in front of the engine: the programme has not moved)
    want = rt.process_blocks_host(x, 2, frames)
    # without num_frames: as many engine frames as the inputs cover
    rt.input_resample_reset()
    assert rt.process_blocks_host(x, 2).shape == (2, frames)
    rt.input_resample_reset()
    assert rt.process_blocks_host(x[:, :ni - 1], 2).shape == (2, frames - 1)
    for bad in (44101, 0.5, 9 * 48000):
        with pytest.raises(ElemHipError):
            rt.set_option("input_rate", bad)
        assert rt._lib.elemhip_set_option(rt._h, b"input_rate", float(bad)) == 6
    info = rt.input_resample_read()
    assert (info["up"], info["down"]) == (160, 147)
    rt.input_resample_reset()
    assert _same_bits(rt.process_blocks_host(x, 2, frames), want)


def test_offline_renderer_walks_an_input_cursor(gpu_required):
    """process and process_pcm hand every engine call the input frames it consumes and pad an input that ends early with silence: the
    floats of the plain call over the padded input."""
    fin, sr, bs, frames = 44100, 48000, 128, 30 * 128 + 50
    roots = _plain_roots(2)
    plain = _settled(fin, sr, bs, 2, batch_blocks=8)
    ni = plain.input_resample_frames(frames)
    x = _inputs(ni - 300)                                  # (ends 300 frames early)
    xp = np.concatenate([x, np.zeros((2, 300), dtype=np.float32)], axis=1)
    want = plain.process_blocks_host(xp, 2, frames)
    core = _renderer(2, 2, sr, bs, roots, input_sample_rate=fin)
    core.process([np.zeros(1, dtype=np.float32)] * 2, [np.zeros(40 * bs, dtype=np.float32) for _ in range(2)])      # (the roots' fade-in)
    core.input_resample_reset()
    out = [np.zeros(frames, dtype=np.float32) for _ in range(2)]
    core.process(list(x), out)
    assert _same_bits(np.stack(out), want)
    assert core.input_resample()["frames_out"] == frames and core.input_resample()["frames_in"] == ni
    core.input_resample_reset()
    _, _, planar = core.process_pcm(list(x), 1, 2, frames, "s16", want_float=True)
    assert _same_bits(planar, want) and float(np.abs(want).max()) > 0.1
