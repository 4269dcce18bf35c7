"""FLAC delivery of the offline host path (elemhip_process_blocks_flac): launch sets whose delivered frames are quantised, encoded and
assembled into RFC 9639 frames on the GPU (elementary_amd/csrc/flac_encode.hip). The central contract: decoding the stream with
tests/flac_reference.py — a decoder written from the RFC, not from the header — gives the s16 / s24 codes process_blocks_pcm delivers
for the same graph, seed and sample time, sample for sample; and the bytes are those of elemhip_flac_encode, the scalar twin, fed with
those codes. Small shapes: engine blocks of 64 and 350 frames, FLAC frames of 256, renders of 3 to 5 FLAC frames and a ragged tail."""
import numpy as np
import pytest

import flac_reference as ref
import loudness_reference as lref
from elementary_amd import el
from elementary_amd.offline import OfflineRenderer
from helpers import lcg_noise_fast

pytestmark = pytest.mark.gpu
SR = 44100.0
FF = 256
GAINS = (1.7, 0.9, -1.3, 0.5, 1.1, -0.7, 0.3, 1.9, -0.2, 0.8, 1.4, -1.0, 0.6, -0.4, 1.2, 0.1)


def _hip(sr, bs, **opts):
    from elementary_amd.runtime import Runtime
    rt = Runtime(sr, bs, device=0)
    for k, v in opts.items():
        rt.set_option(k, v)
    return rt


def _roots(n_out, n_in=2):
    """Channel c = in[c % n_in] scaled by a constant (some beyond full scale: they clip)."""
    return [el.mul(GAINS[c % len(GAINS)], el.in_({"channel": c % n_in})) for c in range(n_out)]


def _inputs(frames, n_in=2, amp=0.8):
    return np.stack([lcg_noise_fast(frames, 41 + c, amp) for c in range(n_in)]).astype(np.float32)


def _codes(stream, bits):
    """A process_blocks_pcm stream -> int32 [G, frames]."""
    if bits == 16:
        return np.ascontiguousarray(stream.astype(np.int32).T)
    b = stream.astype(np.int32)
    v = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return np.ascontiguousarray(np.where(v >= 1 << 23, v - (1 << 24), v).T)


def _pair(bs, roots, **opts):
    """(the engine that delivers FLAC, its twin that delivers PCM), the same graph on both."""
    a, b = _hip(SR, bs, flac_frame=FF, **opts), _hip(SR, bs, **opts)
    assert a.render(*roots())["result"] == 0 and b.render(*roots())["result"] == 0
    return a, b


def _whole(rt, x, S, G, frames, bits, seed, **kw):
    """One call and the flush: per stream the bytes, and the call's statistics."""
    streams, stats = rt.process_blocks_flac(x, S, G, frames, bits, dither_seed=seed, **kw)
    tail = rt.flac_flush()
    return [a + b for a, b in zip(streams, tail)], stats


def _same_as_pcm(flac_streams, pcm_streams, bits, G, rate=44100):
    from elementary_amd.runtime import flac_encode
    for s, (data, pcm) in enumerate(zip(flac_streams, pcm_streams)):
        want = _codes(pcm, bits)
        frames, chans = ref.decode_frames(data, {"rate": rate, "bps": bits})
        assert all(f["bps"] == bits and f["rate"] == rate and len(f["channels"]) == G for f in frames)
        assert [f["number"] for f in frames] == list(range(len(frames)))
        assert all(f["blocksize"] == FF for f in frames[:-1]) and sum(f["blocksize"] for f in frames) == want.shape[1]
        got = np.array(chans, dtype=np.int64)
        assert got.shape == want.shape and np.array_equal(got, want), (s, int((got != want).sum()))
        twin, _ = flac_encode(want, bits=bits, flac_frame=FF, sample_rate=rate)      # GPU and host: the same bytes
        assert data == twin, (s, len(data), len(twin))


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_decoded_samples_are_process_pcms_codes(gpu_required, G, bits):
    """Two streams of G channels, 4 FLAC frames and 37 frames in sets of 8 blocks of 64 (a FLAC frame every half set), without and
    with dither; the statistics are the pack kernel's."""
    bs, n_out, frames = 64, 2 * G, 4 * FF + 37
    a, b = _pair(bs, lambda: _roots(n_out), batch_blocks=8)
    for k, seed in enumerate((None, 4321)):
        x = np.roll(_inputs(frames), 500 * k, axis=1)
        t0 = b.sample_time
        pcm, pst, _ = b.process_blocks_pcm(x, 2, G, frames, "s%d" % bits, dither_seed=seed)
        got, fst = _whole(a, x, 2, G, frames, bits, seed, sample_time=t0)
        a.sample_time = b.sample_time
        _same_as_pcm(got, pcm, bits, G)
        assert np.array_equal(fst["peak"].view(np.uint32), pst["peak"].view(np.uint32))
        assert np.array_equal(fst["over"], pst["over"]) and np.array_equal(fst["nonfinite"], pst["nonfinite"]) and int(pst["over"].sum()) > 0
        info = a.flac_read()
        assert info["flushed"] and info["stream_frames"] == [5, 5] and info["total_samples"] == [frames, frames] and info["bits"] == bits
        assert [int(v.sum()) for v in info["frame_bytes"]] == [len(d) for d in got]
        a.flac_reset()


@pytest.mark.parametrize("opts,rate", [({"resample_rate": 48000}, 48000), ({"limiter_gain_db": 6.0, "limiter": 1}, 44100)])
def test_behind_the_converter_and_the_limiter(gpu_required, opts, rate):
    """The encoder stands where the pack kernel stands: behind the delivery-rate converter, behind the limiter."""
    bs, G, frames = 350, 2, 5 * FF + 99
    a, b = _pair(bs, lambda: _roots(2 * G), batch_blocks=3, **opts)
    x = _inputs(frames)
    pcm, _, _ = b.process_blocks_pcm(x, 2, G, frames, "s24", dither_seed=7)
    got, _ = _whole(a, x, 2, G, frames, 24, 7)
    _same_as_pcm(got, pcm, 24, G, rate)
    assert a.flac_read()["sample_rate"] == rate


def _graph_signals():
    return {
        "const": lambda: [el.const({"value": 0.25}), el.const({"value": -1.0})],
        "ramp": lambda: [el.phasor(10.0), el.phasor(441.0)],
        "cycle": lambda: [el.cycle(440.0), el.mul(0.5, el.cycle(1000.0))],
        "noise": lambda: [el.noise({"seed": 3}), el.mul(0.01, el.noise({"seed": 4}))],
        "equal": lambda: [el.cycle(440.0), el.cycle(440.0)],
    }


@pytest.mark.parametrize("name", ["const", "ramp", "cycle", "noise", "equal"])
def test_gpu_bytes_equal_the_host_twins(gpu_required, name):
    """Signals a graph can produce, as one two-channel stream and as two mono streams, 16 bits: frame for frame the twin's bytes."""
    bs, frames = 64, 5 * FF + 50           # (the roots fade in over 20 ms, 882 frames: the last two FLAC frames lie behind that)
    for S, G in ((1, 2), (2, 1)):
        a, b = _pair(bs, _graph_signals()[name], batch_blocks=5)
        pcm, _, _ = b.process_blocks_pcm(None, S, G, frames, "s16")
        got, _ = _whole(a, None, S, G, frames, 16, None)
        _same_as_pcm(got, pcm, 16, G)
        f0 = ref.decode_frames(got[0], {"rate": 44100, "bps": 16})[0]
        if name == "equal" and G == 2:
            assert all(f["assignment"] in (8, 10) and f["subframes"][1]["kind"] == "CONSTANT" for f in f0[1:])       # (behind the roots' fade-in)
        if name == "const":
            assert all(sub["kind"] == "CONSTANT" for f in f0[-2:] for sub in f["subframes"])


def test_bytes_do_not_depend_on_the_cut(gpu_required):
    """One call = calls of 1, 37, 350 and the rest = launch sets of 1, 3 and 15 blocks."""
    bs, G, frames = 64, 2, 5 * FF + 101
    x = _inputs(frames)
    want = None
    for batch, cuts in ((15, ()), (15, (64, 128, 448)), (1, ()), (3, ())):
        a = _hip(SR, bs, flac_frame=FF, batch_blocks=batch)
        assert a.render(*_roots(2 * G))["result"] == 0
        parts, at = [b"", b""], 0
        for end in list(cuts) + [frames]:            # (calls hold whole blocks, but their last: 64 = 1 block, ... the rest)
            s, _ = a.process_blocks_flac(x[:, at:end], 2, G, end - at, 16, dither_seed=11)
            parts = [p + q for p, q in zip(parts, s)]
            at = end
        parts = [p + q for p, q in zip(parts, a.flac_flush())]
        if want is None:
            want = parts
            b = _hip(SR, bs)
            assert b.render(*_roots(2 * G))["result"] == 0
            _same_as_pcm(want, b.process_blocks_pcm(x, 2, G, frames, "s16", dither_seed=11)[0], 16, G)
        assert parts == want, (batch, cuts)


def test_calls_of_1_37_350_frames_through_the_renderer_with_a_scope_attached(gpu_required):
    """OfflineRenderer.process_flac with a scope listener walks relay windows; the bytes are one call's. A call of 1 and one of 37
    frames end inside a block: the next call starts a new block, as with process_pcm."""
    bs = 64

    def core(listen):
        c = OfflineRenderer(lambda s, k: _hip(s, k, flac_frame=FF, batch_blocks=15))
        c.initialize(num_input_channels=1, num_output_channels=2, sample_rate=SR, block_size=bs)
        x = el.in_({"channel": 0})
        c.render(el.scope({"name": "sc", "size": 256}, el.mul(0.9, x)), el.mul(-0.5, x))
        log = []
        if listen:
            c.on("scope", log.append)
        return c, log
    listening, log = core(True)
    frames = listening.runtime.event_window_blocks() * bs + 3 * FF + 20            # a relay window and a bit: two engine calls
    x = _inputs(frames, 1)
    plain, _ = core(False)
    want, _ = plain.process_flac([x[0]], 1, 2, frames, 16, dither_seed=5)
    want = [a + b for a, b in zip(want, plain.flac_flush())]
    got, _ = listening.process_flac([x[0]], 1, 2, frames, 16, dither_seed=5)
    got = [a + b for a, b in zip(got, listening.flac_flush())]
    assert got == want and len(log) > 4
    chans = ref.decode_frames(got[0], {"rate": 44100, "bps": 16})[1]
    assert len(chans) == 2 and len(chans[0]) == frames
    # ragged calls: 1, 37, 350 frames and the rest, each from a block boundary of the render
    rt = _hip(SR, bs, flac_frame=FF, batch_blocks=15)
    tw = _hip(SR, bs)
    for r in (rt, tw):
        assert r.render(el.mul(0.9, el.in_({"channel": 0})), el.mul(-0.5, el.in_({"channel": 0})))["result"] == 0
    data, codes = b"", []
    frames = 4 * FF + 20
    for n in (1, 37, 350, frames):
        seg = x[:, :n]
        data += rt.process_blocks_flac(seg, 1, 2, n, 16, dither_seed=5)[0][0]
        codes.append(_codes(tw.process_blocks_pcm(seg, 1, 2, n, "s16", dither_seed=5)[0][0], 16))
        rt.sample_time = tw.sample_time
    data += rt.flac_flush()[0]
    assert np.array_equal(np.array(ref.decode_frames(data, {"rate": 44100, "bps": 16})[1]), np.concatenate(codes, axis=1))


@pytest.mark.parametrize("open_frames", [1, 255])
def test_flush_reset_and_refusals(gpu_required, open_frames):
    from elementary_amd.runtime import ElemHipError
    bs, frames = 64, 2 * FF + open_frames
    a, b = _pair(bs, lambda: _roots(2), batch_blocks=4)
    x = _inputs(frames)
    pcm = b.process_blocks_pcm(x, 1, 2, frames, "s16")[0]
    body, _ = a.process_blocks_flac(x, 1, 2, frames, 16)
    assert len(ref.decode_frames(body[0])[0]) == 2 and a.flac_read()["total_samples"] == [2 * FF]
    tail = a.flac_flush()
    f, _ = ref.decode_frame(tail[0])
    assert f["blocksize"] == open_frames and f["number"] == 2
    _same_as_pcm([body[0] + tail[0]], pcm, 16, 2)
    with pytest.raises(ElemHipError) as e:                     # closed until the reset
        a.process_blocks_flac(x, 1, 2, frames, 16)
    assert e.value.code == 6
    with pytest.raises(ElemHipError) as e:
        a.flac_flush()
    assert e.value.code == 6
    a.flac_reset()
    again, _ = a.process_blocks_flac(x[:, :FF], 1, 2, FF, 16)
    assert ref.decode_frame(again[0])[0]["number"] == 0 and a.flac_read()["stream_frames"] == [1]
    with pytest.raises(ElemHipError) as e:                     # another shape inside a programme
        a.process_blocks_flac(x[:, :FF], 2, 1, FF, 16)
    assert e.value.code == 6
    with pytest.raises(ElemHipError) as e:
        a.set_option("flac_frame", 512)
    a.flac_reset()
    c = _hip(SR, bs)
    assert c.render(*_roots(9))["result"] == 0
    with pytest.raises(ElemHipError) as e:                     # nine channels in one stream
        c.process_blocks_flac(x[:, :FF], 1, 9, FF, 16)
    assert e.value.code == 8
    for key, bad in (("flac_frame", 300), ("flac_bits", 20)):
        with pytest.raises(ElemHipError):
            c.set_option(key, bad)


def test_frame_numbers_cross_the_two_byte_coding(gpu_required):
    """200 FLAC frames of one channel: numbers 128 .. 199 take two bytes, and a frame of 4096 on another engine."""
    bs, frames = 350, 200 * FF
    a, b = _pair(bs, lambda: [el.mul(0.3, el.in_({"channel": 0}))], batch_blocks=64)
    x = _inputs(frames, 1)
    pcm = b.process_blocks_pcm(x, 1, 1, frames, "s16", dither_seed=1)[0]
    got, _ = _whole(a, x, 1, 1, frames, 16, 1)
    _same_as_pcm(got, pcm, 16, 1)
    fr = ref.decode_frames(got[0])[0]
    assert len(fr) == 200 and fr[127]["header_bytes"] + 1 == fr[128]["header_bytes"]
    big = _hip(SR, bs, batch_blocks=64)
    assert big.render(el.mul(0.3, el.in_({"channel": 0})))["result"] == 0 and big.flac_read()["flac_frame"] == 4096
    n = 4096 + 300
    got = _whole(big, x[:, :n], 1, 1, n, 24, None)[0][0]
    fr, chans = ref.decode_frames(got)
    assert [f["blocksize"] for f in fr] == [4096, 300]
    tw = _hip(SR, bs)
    assert tw.render(el.mul(0.3, el.in_({"channel": 0})))["result"] == 0
    assert np.array_equal(np.array(chans), _codes(tw.process_blocks_pcm(x[:, :n], 1, 1, n, "s24")[0][0], 24))


def test_host_encoded_fallback_for_taps_under_a_sliced_block(gpu_required):
    """A tap graph at host block 1024 renders host block by host block through process(): its floats are on the host, where the
    header's scalar twin quantises and encodes them — the same bytes; the open frame still travels to the device and back, so a
    programme may go on from such a call into a launch-set call of another graph's."""
    bs, G = 1024, 2
    roots = lambda: [el.tapOut({"name": "fb"}, el.add(el.mul(0.6, el.in_({"channel": 0})), el.mul(0.5, el.tapIn({"name": "fb"})))),
                     el.mul(0.9, el.in_({"channel": 1}))]
    a, b = _hip(48000.0, bs, flac_frame=FF), _hip(48000.0, bs)
    assert a.render(*roots())["result"] == 0 and b.render(*roots())["result"] == 0
    data, pcm = b"", []
    for n in (1024 + 100, 1024 + 211):               # both calls end inside a FLAC frame (and inside a host block)
        x = _inputs(n)
        data += a.process_blocks_flac(x, 1, G, n, 24, dither_seed=3)[0][0]
        pcm.append(b.process_blocks_pcm(x, 1, G, n, "s24", dither_seed=3)[0][0])
    assert a.flac_read()["total_samples"] == [(2 * 1024 + 311) // FF * FF]
    data += a.flac_flush()[0]
    _same_as_pcm([data], [np.concatenate(pcm)], 24, G, 48000)
    assert a.stats()["batch_launches"] == 0


def _tone_file(path, amp, seconds, rate=48000):
    from elementary_amd.wav import WavWriter
    n = int(seconds * rate)
    t = np.arange(n)
    env = np.clip(np.minimum(t, n - 1 - t) / (0.25 * rate), 0.0, 1.0)
    x = np.stack([amp * env * np.sin(2.0 * np.pi * 1000.0 * t / rate), 0.8 * amp * env * np.sin(2.0 * np.pi * 440.0 * t / rate + 1.0)]).astype(np.float32)
    w = WavWriter(str(path), "f32", 2, rate)
    w.write(np.ascontiguousarray(x.T))
    w.close()
    return x


def test_files_decode(gpu_required, tmp_path):
    """write_flac and process_wav(out_fmt='flac16') against write_wav / process_wav in s16: the files hold the same samples."""
    import wave
    bs, frames = 350, 9 * FF + 123

    def core(**kw):
        c = OfflineRenderer(lambda s, k: _hip(s, k, flac_frame=FF, batch_blocks=4))
        c.initialize(num_input_channels=2, num_output_channels=4, sample_rate=SR, block_size=bs, **kw)
        c.render(*_roots(4))
        return c
    x = _inputs(frames)
    for kw in ({}, {"output_sample_rate": 48000.0, "limiter": {"gain_db": 3.0}}):
        core(**kw).write_flac(str(tmp_path / "f{}.flac"), list(x), frames, bits=16, channels_per_stream=2, dither_seed=9, chunk_frames=4 * bs)
        core(**kw).write_wav(str(tmp_path / "w{}.wav"), list(x), frames, "s16", channels_per_stream=2, dither_seed=9, chunk_frames=4 * bs)
        for s in range(2):
            info, fr, chans = ref.decode_file((tmp_path / f"f{s}.flac").read_bytes())
            with wave.open(str(tmp_path / f"w{s}.wav")) as w:
                want = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").reshape(-1, 2).T
                assert info["rate"] == w.getframerate()
            assert info["md5"] == bytes(16) and info["total"] == want.shape[1] and info["min_frame"] > 0
            assert np.array_equal(np.array(chans), want), (kw, s)
    # WAV in, FLAC out
    _tone_file(tmp_path / "in.wav", 0.4, 0.25, rate=44100)
    for fmt, out in (("flac16", "o.flac"), ("s16", "o.wav")):
        c = OfflineRenderer(lambda s, k: _hip(s, k, flac_frame=FF, batch_blocks=4))
        c.initialize(num_input_channels=2, num_output_channels=2, sample_rate=SR, block_size=bs)
        c.render(el.mul(0.5, el.in_({"channel": 0})), el.mul(0.7, el.in_({"channel": 1})))
        c.process_wav(str(tmp_path / "in.wav"), str(tmp_path / out), fmt)
    info, fr, chans = ref.decode_file((tmp_path / "o.flac").read_bytes())
    with wave.open(str(tmp_path / "o.wav")) as w:
        want = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").reshape(-1, 2).T
    assert np.array_equal(np.array(chans), want) and info["total"] == int(0.25 * 44100)


def test_master_wav_writes_a_flac_file_with_the_reported_loudness(gpu_required, tmp_path):
    """master_wav(fmt='flac24'): the decoded file, metered by the float64 reference, has the loudness the call reports. The engine
    meters the floats with the limiter's latency (under 2 ms of silence) in front, the reference the 24-bit codes from frame 0 on: the
    grids of 100 ms sub-blocks differ by that shift and the samples by 2^-24 of full scale, which the existing master test bounds by
    0.01 LU for the same shift."""
    from elementary_amd.master import master_wav
    x = _tone_file(tmp_path / "in.wav", 0.1, 1.5)
    got = master_wav(lambda s, k: _hip(s, k, batch_blocks=64), tmp_path / "in.wav", tmp_path / "out.flac", target_lufs=-16.0, ceiling_dbtp=-1.0, fmt="flac24")
    info, fr, chans = ref.decode_file((tmp_path / "out.flac").read_bytes())
    assert info["rate"] == 48000 and info["bps"] == 24 and info["channels"] == 2 and info["total"] == x.shape[1] and info["max_block"] == 4096
    y = np.array(chans, dtype=np.float64) / float(1 << 23)
    lufs = lref.gate(lref.mean_squares(y, 48000.0))["integrated"]
    print(got["output_lufs"], lufs)
    assert abs(lufs - got["output_lufs"]) < 0.01 and abs(got["output_lufs"] - (-16.0)) < 0.01
