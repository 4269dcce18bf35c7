"""LPC subframes in GPU FLAC delivery (option flac_lpc_order; elementary_amd/csrc/flac_lpc.h, elemhip_flac_encode<true>). The contract is
FLAC delivery's own: the stream decodes — with tests/flac_reference.py, written from the RFC — to the codes process_blocks_pcm delivers
for the same render, and its bytes are those of the scalar twin (flac_encode(codes, lpc_order=P)) fed with those codes. Engine blocks
of 64 frames, FLAC frames of 256 unless said otherwise; one input is a bright signal (5 kHz + 9 kHz + noise 60 dB below, where LPC
pays), the other white noise (where nothing pays), so LPC, FIXED and VERBATIM subframes and the stereo modes appear."""
import math

import numpy as np
import pytest

import flac_reference as ref
from elementary_amd import el
from elementary_amd.offline import OfflineRenderer
from helpers import lcg_noise_fast

pytestmark = pytest.mark.gpu
SR = 44100.0
FF = 256
GAINS = (0.9, 0.8, -0.7, 0.5, 1.0, -0.6, 0.3, 0.95, 0.85, -0.4, 0.6, 0.2, -0.9, 0.7, 0.45, -0.3)


def _hip(sr, bs, **opts):
    from elementary_amd.runtime import Runtime
    rt = Runtime(sr, bs, device=0)
    for k, v in opts.items():
        rt.set_option(k, v)
    return rt


def _roots(n_out, n_in=2):
    """Channel c = in[c % n_in] scaled; in the second half of the channels (the second stream of two) an odd channel is nearly its left
    neighbour instead — 0.98 of it and a little of the noise — so that a stereo stream there has a small side channel."""
    def root(c):
        g = GAINS[c % len(GAINS)]
        if c % 2 == 1 and c >= max(n_out // 2, 2):
            return el.add(el.mul(0.98 * GAINS[(c - 1) % len(GAINS)], el.in_({"channel": (c - 1) % n_in})), el.mul(0.01, el.in_({"channel": 1})))
        return el.mul(g, el.in_({"channel": c % n_in}))
    return [root(c) for c in range(n_out)]


def _inputs(frames):
    """Channel 0: 0.3 sin 5 kHz + 0.2 sin 9 kHz at 44.1 kHz plus noise 60 dB below; channel 1: white noise."""
    i = np.arange(frames)
    bright = 0.3 * np.sin(2 * math.pi * 5000.0 * i / 44100.0) + 0.2 * np.sin(2 * math.pi * 9000.0 * i / 44100.0) + lcg_noise_fast(frames, 77, 1e-3)
    return np.stack([bright, lcg_noise_fast(frames, 42, 0.8)]).astype(np.float32)


def _codes(stream, bits):
    """A process_blocks_pcm stream -> int32 [G, frames]."""
    if bits == 16:
        return np.ascontiguousarray(stream.astype(np.int32).T)
    b = stream.astype(np.int32)
    v = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return np.ascontiguousarray(np.where(v >= 1 << 23, v - (1 << 24), v).T)


def _whole(rt, x, S, G, frames, bits, seed, **kw):
    streams, _ = rt.process_blocks_flac(x, S, G, frames, bits, dither_seed=seed, **kw)
    return [a + b for a, b in zip(streams, rt.flac_flush())]


def _check(flac_streams, pcm_streams, bits, G, order, ff=FF):
    """Decoded = the PCM codes; bytes = the twin's. Returns the subframe kinds and the channel assignments that occurred."""
    from elementary_amd.runtime import flac_encode
    kinds, modes = set(), set()
    for s, (data, pcm) in enumerate(zip(flac_streams, pcm_streams)):
        want = _codes(pcm, bits)
        frames, chans = ref.decode_frames(data, {"rate": 44100, "bps": bits})
        assert [f["number"] for f in frames] == list(range(len(frames)))
        assert all(f["blocksize"] == ff for f in frames[:-1]) and sum(f["blocksize"] for f in frames) == want.shape[1]
        got = np.array(chans, dtype=np.int64)
        assert got.shape == want.shape and np.array_equal(got, want), (s, int((got != want).sum()))
        twin, _ = flac_encode(want, bits=bits, flac_frame=ff, sample_rate=44100, lpc_order=order)
        assert data == twin, (s, len(data), len(twin))
        for f in frames:
            modes.add(f["assignment"])
            for sub in f["subframes"]:
                kinds.add(sub["kind"])
                assert sub["kind"] != "LPC" or sub["order"] in (order, (order + 1) // 2)
    return kinds, modes


@pytest.mark.parametrize("order", [8, 12])
@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_lpc_streams_decode_to_process_pcms_codes_and_equal_the_twin(gpu_required, G, bits, order):
    """Two streams of G channels, 4 FLAC frames and 37 frames in sets of 8 blocks. (Fails on an engine without the option.)"""
    bs, n_out, frames = 64, 2 * G, 4 * FF + 37
    a, b = _hip(SR, bs, flac_frame=FF, flac_lpc_order=order, batch_blocks=8), _hip(SR, bs, batch_blocks=8)
    assert a.render(*_roots(n_out))["result"] == 0 and b.render(*_roots(n_out))["result"] == 0
    x = _inputs(frames)
    pcm, _, _ = b.process_blocks_pcm(x, 2, G, frames, "s%d" % bits, dither_seed=4321)
    got = _whole(a, x, 2, G, frames, bits, 4321)
    kinds, modes = _check(got, pcm, bits, G, order)
    assert "LPC" in kinds and len(kinds) > 1, kinds
    info = a.flac_read()
    assert info["lpc_order"] == order and info["flushed"] and info["stream_frames"] == [5, 5]


def test_frames_of_4096_with_order_12(gpu_required):
    """Lane runs of 16 samples: two whole frames and 50 samples, one stereo stream, 16 bits."""
    bs, frames = 64, 2 * 4096 + 50
    a, b = _hip(SR, bs, flac_frame=4096, flac_lpc_order=12, batch_blocks=32), _hip(SR, bs, batch_blocks=32)
    assert a.render(*_roots(2))["result"] == 0 and b.render(*_roots(2))["result"] == 0
    x = _inputs(frames)
    pcm, _, _ = b.process_blocks_pcm(x, 1, 2, frames, "s16", dither_seed=3)
    kinds, _ = _check(_whole(a, x, 1, 2, frames, 16, 3), pcm, 16, 2, 12, ff=4096)
    assert "LPC" in kinds


def test_lpc_bytes_do_not_depend_on_the_cut(gpu_required):
    """One call = calls of 1 block, 37 frames' worth of blocks, 350 and the rest = launch sets of 1, 3 and 15 blocks."""
    bs, G, frames = 64, 2, 5 * FF + 101
    x = _inputs(frames)
    want = None
    for batch, cuts in ((15, ()), (15, (64, 128, 448)), (1, ()), (3, ())):
        a = _hip(SR, bs, flac_frame=FF, flac_lpc_order=8, batch_blocks=batch)
        assert a.render(*_roots(2 * G))["result"] == 0
        parts, at = [b"", b""], 0
        for end in list(cuts) + [frames]:
            s, _ = a.process_blocks_flac(x[:, at:end], 2, G, end - at, 16, dither_seed=11)
            parts = [p + q for p, q in zip(parts, s)]
            at = end
        parts = [p + q for p, q in zip(parts, a.flac_flush())]
        if want is None:
            want = parts
            b = _hip(SR, bs)
            assert b.render(*_roots(2 * G))["result"] == 0
            _check(want, b.process_blocks_pcm(x, 2, G, frames, "s16", dither_seed=11)[0], 16, G, 8)
        assert parts == want, (batch, cuts)
    # ragged calls of 1, 37 and 350 frames and the rest, each from a block boundary of the render: the decoded programme is the calls' codes
    rt, tw = _hip(SR, bs, flac_frame=FF, flac_lpc_order=8, batch_blocks=15), _hip(SR, bs)
    for r in (rt, tw):
        assert r.render(*_roots(2))["result"] == 0
    data, codes = b"", []
    for n in (1, 37, 350, 4 * FF + 20):
        seg = x[:, :n]
        data += rt.process_blocks_flac(seg, 1, 2, n, 16, dither_seed=5)[0][0]
        codes.append(_codes(tw.process_blocks_pcm(seg, 1, 2, n, "s16", dither_seed=5)[0][0], 16))
        rt.sample_time = tw.sample_time
    data += rt.flac_flush()[0]
    want = np.concatenate(codes, axis=1)
    assert np.array_equal(np.array(ref.decode_frames(data, {"rate": 44100, "bps": 16})[1]), want)
    from elementary_amd.runtime import flac_encode
    assert data == flac_encode(want, bits=16, flac_frame=FF, lpc_order=8)[0]


def test_order_0_is_the_default_and_changes_nothing(gpu_required):
    from elementary_amd.runtime import flac_encode
    bs, frames = 64, 3 * FF + 60
    x = _inputs(frames)
    out = []
    for opts in ({}, {"flac_lpc_order": 0}):
        a = _hip(SR, bs, flac_frame=FF, batch_blocks=8, **opts)
        assert a.render(*_roots(4))["result"] == 0 and a.flac_read()["lpc_order"] == 0
        out.append(_whole(a, x, 2, 2, frames, 24, 9))
    assert out[0] == out[1]
    b = _hip(SR, bs)
    assert b.render(*_roots(4))["result"] == 0
    pcm, _, _ = b.process_blocks_pcm(x, 2, 2, frames, "s24", dither_seed=9)
    for data, p in zip(out[0], pcm):
        assert data == flac_encode(_codes(p, 24), bits=24, flac_frame=FF)[0]          # elemhip_flac_encode's bytes, as before
        assert all(sub["kind"] != "LPC" for f in ref.decode_frames(data)[0] for sub in f["subframes"])


def test_the_programme_keeps_its_order(gpu_required):
    """Like flac_frame: another order is refused while a programme is open, and taken after the reset."""
    from elementary_amd.runtime import ElemHipError
    bs = 64
    a = _hip(SR, bs, flac_frame=FF, flac_lpc_order=8, batch_blocks=4)
    assert a.render(*_roots(2))["result"] == 0
    x = _inputs(FF + 10)
    a.process_blocks_flac(x, 1, 2, FF + 10, 16)
    for other in (0, 12):
        with pytest.raises(ElemHipError) as e:
            a.set_option("flac_lpc_order", other)
        assert e.value.code == 6
    a.set_option("flac_lpc_order", 8)                    # the programme's own value is no change
    assert a.flac_read()["lpc_order"] == 8
    for bad in (13, -1, 2.5):
        with pytest.raises(ElemHipError):
            a.set_option("flac_lpc_order", bad)
    a.flac_flush()
    a.flac_reset()
    a.set_option("flac_lpc_order", 12)
    data = _whole(a, x, 1, 2, FF + 10, 16, None)[0]
    assert a.flac_read()["lpc_order"] == 12
    assert any(sub["kind"] == "LPC" and sub["order"] in (6, 12) for f in ref.decode_frames(data)[0] for sub in f["subframes"])


def test_an_lpc_stream_fed_back_equals_its_samples_fed_as_s16(gpu_required):
    """The GPU decoder reads what the GPU encoder wrote: a pass-through graph fed the LPC stream as a FlacChunk gives bit for bit the
    floats it gives when fed the same samples as s16."""
    from elementary_amd.runtime import FlacChunk, flac_index
    bs, frames = 64, 4 * FF + 37
    a, b = _hip(SR, bs, flac_frame=FF, flac_lpc_order=8, batch_blocks=8), _hip(SR, bs, batch_blocks=8)
    assert a.render(*_roots(2))["result"] == 0 and b.render(*_roots(2))["result"] == 0
    x = _inputs(frames)
    data = _whole(a, x, 1, 2, frames, 16, 21)[0]
    pcm = b.process_blocks_pcm(x, 1, 2, frames, "s16", dither_seed=21)[0][0]
    assert any(sub["kind"] == "LPC" for f in ref.decode_frames(data)[0] for sub in f["subframes"])
    off, first = flac_index(data, 2, 16, FF)
    chunk = FlacChunk(np.frombuffer(data, dtype=np.uint8), off, first, 2, 16, int(first[-1]), 0, int(first[-1]))
    outs = []
    for feed, fmt in ((chunk, "flac"), (np.ascontiguousarray(pcm), "s16")):
        rt = _hip(SR, bs, batch_blocks=8)
        assert rt.render(el.in_({"channel": 0}), el.in_({"channel": 1}))["result"] == 0
        outs.append(rt.process_blocks_pcm_io([feed], fmt, 2, frames))
    assert outs[0].shape == outs[1].shape and np.array_equal(np.ascontiguousarray(outs[0]).view(np.uint8), np.ascontiguousarray(outs[1]).view(np.uint8))


def test_write_flac_with_the_option(gpu_required, tmp_path):
    bs, frames = 64, 6 * FF + 123
    c = OfflineRenderer(lambda s, k: _hip(s, k, flac_frame=FF, flac_lpc_order=8, batch_blocks=4))
    c.initialize(num_input_channels=2, num_output_channels=2, sample_rate=SR, block_size=bs)
    c.render(*_roots(2))
    w = OfflineRenderer(lambda s, k: _hip(s, k, batch_blocks=4))
    w.initialize(num_input_channels=2, num_output_channels=2, sample_rate=SR, block_size=bs)
    w.render(*_roots(2))
    x = _inputs(frames)
    c.write_flac(str(tmp_path / "f.flac"), list(x), frames, bits=16, channels_per_stream=2, dither_seed=9, chunk_frames=4 * bs)
    assert c.runtime.flac_read()["lpc_order"] == 8
    w.write_wav(str(tmp_path / "w.wav"), list(x), frames, "s16", channels_per_stream=2, dither_seed=9, chunk_frames=4 * bs)
    import wave
    info, fr, chans = ref.decode_file((tmp_path / "f.flac").read_bytes())
    with wave.open(str(tmp_path / "w.wav")) as f:
        want = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2").reshape(-1, 2).T
    assert info["total"] == frames and np.array_equal(np.array(chans), want)
    assert any(sub["kind"] == "LPC" for f in fr for sub in f["subframes"])


def test_host_encoded_fallback_takes_the_order_too(gpu_required):
    """A tap graph at host block 1024 renders host block by host block; its frames are encoded by the scalar twin on the host — with the
    programme's LPC order, so the bytes are those of flac_encode(codes, lpc_order=8) all the same."""
    bs, G = 1024, 2
    roots = lambda: [el.tapOut({"name": "fb"}, el.add(el.mul(0.6, el.in_({"channel": 0})), el.mul(0.5, el.tapIn({"name": "fb"})))),
                     el.mul(0.9, el.in_({"channel": 1}))]
    a, b = _hip(48000.0, bs, flac_frame=FF, flac_lpc_order=8), _hip(48000.0, bs)
    assert a.render(*roots())["result"] == 0 and b.render(*roots())["result"] == 0
    data, pcm = b"", []
    for n in (1024 + 100, 1024 + 211):
        x = _inputs(n)
        data += a.process_blocks_flac(x, 1, G, n, 24, dither_seed=3)[0][0]
        pcm.append(b.process_blocks_pcm(x, 1, G, n, "s24", dither_seed=3)[0][0])
    data += a.flac_flush()[0]
    from elementary_amd.runtime import flac_encode
    want = _codes(np.concatenate(pcm), 24)
    frames, chans = ref.decode_frames(data, {"rate": 48000, "bps": 24})
    assert np.array_equal(np.array(chans, dtype=np.int64), want)
    assert data == flac_encode(want, bits=24, flac_frame=FF, sample_rate=48000, lpc_order=8)[0]
    assert any(sub["kind"] == "LPC" for f in frames for sub in f["subframes"]) and a.stats()["batch_launches"] == 0
