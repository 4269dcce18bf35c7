"""The STREAMINFO MD5 of FLAC delivery computed on the GPU (option "flac_md5"; elementary_amd/csrc/flac_md5.hip): after the flush,
flac_read()["md5"][s] is hashlib.md5 of the bytes the twin engine's process_blocks_pcm delivers for stream s in s16 / s24 — and of
the samples tests/flac_reference.py decodes from the delivered stream, repacked. The oracle is exact: nothing here has a tolerance.
Small shapes in the style of test_gpu_flac.py: engine blocks of 64, FLAC frames of 256, renders of a few FLAC frames."""
import hashlib

import numpy as np
import pytest

import flac_reference as ref
from elementary_amd import el
from elementary_amd.offline import OfflineRenderer
from helpers import lcg_noise_fast

pytestmark = pytest.mark.gpu
SR = 44100.0
FF = 256
GAINS = (1.7, 0.9, -1.3, 0.5, 1.1, -0.7, 0.3, 1.9, -0.2, 0.8, 1.4, -1.0, 0.6, -0.4, 1.2, 0.1)
EMPTY = bytes.fromhex("d41d8cd98f00b204e9800998ecf8427e")


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


def _pair(bs, roots, **opts):
    """(the engine that delivers FLAC with its MD5, its twin that delivers PCM), the same graph on both."""
    a, b = _hip(SR, bs, flac_frame=FF, flac_md5=1, **opts), _hip(SR, bs, **opts)
    assert a.render(*roots())["result"] == 0 and b.render(*roots())["result"] == 0
    return a, b


def _md5(stream):
    """A process_blocks_pcm stream (int16 [frames, G] or uint8 [frames, G, 3]) -> the digest of its bytes."""
    return hashlib.md5(np.ascontiguousarray(stream).tobytes()).digest()


def _repacked(data, bits, rate=44100):
    """The delivered FLAC frames decoded by the reference decoder and packed again as s16 / s24 -> their digest."""
    _, chans = ref.decode_frames(data, {"rate": rate, "bps": bits})
    a = np.ascontiguousarray(np.array(chans, dtype=np.int64).astype(np.int32).T)
    if bits == 16:
        return hashlib.md5(a.astype("<i2").tobytes()).digest()
    return hashlib.md5(np.ascontiguousarray(a.astype("<i4").view(np.uint8).reshape(a.shape[0], a.shape[1], 4)[:, :, :3]).tobytes()).digest()


def test_option_off_reports_nothing(gpu_required):
    """Without the option: state 0 and zero digests, before and after the flush."""
    a = _hip(SR, 64, flac_frame=FF, batch_blocks=8)
    assert a.render(*_roots(2))["result"] == 0
    x = _inputs(2 * FF + 9)
    a.process_blocks_flac(x, 1, 2, x.shape[1], 16)
    assert a.flac_read()["md5_state"] == 0 and a.flac_read()["md5"] == [bytes(16)]
    a.flac_flush()
    assert a.flac_read()["md5_state"] == 0 and a.flac_read()["md5"] == [bytes(16)]


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_digest_is_md5_of_process_pcms_bytes(gpu_required, G, bits):
    """Two streams of G channels, 4 FLAC frames and 37 frames in sets of 8 blocks of 64, without and with dither. G = 8 at 24 bits
    puts 192 MD5 blocks into a set (three chunks), G = 3 at 24 bits 72 blocks of 9-byte frames."""
    bs, n_out, frames = 64, 2 * G, 4 * FF + 37
    a, b = _pair(bs, lambda: _roots(n_out), batch_blocks=8)
    for k, seed in enumerate((None, 4321)):
        x = np.roll(_inputs(frames), 500 * k, axis=1)
        t0 = b.sample_time
        pcm, _, _ = b.process_blocks_pcm(x, 2, G, frames, "s%d" % bits, dither_seed=seed)
        body, _ = a.process_blocks_flac(x, 2, G, frames, bits, dither_seed=seed, sample_time=t0)
        a.sample_time = b.sample_time
        got = a.flac_read()
        assert got["md5_state"] == 1 and got["md5"] == [bytes(16)] * 2
        tail = a.flac_flush()
        got = a.flac_read()
        assert got["md5_state"] == 2
        for s in range(2):
            print(G, bits, seed, s, got["md5"][s].hex(), _md5(pcm[s]).hex())
            assert got["md5"][s] == _md5(pcm[s]), (s, seed)
            assert got["md5"][s] == _repacked(body[s] + tail[s], bits), (s, seed)
        assert got["md5"][0] != got["md5"][1]
        a.flac_reset()


# mono s24: 64, 43, 61, 40, 21 frames leave 0, 1, 55, 56, 63 bytes behind the last whole block; mono s16: 32 and 28 leave 0 and 56; 5: under a block
@pytest.mark.parametrize("bits,frames", [(24, 64), (24, 43), (24, 61), (24, 40), (24, 21), (16, 32), (16, 28), (16, 5)])
def test_padding_residues(gpu_required, bits, frames):
    a, b = _pair(64, lambda: _roots(1, 1), batch_blocks=8)
    x = _inputs(frames, 1)
    pcm, _, _ = b.process_blocks_pcm(x, 1, 1, frames, "s%d" % bits, dither_seed=5)
    a.process_blocks_flac(x, 1, 1, frames, bits, dither_seed=5)
    a.flac_flush()
    got = a.flac_read()
    assert got["md5_state"] == 2 and got["md5"] == [_md5(pcm[0])], (got["md5"][0].hex(), _md5(pcm[0]).hex())


def test_a_programme_whose_frames_were_all_dropped(gpu_required):
    a, _ = _pair(64, lambda: _roots(1, 1), batch_blocks=8)
    x = _inputs(300, 1)
    body, _ = a.process_blocks_flac(x, 1, 1, 300, 16, drop=300)
    assert body == [b""] and a.flac_read()["md5_state"] == 1
    assert a.flac_flush() == [b""]
    got = a.flac_read()
    assert got["md5_state"] == 2 and got["md5"] == [EMPTY] and got["total_samples"] == [0]


def test_digest_does_not_depend_on_the_cut(gpu_required):
    """One call = calls cut at 64, 128 and 448 = launch sets of 1, 3 and 15 blocks: one digest, the PCM twin's."""
    bs, G, frames = 64, 2, 5 * FF + 101
    x = _inputs(frames)
    b = _hip(SR, bs)
    assert b.render(*_roots(2 * G))["result"] == 0
    want = [_md5(p) for p in b.process_blocks_pcm(x, 2, G, frames, "s16", dither_seed=11)[0]]
    for batch, cuts in ((15, ()), (15, (64, 128, 448)), (1, ()), (3, ())):
        a = _hip(SR, bs, flac_frame=FF, flac_md5=1, batch_blocks=batch)
        assert a.render(*_roots(2 * G))["result"] == 0
        at = 0
        for end in list(cuts) + [frames]:
            a.process_blocks_flac(x[:, at:end], 2, G, end - at, 16, dither_seed=11)
            at = end
        a.flac_flush()
        assert a.flac_read()["md5"] == want, (batch, cuts)


@pytest.mark.parametrize("opts,rate", [({"resample_rate": 48000}, 48000), ({"limiter_gain_db": 6.0, "limiter": 1}, 44100)])
def test_behind_the_converter_and_the_limiter(gpu_required, opts, rate):
    bs, G, frames = 350, 2, 5 * FF + 99
    a, b = _pair(bs, lambda: _roots(2 * G), batch_blocks=3, **opts)
    x = _inputs(frames)
    pcm, _, _ = b.process_blocks_pcm(x, 2, G, frames, "s24", dither_seed=7)
    body, _ = a.process_blocks_flac(x, 2, G, frames, 24, dither_seed=7)
    tail = a.flac_flush()
    got = a.flac_read()
    assert got["md5_state"] == 2 and got["sample_rate"] == rate
    for s in range(2):
        assert got["md5"][s] == _md5(pcm[s]) == _repacked(body[s] + tail[s], 24, rate)


def test_host_encoded_fallback_and_on_into_a_launch_set(gpu_required):
    """The tap graph at host block 1024 renders block by block on the host, where the header's serial walk hashes the codes; the records
    travel to the device and back with the open frame. Then the same programme goes on in a launch-set call of another graph."""
    bs, G = 1024, 2
    taps = lambda: [el.tapOut({"name": "fb"}, el.add(el.mul(0.6, el.in_({"channel": 0})), el.mul(0.5, el.tapIn({"name": "fb"})))),
                    el.mul(0.9, el.in_({"channel": 1}))]
    a, b = _hip(48000.0, bs, flac_frame=FF, flac_md5=1, batch_blocks=8), _hip(48000.0, bs)
    assert a.render(*taps())["result"] == 0 and b.render(*taps())["result"] == 0
    pcm = []
    for n in (1024 + 100, 1024 + 211):
        x = _inputs(n)
        a.process_blocks_flac(x, 1, G, n, 24, dither_seed=3)
        pcm.append(b.process_blocks_pcm(x, 1, G, n, "s24", dither_seed=3)[0][0])
    assert a.stats()["batch_launches"] == 0 and a.flac_read()["md5_state"] == 1
    # a twin programme that flushes here
    c = _hip(48000.0, bs, flac_frame=FF, flac_md5=1)
    assert c.render(*taps())["result"] == 0
    for n in (1024 + 100, 1024 + 211):
        c.process_blocks_flac(_inputs(n), 1, G, n, 24, dither_seed=3)
    c.flac_flush()
    assert c.flac_read()["md5"] == [_md5(np.concatenate(pcm))]
    # ... and `a` goes on with another graph. The tap nodes live until a render sequence without them is current and they are
    # collected: a call block by block while the tap roots fade out, other roots rendered once more, one more host block, gc() —
    # and then a call in launch sets of 8 blocks
    for step, n in enumerate((2 * 1024 + 100, 1024, 8 * 1024)):
        if step < 2:        # (two different graphs: rendering the same roots again would change nothing)
            for r in (a, b):
                assert r.render(*[el.mul(0.4 + 0.3 * step + 0.1 * c, el.in_({"channel": c})) for c in range(G)])["result"] == 0
        else:
            a.gc(), b.gc()
        assert a.stats()["batch_launches"] == 0
        x = _inputs(n)
        a.sample_time = b.sample_time
        a.process_blocks_flac(x, 1, G, n, 24, dither_seed=3)
        pcm.append(b.process_blocks_pcm(x, 1, G, n, "s24", dither_seed=3)[0][0])
    assert a.stats()["batch_launches"] > 0
    a.flac_flush()
    assert a.flac_read()["md5"] == [_md5(np.concatenate(pcm))]


def test_programme_rules(gpu_required):
    from elementary_amd.runtime import ElemHipError
    bs, frames = 64, 2 * FF + 50
    a, b = _pair(bs, lambda: _roots(2), batch_blocks=4)
    x = _inputs(frames)
    a.process_blocks_flac(x, 1, 2, frames, 16)
    with pytest.raises(ElemHipError) as e:                     # another value inside an open programme
        a.set_option("flac_md5", 0)
    assert e.value.code == 6
    a.set_option("flac_md5", 1)                                # (the programme's own value is no change)
    a.flac_flush()
    first = a.flac_read()["md5"]
    assert first == [_md5(b.process_blocks_pcm(x, 1, 2, frames, "s16")[0][0])]
    a.flac_reset()
    assert a.flac_read()["md5_state"] == 0
    # the second render's digest is the second render's alone
    y = _inputs(frames)[:, ::-1].copy()
    a.sample_time = b.sample_time
    a.process_blocks_flac(y, 1, 2, frames, 16)
    a.flac_flush()
    second = a.flac_read()["md5"]
    assert second == [_md5(b.process_blocks_pcm(y, 1, 2, frames, "s16")[0][0])] and second != first
    a.flac_reset()
    a.set_option("flac_md5", 0)                                # accepted after the reset
    a.process_blocks_flac(x, 1, 2, frames, 16)
    a.flac_flush()
    assert a.flac_read()["md5_state"] == 0


def _file_verifies(path):
    info, _, chans = ref.decode_file(path.read_bytes())
    a = np.ascontiguousarray(np.array(chans, dtype=np.int64).astype(np.int32).T)
    if info["bps"] == 16:
        own = hashlib.md5(a.astype("<i2").tobytes()).digest()
    else:
        own = hashlib.md5(np.ascontiguousarray(a.astype("<i4").view(np.uint8).reshape(a.shape[0], a.shape[1], 4)[:, :, :3]).tobytes()).digest()
    return info["md5"], own


def _tone_file(path, amp, seconds, rate=44100):
    from elementary_amd.wav import WavWriter
    n = int(seconds * rate)
    t = np.arange(n)
    x = np.stack([amp * np.sin(2.0 * np.pi * 1000.0 * t / rate), 0.8 * amp * np.sin(2.0 * np.pi * 440.0 * t / rate + 1.0)]).astype(np.float32)
    w = WavWriter(str(path), "f32", 2, rate)
    w.write(np.ascontiguousarray(x.T))
    w.close()


def test_files_verify(gpu_required, tmp_path):
    """write_flac and process_wav(out_fmt='flac24') on an engine factory with flac_md5 = 1: the files announce the MD5 of their own
    samples; the same factory without the option still writes zeros."""
    bs, frames = 350, 9 * FF + 123

    def core(md5, n_out=4, **kw):
        opts = {"flac_md5": 1} if md5 else {}
        c = OfflineRenderer(lambda s, k: _hip(s, k, flac_frame=FF, batch_blocks=4, **opts))
        c.initialize(num_input_channels=2, num_output_channels=n_out, sample_rate=SR, block_size=bs, **kw)
        return c
    x = _inputs(frames)
    for i, kw in enumerate(({}, {"output_sample_rate": 48000.0, "limiter": {"gain_db": 3.0}})):
        for md5 in (True, False):
            c = core(md5, **kw)
            c.render(*_roots(4))
            c.write_flac(str(tmp_path / ("f%d%d_{}.flac" % (i, md5))), list(x), frames, bits=16, channels_per_stream=2, dither_seed=9, chunk_frames=4 * bs)
            for s in range(2):
                announced, own = _file_verifies(tmp_path / ("f%d%d_%d.flac" % (i, md5, s)))
                assert announced == (own if md5 else bytes(16)) and own != bytes(16), (kw, md5, s)
    _tone_file(tmp_path / "in.wav", 0.4, 0.25)
    for md5 in (True, False):
        c = core(md5, n_out=2)
        c.render(el.mul(0.5, el.in_({"channel": 0})), el.mul(0.7, el.in_({"channel": 1})))
        c.process_wav(str(tmp_path / "in.wav"), str(tmp_path / ("o%d.flac" % md5)), "flac24")
        announced, own = _file_verifies(tmp_path / ("o%d.flac" % md5))
        assert announced == (own if md5 else bytes(16)) and own != bytes(16), md5
