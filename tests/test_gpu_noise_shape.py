"""Noise-shaped requantisation on the GPU (Runtime.noise_shape; elementary_amd/csrc/noise_shape.hip): the bytes of s16 / s24 / FLAC
delivery with shaping on are exactly the codes tests/noise_shape_reference.py computes from the floats the same call delivers
(want_float) — whatever the channel count, the grouping, the filter length, the cut into calls and launch sets, and the renderer
(launch sets or host block by host block). Nothing here has a tolerance. Small shapes in the style of test_gpu_flac_md5.py: engine
blocks of 64, sets of 8 blocks, FLAC frames of 256, renders of 4 * 256 + 37 frames, some channels beyond full scale."""
import hashlib

import numpy as np
import pytest

import flac_reference
import noise_shape_reference as ref
from elementary_amd import el
from elementary_amd import noise_shape as presets
from elementary_amd.runtime import ElemHipError, noise_shape_host
from helpers import lcg_noise_fast

pytestmark = pytest.mark.gpu
SR = 44100.0
FF = 256
FRAMES = 4 * FF + 37
GAINS = (1.7, 0.9, -1.3, 0.5, 1.1, -0.7, 0.3, 1.9, -0.2, 0.8, 1.4, -1.0, 0.6, -0.4, 1.2, 0.1)
TAPS = {1: presets.PRESETS["first"], 9: presets.PRESETS["fweighted9"], 12: presets.PRESETS["fweighted9"] + [0.31, -0.17, 0.05]}


def _hip(sr, bs, **opts):
    from elementary_amd.runtime import Runtime
    rt = Runtime(sr, bs, device=0)
    for k, v in opts.items():
        rt.set_option(k, v)
    return rt


def _roots(n_out, n_in=2):
    """Channel c = in[c % n_in] scaled by a constant (some beyond full scale: they clip)."""
    return [el.mul(GAINS[c % len(GAINS)] * (1.0 + 0.01 * (c // len(GAINS))), el.in_({"channel": c % n_in})) for c in range(n_out)]


def _inputs(frames, n_in=2, amp=0.8):
    return np.stack([lcg_noise_fast(frames, 41 + c, amp) for c in range(n_in)]).astype(np.float32)


def _engine(n_out, coeffs, bs=64, **opts):
    opts.setdefault("batch_blocks", 8)
    a = _hip(SR, bs, **opts)
    assert a.render(*_roots(n_out))["result"] == 0
    if coeffs is not None:
        a.noise_shape(coeffs)
    return a


def _same(streams, codes, G, fmt):
    want = ref.pack(codes, G, fmt)
    return len(streams) == len(want) and all(np.ascontiguousarray(s).tobytes() == w.tobytes() for s, w in zip(streams, want))


def test_off_reports_nothing(gpu_required):
    a = _engine(2, None)
    x = _inputs(FRAMES)
    a.process_blocks_pcm(x, 1, 2, FRAMES, "s16", dither_seed=3)
    got = a.noise_shape_read()
    assert got["taps"] == 0 and got["channels"] == 0 and got["frames"] == 0 and got["saturated"].size == 0


@pytest.mark.parametrize("channels,G", [(1, 1), (2, 2), (3, 3), (3, 1), (16, 2), (17, 1), (33, 3), (33, 1)])
def test_bytes_equal_the_reference(gpu_required, channels, G):
    """Channel counts that straddle a workgroup's 16, every grouping, K = 1, 9 and 12, s16 and s24, with and without dither — one
    engine, a programme per combination, each at the render's own sample time; the read-out equals the reference's counts."""
    a = _engine(channels, None)
    x = _inputs(FRAMES)
    combos = [(1, "s16", 5), (9, "s16", None), (12, "s24", 77), (9, "s24", 1234), (12, "s16", None), (1, "s24", None)]
    for K, fmt, seed in combos:
        a.noise_shape(TAPS[K])
        t0 = a.sample_time
        streams, _, planar = a.process_blocks_pcm(x, channels // G, G, FRAMES, fmt, dither_seed=seed, want_float=True)
        bits = 16 if fmt == "s16" else 24
        codes, st = ref.shape(TAPS[K], planar, bits, seed, time0=t0)
        assert _same(streams, codes, G, fmt), (K, fmt, seed)
        S = 1 << (bits - 1)
        assert codes.min() == -S and codes.max() == S - 1           # (channel 0 has a gain beyond 1: it clips)
        got = a.noise_shape_read()
        assert got["taps"] == K and got["channels"] == channels and got["frames"] == FRAMES
        assert got["coeffs_q"].tolist() == ref.quantise_coeffs(TAPS[K])
        assert got["saturated"].tolist() == st["saturated"].tolist(), (K, fmt, seed)
        twin, tst = noise_shape_host(TAPS[K], planar, bits, seed, time0=t0)
        assert np.array_equal(twin.astype(np.int64), codes) and np.array_equal(tst, ref.state_bytes(st))


def test_a_tile_of_its_own_per_256_frames(gpu_required):
    """Engine blocks of 350 hold two tiles (256 + 94), sets of 3 blocks, the last block cut."""
    a = _engine(5, TAPS[9], bs=350, batch_blocks=3)
    frames = 7 * 350 + 123
    x = _inputs(frames)
    t0 = a.sample_time
    streams, _, planar = a.process_blocks_pcm(x, 5, 1, frames, "s16", dither_seed=8, want_float=True)
    codes, st = ref.shape(TAPS[9], planar, 16, 8, time0=t0)
    assert _same(streams, codes, 1, "s16")
    assert a.noise_shape_read()["saturated"].tolist() == st["saturated"].tolist()


def test_bytes_do_not_depend_on_the_cut(gpu_required):
    """One call = calls of 100, 1, 511 and the rest = launch sets of 3 blocks. (A call renders whole blocks: the roots' fade-in is
    rendered out first, on float delivery, which shapes nothing, so that every cut delivers the same floats; the dither's time is
    given.)"""
    x = _inputs(FRAMES)
    T0 = 1 << 20

    def engine(batch):
        a = _engine(4, TAPS[12], batch_blocks=batch)
        a.process_blocks_pcm(_inputs(2048), 2, 2, 2048, "f32")
        assert a.noise_shape_read()["frames"] == 0
        return a
    whole = engine(8).process_blocks_pcm(x, 2, 2, FRAMES, "s16", dither_seed=11, sample_time=T0)[0]
    for batch, cuts in ((8, (100, 101, 612)), (3, ())):
        a = engine(batch)
        parts, at = [], 0
        for end in list(cuts) + [FRAMES]:
            parts.append(a.process_blocks_pcm(x[:, at:end], 2, 2, end - at, "s16", dither_seed=11, sample_time=T0 + at)[0])
            at = end
        for s in range(2):
            assert np.concatenate([p[s] for p in parts]).tobytes() == whole[s].tobytes(), (batch, cuts, s)
        assert a.noise_shape_read()["frames"] == FRAMES


def _decoded(data, bits):
    _, chans = flac_reference.decode_frames(data, {"rate": 44100, "bps": bits})
    return np.array(chans, dtype=np.int64)


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("G", [1, 2])
def test_flac_delivers_the_pcm_paths_codes(gpu_required, G, bits):
    """FLAC delivery with shaping on decodes to the PCM path's codes, its MD5 is that of the PCM bytes; drop and take discard codes,
    not state: the frames that enter are the whole render's codes [drop, drop + take)."""
    n_out, fmt = 2 * G, "s%d" % bits
    x = _inputs(FRAMES)
    b = _engine(n_out, TAPS[9])
    pcm, _, planar = b.process_blocks_pcm(x, 2, G, FRAMES, fmt, dither_seed=21, want_float=True)
    codes, _ = ref.shape(TAPS[9], planar, bits, 21, time0=0)
    assert _same(pcm, codes, G, fmt)
    a = _engine(n_out, TAPS[9], flac_frame=FF, flac_md5=1)
    body, _ = a.process_blocks_flac(x, 2, G, FRAMES, bits, dither_seed=21)
    tail = a.flac_flush()
    got = a.flac_read()
    for s in range(2):
        assert np.array_equal(_decoded(body[s] + tail[s], bits), codes[s * G:(s + 1) * G]), s
        assert got["md5"][s] == hashlib.md5(np.ascontiguousarray(pcm[s]).tobytes()).digest(), s
    assert a.noise_shape_read()["frames"] == FRAMES
    c = _engine(n_out, TAPS[9], flac_frame=FF)
    body, _ = c.process_blocks_flac(x, 2, G, FRAMES, bits, dither_seed=21, drop=70, take=600)
    tail = c.flac_flush()
    for s in range(2):
        assert np.array_equal(_decoded(body[s] + tail[s], bits), codes[s * G:(s + 1) * G, 70:670]), s
    assert c.noise_shape_read()["frames"] == FRAMES


def test_behind_the_converter_and_the_limiter(gpu_required):
    """resample_rate and limiter on: the codes are the twin's on the floats the call delivers, at the programme's output frame."""
    a = _engine(4, TAPS[9], bs=350, batch_blocks=3, resample_rate=48000, limiter_gain_db=6.0, limiter=1)
    st, at = None, 0
    for frames in (5 * FF + 99, 700):
        x = _inputs(frames)
        streams, _, planar = a.process_blocks_pcm(x, 2, 2, frames, "s24", dither_seed=7, want_float=True)
        assert planar.shape[1] == streams[0].shape[0] != frames
        codes, st = noise_shape_host(TAPS[9], planar, 24, 7, time0=at, state=st)
        assert _same(streams, codes, 2, "s24")
        at += planar.shape[1]
    assert a.noise_shape_read()["frames"] == at == a.resample_read()["frames_out"]


def test_host_block_path_and_on_into_launch_sets(gpu_required):
    """A tap graph at host block 1024 renders host block by host block, where the header's scalar loop shapes; the states travel to the
    device and back. Then the same programme goes on in launch sets of another graph: one reference programme throughout."""
    bs, G = 1024, 2
    taps = [el.tapOut({"name": "fb"}, el.add(el.mul(0.6, el.in_({"channel": 0})), el.mul(0.5, el.tapIn({"name": "fb"})))),
            el.mul(1.3, el.in_({"channel": 1}))]
    a = _hip(48000.0, bs, batch_blocks=8)
    assert a.render(*taps)["result"] == 0
    a.noise_shape(TAPS[12])
    st, total = None, 0

    def call(n):
        nonlocal st, total
        x = _inputs(n)
        t0 = a.sample_time
        streams, _, planar = a.process_blocks_pcm(x, 1, G, n, "s16", dither_seed=3, want_float=True)
        codes, st = ref.shape(TAPS[12], planar, 16, 3, time0=t0, state=st)
        assert _same(streams, codes, G, "s16"), n
        total += n
    for n in (1024 + 100, 1024 + 211):
        call(n)
    assert a.stats()["batch_launches"] == 0
    for step, n in enumerate((2 * 1024 + 100, 1024, 4 * 1024)):
        if step < 2:
            assert a.render(*[el.mul(0.4 + 0.3 * step + 0.1 * c, el.in_({"channel": c})) for c in range(G)])["result"] == 0
        else:
            a.gc()
        call(n)
    assert a.stats()["batch_launches"] > 0
    got = a.noise_shape_read()
    assert got["frames"] == total and got["saturated"].tolist() == st["saturated"].tolist()


def test_resets_and_unaffected_paths(gpu_required):
    x = _inputs(FRAMES)
    a = _engine(2, TAPS[9], flac_frame=FF)
    a.process_blocks_pcm(_inputs(2048), 1, 2, 2048, "f32")          # (the roots' fade-in, rendered out on float delivery)
    fresh = a.process_blocks_pcm(x, 1, 2, FRAMES, "s16", dither_seed=2, sample_time=0)[0][0].tobytes()
    carried = a.process_blocks_pcm(x, 1, 2, FRAMES, "s16", dither_seed=2, sample_time=0)[0][0].tobytes()
    assert carried != fresh                                       # (the second call went on from the first one's errors)
    a.noise_shape_reset()
    assert a.noise_shape_read()["frames"] == 0
    assert a.process_blocks_pcm(x, 1, 2, FRAMES, "s16", dither_seed=2, sample_time=0)[0][0].tobytes() == fresh
    a.noise_shape(TAPS[9])                                        # setting coefficients starts a new programme
    assert a.process_blocks_pcm(x, 1, 2, FRAMES, "s16", dither_seed=2, sample_time=0)[0][0].tobytes() == fresh
    with pytest.raises(ElemHipError):                             # a refused set changes nothing, the programme included
        a.noise_shape([64.0])
    assert a.noise_shape_read()["frames"] == FRAMES
    # a call that fails starts a new programme: a FLAC call behind the flush is refused
    a.process_blocks_flac(x, 1, 2, FRAMES, 16, dither_seed=2, sample_time=0)
    a.flac_flush()
    assert a.noise_shape_read()["frames"] == 2 * FRAMES
    with pytest.raises(ElemHipError):
        a.process_blocks_flac(x, 1, 2, FRAMES, 16, dither_seed=2, sample_time=0)
    assert a.noise_shape_read()["frames"] == 0
    assert a.process_blocks_pcm(x, 1, 2, FRAMES, "s16", dither_seed=2, sample_time=0)[0][0].tobytes() == fresh
    # another channel count starts a new programme
    assert a.render(*_roots(3))["result"] == 0
    a.process_blocks_pcm(x, 3, 1, FRAMES, "s16", dither_seed=2)
    got = a.noise_shape_read()
    assert got["channels"] == 3 and got["frames"] == FRAMES
    # float delivery is not touched, and shapes nothing; turned off again: plain dither's bytes, as an engine that never heard of it
    b, c = _engine(2, None), _engine(2, TAPS[9])
    f_on = c.process_blocks_pcm(x, 1, 2, FRAMES, "f32")[0][0]
    f_off = b.process_blocks_pcm(x, 1, 2, FRAMES, "f32")[0][0]
    assert f_on.tobytes() == f_off.tobytes() and c.noise_shape_read()["frames"] == 0
    shaped = c.process_blocks_pcm(x, 1, 2, FRAMES, "s16", dither_seed=2)[0][0].tobytes()
    plain = b.process_blocks_pcm(x, 1, 2, FRAMES, "s16", dither_seed=2)[0][0].tobytes()
    assert shaped != plain
    c.noise_shape(None)
    assert c.process_blocks_pcm(x, 1, 2, FRAMES, "s16", dither_seed=2)[0][0].tobytes() == b.process_blocks_pcm(x, 1, 2, FRAMES, "s16", dither_seed=2)[0][0].tobytes()


def test_master_and_offline_renderer_take_a_preset(gpu_required, tmp_path):
    from elementary_amd.offline import OfflineRenderer
    from elementary_amd.wav import WavWriter
    core = OfflineRenderer(lambda s, k: _hip(s, k, batch_blocks=4))
    with pytest.raises(ValueError):
        core.initialize(num_input_channels=2, num_output_channels=2, sample_rate=96000.0, block_size=64, noise_shape="fweighted9")
    core = OfflineRenderer(lambda s, k: _hip(s, k, batch_blocks=4))
    core.initialize(num_input_channels=2, num_output_channels=2, sample_rate=SR, block_size=64, noise_shape="fweighted9")
    assert core.noise_shape()["taps"] == 9
    n = 44100                                                     # (a second: the loudness gate wants 400 ms blocks)
    t = np.arange(n)
    x = np.stack([0.001 * np.sin(2.0 * np.pi * 997.0 * t / SR), 0.3 * np.sin(2.0 * np.pi * 440.0 * t / SR)]).astype(np.float32)
    w = WavWriter(str(tmp_path / "in.wav"), "f32", 2, int(SR))
    w.write(np.ascontiguousarray(x.T))
    w.close()
    from elementary_amd.master import master_wav
    got = master_wav(lambda s, k: _hip(s, k), tmp_path / "in.wav", tmp_path / "out.wav", fmt="s16", noise_shape="lipshitz5")
    assert got["saturated"] == 0 and (tmp_path / "out.wav").stat().st_size > 2 * 2 * n
