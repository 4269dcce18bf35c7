"""PCM delivery of the offline host path (elemhip_process_blocks_pcm): launch sets whose output is packed on the GPU
(elementary_amd/csrc/pcm_pack.hip) into interleaved int16 / packed 24-bit / float32 streams. Every comparison of packed bytes is exact
equality against tests/pcm_reference.py — a numpy restatement of the specification, not of the header — applied to the planar floats
the SAME call returned; the floats themselves are held to the reference engine within the suite's tolerance."""
import wave

import numpy as np
import pytest

import pcm_reference as ref
from elementary_amd import el, graphs
from elementary_amd.offline import OfflineRenderer
from helpers import lcg_noise_fast
from test_gpu_events import TOL

pytestmark = pytest.mark.gpu
SR = graphs.C2_SAMPLE_RATE
GAINS = (1.7, 0.9, -1.3, 0.5, 1.1, -0.7, 0.3, 1.9, -0.2, 0.8, 1.4, -1.0)


def _hip(sr, bs, **opts):
    from elementary_amd.runtime import Runtime
    rt = Runtime(sr, bs, device=0)
    for k, v in opts.items():
        rt.set_option(k, v)
    return rt


def _checker(sr, bs):
    import oracle
    return oracle.RefRuntime(sr, bs) if oracle.have_ref() else oracle.PortRuntime(sr, bs)


def _roots(n_out, n_in=2):
    """Channel c = in[c % n_in] scaled by a constant (some beyond full scale: they clip); the first two also carry the C2 voices."""
    c2 = graphs.c2_graph(voices=4)
    roots = [el.mul(GAINS[c % len(GAINS)], el.in_({"channel": c % n_in})) for c in range(n_out)]
    for c in range(min(2, n_out)):
        roots[c] = el.add(c2[c], roots[c])
    return roots


def _inputs(frames, n_in=2, amp=0.8):
    return np.stack([lcg_noise_fast(frames, 41 + c, amp) for c in range(n_in)]).astype(np.float32)


def _ref_planar(c, x, n_out, bs, frames):
    nb = (frames + bs - 1) // bs
    xp = np.zeros((x.shape[0], nb * bs), dtype=np.float32)
    xp[:, :frames] = x[:, :frames]
    return np.concatenate([c.process(xp[:, b * bs:(b + 1) * bs], n_out, bs) for b in range(nb)], axis=1)[:, :frames]


def _check_call(streams, stats, planar, G, fmt, seed, t0):
    want = ref.pack(planar, G, fmt, seed, t0)
    assert len(streams) == len(want)
    for s, (a, b) in enumerate(zip(streams, want)):
        assert ref.same_bytes(a, b), (fmt, G, s, int((np.ascontiguousarray(a).view(np.uint8) != np.ascontiguousarray(b).view(np.uint8)).sum()))
    st = ref.stats(planar)
    print(fmt, G, "peak", stats["peak"].tolist(), "over", stats["over"].tolist(), "nonfinite", stats["nonfinite"].tolist())
    assert np.array_equal(stats["peak"].view(np.uint32), st["peak"].view(np.uint32))
    assert np.array_equal(stats["over"], st["over"]) and np.array_equal(stats["nonfinite"], st["nonfinite"])


@pytest.mark.parametrize("G", [1, 2, 3, 6])
@pytest.mark.parametrize("bs", [128, 512])
def test_bytes_and_stats_equal_the_reference(gpu_required, bs, G):
    """37 blocks + 37 frames in sets of 8 blocks: five sets (both halves of every double buffer, a short last set, a cut last block),
    two streams of G channels, the three formats one call after another on one engine."""
    n_out, frames = 2 * G, 37 * bs + 37
    a, c = _hip(SR, bs, batch_blocks=8), _checker(SR, bs)
    assert a.render(*_roots(n_out))["result"] == 0 and c.render(*_roots(n_out))["result"] == 0
    for k, fmt in enumerate(("s16", "s24", "f32")):
        x = _inputs(frames) if k == 0 else np.roll(_inputs(frames), 1000 * k, axis=1)
        seed = 1234 + k if G % 2 == 0 else None
        t0 = a.sample_time
        streams, stats, planar = a.process_blocks_pcm(x, 2, G, frames, fmt, dither_seed=seed, want_float=True)
        _check_call(streams, stats, planar, G, fmt, seed, t0)
        want = _ref_planar(c, x, n_out, bs, frames)
        assert float(np.abs(planar - want).max()) <= TOL * max(1.0, float(np.abs(want).max())), (fmt, G)
        assert int(stats["over"].sum()) > 0                      # (the scaled inputs do clip)
    st = a.stats()
    assert st["batch_launches"] >= 5 and st["blocks_rendered"] == 3 * 38, st


def test_sliced_host_block_700_s24_three_channels(gpu_required):
    """Block 700 renders as two slices of 350 frames: rows that start 8 bytes off a 16-byte line, streams whose sets do not end on one."""
    bs, G, n_out = 700, 3, 6
    frames = 37 * bs + 37
    a, c = _hip(SR, bs, batch_blocks=8), _checker(SR, bs)
    assert a.render(*_roots(n_out))["result"] == 0 and c.render(*_roots(n_out))["result"] == 0
    x = _inputs(frames)
    streams, stats, planar = a.process_blocks_pcm(x, 2, G, frames, "s24", dither_seed=99, want_float=True)
    _check_call(streams, stats, planar, G, "s24", 99, 0)
    want = _ref_planar(c, x, n_out, bs, frames)
    assert float(np.abs(planar - want).max()) <= TOL * max(1.0, float(np.abs(want).max()))
    assert a.stats()["batch_launches"] >= 1


def test_dither_is_keyed_on_seed_and_absolute_time(gpu_required):
    bs, G, n_out, frames = 512, 2, 4, 16 * 512
    t0 = (1 << 32) + 5 * 512                                # absolute times whose upper half is not zero
    x = _inputs(frames)

    def fresh():
        rt = _hip(SR, bs, batch_blocks=4)
        assert rt.render(*_roots(n_out))["result"] == 0
        return rt

    one = fresh().process_blocks_pcm(x, 2, G, frames, "s16", dither_seed=7, want_float=True, sample_time=t0)
    _check_call(*one, G, "s16", 7, t0)
    b = fresh()
    cut = 7 * 512
    p1 = b.process_blocks_pcm(x[:, :cut], 2, G, cut, "s16", dither_seed=7, want_float=True, sample_time=t0)
    p2 = b.process_blocks_pcm(x[:, cut:], 2, G, frames - cut, "s16", dither_seed=7, want_float=True, sample_time=t0 + cut)
    _check_call(*p1, G, "s16", 7, t0)
    _check_call(*p2, G, "s16", 7, t0 + cut)
    for s in range(2):                                          # the same seed, the same render: the same bytes however it is cut
        assert ref.same_bytes(np.concatenate([p1[0][s], p2[0][s]]), one[0][s])
    other = fresh().process_blocks_pcm(x, 2, G, frames, "s16", dither_seed=8, want_float=True, sample_time=t0)
    _check_call(*other, G, "s16", 8, t0)
    plain = fresh().process_blocks_pcm(x, 2, G, frames, "s16", dither_seed=None, want_float=True, sample_time=t0)
    _check_call(*plain, G, "s16", None, t0)
    assert np.array_equal(other[2], one[2]) and np.array_equal(plain[2], one[2])       # the same floats ...
    for s in range(2):                                                                  # ... other bytes
        assert not ref.same_bytes(other[0][s], one[0][s]) and not ref.same_bytes(plain[0][s], one[0][s])


def test_nonfinite_input(gpu_required):
    bs, G, n_out, frames = 512, 2, 2, 12 * 512 + 100
    x = _inputs(frames, n_in=2, amp=0.5)
    spots = {6 * 512 + 3: np.nan, 7 * 512 + 511: np.inf, 9 * 512: -np.inf, 12 * 512 + 50: np.nan}
    for f, v in spots.items():
        x[0, f] = v
    roots = [el.mul(1.0, el.in_({"channel": 0})), el.mul(0.5, el.in_({"channel": 1}))]
    got = {}
    for fmt in ("s16", "s24", "f32"):
        a = _hip(SR, bs, batch_blocks=8)
        assert a.render(*roots)["result"] == 0
        streams, stats, planar = a.process_blocks_pcm(x, 1, G, frames, fmt, want_float=True)
        _check_call(streams, stats, planar, G, fmt, None, 0)
        got[fmt] = (streams[0], stats, planar)
        assert stats["nonfinite"].tolist() == [len(spots), 0] and not np.isfinite(planar[0, list(spots)]).any()
        finite = np.where(np.isfinite(planar[0]), np.abs(planar[0]), 0)
        assert stats["peak"][0] == np.float32(finite.max()) and 0.4 < stats["peak"][0] <= 0.5         # the peak ignores them
    assert (got["s16"][0][list(spots), 0] == 0).all() and (got["s24"][0][list(spots), 0, :] == 0).all()
    f32 = got["f32"]
    assert np.array_equal(f32[0][:, 0].view(np.uint32), f32[2][0].view(np.uint32))                    # the bits pass through


def test_launch_sets_and_listeners(gpu_required):
    bs, G, n_out, frames = 512, 2, 2, 40 * 512 + 11
    x = _inputs(frames)

    def roots():
        return [el.meter({"name": "l"}, el.mul(1.2, el.in_({"channel": 0}))), el.meter({"name": "r"}, el.add(graphs.c2_graph(voices=4)[1], el.in_({"channel": 1})))]

    a, b = _hip(SR, bs, batch_blocks=8), _hip(SR, bs, batch_blocks=8)
    assert a.render(*roots())["result"] == 0 and b.render(*roots())["result"] == 0
    streams, stats, planar = a.process_blocks_pcm(x, 1, G, frames, "s16", dither_seed=5, want_float=True)
    host = b.process_blocks_host(x, n_out, frames)
    _check_call(streams, stats, planar, G, "s16", 5, 0)
    assert np.array_equal(planar, host)                          # the float path's samples, bit for bit
    assert a.stats()["batch_launches"] >= 1 and a.stats()["blocks_rendered"] == b.stats()["blocks_rendered"] == 41

    logs = []
    for use_pcm in (True, False):
        core = OfflineRenderer(lambda sr, n: _hip(sr, n, batch_blocks=8))
        core.initialize(num_input_channels=2, num_output_channels=n_out, sample_rate=SR, block_size=bs)
        log = []
        core.on("meter", lambda p, log=log: log.append(p))
        core.render(*roots())
        if use_pcm:
            s2, st2, pl2 = core.process_pcm(list(x), 1, G, frames, "s24", dither_seed=5, want_float=True)
            _check_call(s2, st2, pl2, G, "s24", 5, 0)
            assert core.runtime.stats()["batch_launches"] >= 1
        else:
            out = [np.zeros(frames, np.float32) for _ in range(n_out)]
            core.process(list(x), out)
            assert np.array_equal(np.stack(out), pl2)
        logs.append(log)
    assert len(logs[0]) == 2 * 41 and logs[0] == logs[1]


def test_host_packed_fallback_for_taps_under_a_sliced_block(gpu_required):
    """A tap graph at host block 1024 renders host block by host block through process(): its floats are on the host and are packed
    there by the header's scalar loop — the same bytes."""
    bs, G, frames = 1024, 2, 5 * 1024 + 211
    roots = [el.tapOut({"name": "fb"}, el.add(el.mul(1.5, el.in_({"channel": 0})), el.mul(0.5, el.tapIn({"name": "fb"})))),
             el.mul(0.9, el.in_({"channel": 1}))]
    a, c = _hip(48000.0, bs), _checker(48000.0, bs)
    assert a.render(*roots)["result"] == 0 and c.render(*roots)["result"] == 0
    x = _inputs(frames)
    for fmt, seed in (("s16", 3), ("s24", None), ("f32", None)):
        t0 = a.sample_time
        streams, stats, planar = a.process_blocks_pcm(x, 1, G, frames, fmt, dither_seed=seed, want_float=True)
        _check_call(streams, stats, planar, G, fmt, seed, t0)
        want = _ref_planar(c, x, 2, bs, frames)
        assert float(np.abs(planar - want).max()) <= TOL * max(1.0, float(np.abs(want).max()))
    assert a.stats()["batch_launches"] == 0                      # (it did take the block-by-block path)


def test_write_wav_end_to_end(gpu_required, tmp_path):
    bs, n_out, frames = 512, 4, 20 * 512 + 123
    x = _inputs(frames)
    made = []
    for _ in range(2):
        core = OfflineRenderer(lambda sr, n: _hip(sr, n, batch_blocks=8))
        core.initialize(num_input_channels=2, num_output_channels=n_out, sample_rate=SR, block_size=bs)
        core.render(*_roots(n_out))
        made.append(core)
    streams, stats, _ = made[0].process_pcm(list(x), 2, 2, frames, "s24", dither_seed=11)
    wstats = made[1].write_wav(str(tmp_path / "stem{}.wav"), list(x), frames, "s24", channels_per_stream=2, dither_seed=11, chunk_frames=7 * 512)
    for s in range(2):
        with wave.open(str(tmp_path / f"stem{s}.wav"), "rb") as r:
            assert (r.getnchannels(), r.getsampwidth(), r.getframerate(), r.getnframes()) == (2, 3, int(SR), frames)
            assert r.readframes(frames) == streams[s].tobytes()
    assert np.array_equal(wstats["peak"], stats["peak"]) and np.array_equal(wstats["over"], stats["over"])


def test_error_codes_render_nothing(gpu_required):
    from elementary_amd.runtime import ElemHipError, Runtime
    a = _hip(SR, 512)
    assert a.render(*_roots(2))["result"] == 0
    before = a.stats()["blocks_rendered"]
    for kwargs, code in ((dict(num_streams=1, channels_per_stream=2, fmt=4), 8), (dict(num_streams=1, channels_per_stream=2, fmt=0), 8),
                         (dict(num_streams=2, channels_per_stream=0, fmt="s16"), 8), (dict(num_streams=513, channels_per_stream=2, fmt="s16"), 103)):
        with pytest.raises(ElemHipError) as e:
            a.process_blocks_pcm(None, num_frames=512, **kwargs)
        assert e.value.code == code, (kwargs, e.value.code)
    assert a.stats()["blocks_rendered"] == before
    dry = Runtime(SR, 512, device=-1)
    with pytest.raises(ElemHipError) as e:
        dry.process_blocks_pcm(None, 1, 2, 512, "s16")
    assert e.value.code == 101
