"""PCM input of the offline host path (elemhip_process_blocks_pcm_io): launch sets whose input arrives as interleaved int16 / packed
24-bit / float32 streams and is unpacked on the GPU (elementary_amd/csrc/pcm_unpack.hip). The main check needs no tolerance: a twin
engine that is handed ``process_blocks_host(decode(streams))`` — decode being tests/pcm_unpack_reference.py, a numpy restatement of
the specification, not of the header — must return bit-identical floats. The floats are additionally held to the reference engine
within the suite's tolerance, as tests/test_gpu_pcm.py does."""
import ctypes as C
import wave

import numpy as np
import pytest

import pcm_reference as ref
import pcm_unpack_reference as uref
from elementary_amd import el, graphs
from elementary_amd.offline import OfflineRenderer
from test_gpu_events import TOL
from test_gpu_pcm import GAINS, _check_call, _checker, _hip, _ref_planar

pytestmark = pytest.mark.gpu
SR = graphs.C2_SAMPLE_RATE


def _roots(n_in):
    """Output c = input c scaled by its own constant plus a one-pole over its one-sample delay: every channel is told apart, and both
    the delay and the pole carry the end of one call into the next — a wrong sample behind a cut last block shows there."""
    def one(c):
        x = el.in_({"channel": c})
        return el.add(el.mul(GAINS[c % len(GAINS)], x), el.mul(0.25, el.pole(0.5, el.z(x))))
    return [one(c) for c in range(n_in)]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("G", [1, 2, 3, 6])
@pytest.mark.parametrize("bs", [128, 512])
def test_floats_equal_the_planar_path_bit_for_bit(gpu_required, bs, G):
    """37 blocks + 37 frames in sets of 8 blocks: five sets (both halves of every double buffer, a short last set, a cut last block),
    two streams of G channels, the three formats, each twice in a row on the same engines: the second call starts from the state the
    first one's zero-padded tail left."""
    n_in, frames = 2 * G, 37 * bs + 37
    a, b, c = _hip(SR, bs, batch_blocks=8), _hip(SR, bs, batch_blocks=8), _checker(SR, bs)
    for rt in (a, b, c):
        assert rt.render(*_roots(n_in))["result"] == 0
    calls = 0
    for k, fmt in enumerate(("s16", "s24", "f32")):
        for rep in range(2):
            streams = uref.random_streams(fmt, frames, G, 2, 100 * k + rep)
            x = uref.decode(streams, fmt)
            got = a.process_blocks_pcm_io(streams, fmt, n_in)
            twin = b.process_blocks_host(x, n_in, frames)
            assert got.shape == (n_in, frames) and _same_bits(got, twin), (fmt, G, rep, int((got != twin).sum()))
            want = _ref_planar(c, x, n_in, bs, frames)
            worst = float(np.abs(got - want).max())
            print(fmt, G, rep, "max abs err vs the reference engine", worst)
            assert worst <= TOL * max(1.0, float(np.abs(want).max())), (fmt, G, rep)
            calls += 1
    st = a.stats()
    assert st["batch_launches"] >= 5 and st["blocks_rendered"] == calls * 38 == b.stats()["blocks_rendered"], st


def test_sliced_host_block_700_s24_three_channels(gpu_required):
    """Block 700 renders as two slices of 350 frames: input rows that start 8 bytes off a 16-byte line, streams whose sets do not end on one."""
    bs, G, n_in = 700, 3, 6
    frames = 37 * bs + 37
    a, b, c = _hip(SR, bs, batch_blocks=8), _hip(SR, bs, batch_blocks=8), _checker(SR, bs)
    for rt in (a, b, c):
        assert rt.render(*_roots(n_in))["result"] == 0
    for rep in range(2):
        streams = uref.random_streams("s24", frames, G, 2, 7 + rep)
        x = uref.decode(streams, "s24")
        got = a.process_blocks_pcm_io(streams, "s24", n_in)
        assert _same_bits(got, b.process_blocks_host(x, n_in, frames)), rep
        want = _ref_planar(c, x, n_in, bs, frames)
        assert float(np.abs(got - want).max()) <= TOL * max(1.0, float(np.abs(want).max()))
    assert a.stats()["batch_launches"] >= 1


def test_pcm_in_pcm_out(gpu_required):
    """s16 in, s24 out with dither: the bytes are the restatement's pack of the planar floats of the same call, and the twin engine's
    process_blocks_pcm bytes for the decoded input."""
    bs, G, n_in, frames = 512, 2, 4, 20 * 512 + 37
    a, b = _hip(SR, bs, batch_blocks=8), _hip(SR, bs, batch_blocks=8)
    for rt in (a, b):
        assert rt.render(*_roots(n_in))["result"] == 0
    for rep in range(2):
        streams = uref.random_streams("s16", frames, G, 2, 50 + rep, amp=0.95)
        t0 = a.sample_time
        out, stats, planar = a.process_blocks_pcm_io(streams, "s16", None, None, "s24", 2, 2, dither_seed=77, want_float=True)
        _check_call(out, stats, planar, 2, "s24", 77, t0)
        tout, tstats, tplanar = b.process_blocks_pcm(uref.decode(streams, "s16"), 2, 2, frames, "s24", dither_seed=77, want_float=True)
        assert _same_bits(planar, tplanar)
        for s in range(2):
            assert ref.same_bytes(out[s], tout[s])
        assert np.array_equal(stats["over"], tstats["over"]) and int(stats["over"].sum()) > 0
    # without the planar floats: the same bytes (both engines go on from the same state)
    t0 = a.sample_time
    out, stats, planar = a.process_blocks_pcm_io(streams, "s16", None, None, "s24", 2, 2, dither_seed=78)
    tout = b.process_blocks_pcm(uref.decode(streams, "s16"), 2, 2, frames, "s24", dither_seed=78, sample_time=t0)[0]
    assert planar is None and all(ref.same_bytes(out[s], tout[s]) for s in range(2))
    assert a.stats()["batch_launches"] >= 3


def test_nonfinite_f32_input_arrives(gpu_required):
    bs, G, frames = 512, 2, 12 * 512 + 100
    stream = uref.random_streams("f32", frames, G, 1, 9, amp=0.5)[0]
    spots = {6 * 512: np.nan, 7 * 512 + 511: np.inf, 9 * 512 + 3: -np.inf, 12 * 512 + 50: np.nan, 12 * 512 + 99: np.inf}
    for f, v in spots.items():
        stream[f, 0] = v
    roots = [el.mul(1.0, el.in_({"channel": 0})), el.mul(0.5, el.in_({"channel": 1}))]
    a, b = _hip(SR, bs, batch_blocks=8), _hip(SR, bs, batch_blocks=8)
    assert a.render(*roots)["result"] == 0 and b.render(*roots)["result"] == 0
    out, stats, planar = a.process_blocks_pcm_io([stream], "f32", None, None, "f32", 1, 2, want_float=True)
    _check_call(out, stats, planar, 2, "f32", None, 0)
    assert stats["nonfinite"].tolist() == [len(spots), 0]
    idx = sorted(spots)
    assert np.isnan(planar[0, [idx[0], idx[3]]]).all() and planar[0, idx[1]] == np.inf and planar[0, idx[2]] == -np.inf and planar[0, idx[4]] == np.inf
    finite = np.ones(frames, bool); finite[idx] = False
    assert np.isfinite(planar[0, finite]).all() and np.isfinite(planar[1]).all()
    assert _same_bits(planar, b.process_blocks_host(uref.decode([stream], "f32"), 2, frames))


def test_tap_graph_under_a_sliced_host_block_unpacks_on_the_host(gpu_required):
    """A tap graph at host block 1024 renders host block by host block through process(): its inputs are needed on the host and are
    unpacked there by the header's scalar loop — the same samples."""
    bs, G, frames = 1024, 2, 5 * 1024 + 211
    roots = [el.tapOut({"name": "fb"}, el.add(el.mul(1.5, el.in_({"channel": 0})), el.mul(0.5, el.tapIn({"name": "fb"})))),
             el.mul(0.9, el.in_({"channel": 1}))]
    a, b, c = _hip(48000.0, bs), _hip(48000.0, bs), _checker(48000.0, bs)
    for rt in (a, b, c):
        assert rt.render(*roots)["result"] == 0
    for fmt in ("s16", "s24", "f32"):
        streams = uref.random_streams(fmt, frames, G, 1, 21)
        x = uref.decode(streams, fmt)
        got = a.process_blocks_pcm_io(streams, fmt, 2)
        assert _same_bits(got, b.process_blocks_host(x, 2, frames)), fmt
        want = _ref_planar(c, x, 2, bs, frames)
        assert float(np.abs(got - want).max()) <= TOL * max(1.0, float(np.abs(want).max()))
    out, stats, planar = a.process_blocks_pcm_io(streams, "f32", None, None, "s16", 1, 2, dither_seed=3, want_float=True, sample_time=0)
    _check_call(out, stats, planar, 2, "s16", 3, 0)
    assert a.stats()["batch_launches"] == 0                      # (it did take the block-by-block path)


def test_offline_renderer_listeners(gpu_required):
    bs, n, frames = 512, 2, 40 * 512 + 11
    streams = uref.random_streams("s24", frames, 2, 1, 4)
    x = uref.decode(streams, "s24")

    def roots():
        return [el.meter({"name": "l"}, el.mul(1.2, el.in_({"channel": 0}))), el.meter({"name": "r"}, el.add(el.z(el.in_({"channel": 0})), el.in_({"channel": 1})))]

    logs, outs = [], []
    for use_pcm in (True, False):
        core = OfflineRenderer(lambda sr, nn: _hip(sr, nn, batch_blocks=8))
        core.initialize(num_input_channels=2, num_output_channels=n, sample_rate=SR, block_size=bs)
        log = []
        core.on("meter", lambda p, log=log: log.append(p))
        core.render(*roots())
        if use_pcm:
            outs.append(core.process_pcm_io(streams, "s24"))
            assert core.runtime.stats()["batch_launches"] >= 1
        else:
            out = [np.zeros(frames, np.float32) for _ in range(n)]
            core.process(list(x), out)
            outs.append(np.stack(out))
        logs.append(log)
    assert _same_bits(outs[0], outs[1])
    assert len(logs[0]) == 2 * 41 and logs[0] == logs[1]


def test_process_wav_end_to_end(gpu_required, tmp_path):
    from elementary_amd.wav import WavWriter
    bs, frames, tail = 512, 20 * 512 + 123, 300
    stream = uref.random_streams("s16", frames, 2, 1, 12, amp=0.9)[0]
    with WavWriter(str(tmp_path / "in.wav"), "s16", 2, SR) as w:
        w.write(stream)
    made = []
    for _ in range(2):
        core = OfflineRenderer(lambda sr, n: _hip(sr, n, batch_blocks=8))
        core.initialize(num_input_channels=2, num_output_channels=2, sample_rate=SR, block_size=bs)
        core.render(*_roots(2))
        made.append(core)
    x = np.zeros((2, frames + tail), np.float32)
    x[:, :frames] = uref.decode([stream], "s16")
    streams, stats, _ = made[0].process_pcm(list(x), 1, 2, frames + tail, "s24", dither_seed=11)
    wstats = made[1].process_wav(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), "s24", num_frames=frames + tail, dither_seed=11, chunk_frames=7 * 512)
    with wave.open(str(tmp_path / "out.wav"), "rb") as r:
        assert (r.getnchannels(), r.getsampwidth(), r.getframerate(), r.getnframes()) == (2, 3, int(SR), frames + tail)
        assert r.readframes(frames + tail) == streams[0].tobytes()
    assert np.array_equal(wstats["peak"], stats["peak"]) and np.array_equal(wstats["over"], stats["over"])
    # the default length is the input's; another sample rate is refused
    made[1].process_wav([str(tmp_path / "in.wav")], str(tmp_path / "out2.wav"), "s16")
    with wave.open(str(tmp_path / "out2.wav"), "rb") as r:
        assert r.getnframes() == frames
    with WavWriter(str(tmp_path / "in8k.wav"), "s16", 2, 8000.0) as w:
        w.write(stream[:100])
    with pytest.raises(ValueError, match="sample rate"):
        made[1].process_wav(str(tmp_path / "in8k.wav"), str(tmp_path / "out3.wav"), "s16")


def test_error_codes_render_nothing(gpu_required):
    from elementary_amd.runtime import ElemHipError, Runtime, _PcmInSpec
    a = _hip(SR, 512)
    assert a.render(*_roots(2))["result"] == 0
    before = a.stats()["blocks_rendered"]
    s16 = np.zeros((512, 2), np.int16)
    for args, kwargs, code in ((([s16], 4, 2), {}, 8), (([s16], 0, 2), {}, 8), (([s16], "s16", 2), dict(in_channels_per_stream=0), 8),
                               (([np.zeros((512, 17), np.int16)] * 2, "s16", 2), {}, 103),
                               (([s16], "s16"), dict(out_fmt="s16", num_streams=513, channels_per_stream=2), 103),
                               (([s16], "s16"), dict(out_fmt=7, num_streams=1, channels_per_stream=2), 8)):
        with pytest.raises(ElemHipError) as e:
            a.process_blocks_pcm_io(*args, **kwargs)
        assert e.value.code == code, (kwargs, e.value.code)
    # NULL spec / NULL streams with a stream count
    ip = (C.c_void_p * 1)(C.c_void_p(s16.ctypes.data))
    out = np.zeros((2, 512), np.float32)
    op = (C.POINTER(C.c_float) * 2)(*[row.ctypes.data_as(C.POINTER(C.c_float)) for row in out])
    spec = _PcmInSpec(1, 2)
    assert a._lib.elemhip_process_blocks_pcm_io(a._h, ip, 1, None, None, 0, None, op, 2, 512, 0, None) == 8
    assert a._lib.elemhip_process_blocks_pcm_io(a._h, None, 1, C.byref(spec), None, 0, None, op, 2, 512, 0, None) == 8
    assert a.stats()["blocks_rendered"] == before
    assert a._lib.elemhip_process_blocks_pcm_io(a._h, ip, 1, C.byref(spec), None, 0, None, op, 2, 512, 0, None) == 0     # (the call as it should be)
    assert a.stats()["blocks_rendered"] == before + 1
    dry = Runtime(SR, 512, device=-1)
    with pytest.raises(ElemHipError) as e:
        dry.process_blocks_pcm_io([s16], "s16", 2)
    assert e.value.code == 101
