"""FLAC input of the offline host path (input format 4; elementary_amd/csrc/flac_decode.hip): launch sets whose input arrives as FLAC
frames and is decoded on the GPU. Every check is exact: feeding a stream as FLAC gives, bit for bit, what feeding the codes
tests/flac_reference.py decodes from it — shifted to s16 / s24 — through the PCM input path gives, whatever the output form and however
the render is cut. Engines are created with batch_blocks=8, so launch-set boundaries fall inside FLAC frames."""
import os

import numpy as np
import pytest

import flac_reference as ref
import flac_writer as fw
from cases import NODE_CASES
from elementary_amd import el
from elementary_amd.offline import OfflineRenderer
from test_flac_in_host import good_frame, named_corrupt
from test_gpu_pcm import _hip

pytestmark = pytest.mark.gpu
SR = 44100.0


def _chunk(data, nch, bps, bs=0):
    from elementary_amd.runtime import FlacChunk, flac_index
    off, first = flac_index(data, nch, bps, bs)
    return FlacChunk(np.frombuffer(data, dtype=np.uint8), off, first, nch, bps, int(first[-1]), 0, int(first[-1]))


def _pcm(chans, bps):
    """The codes as the interleaved PCM stream of the same samples: s16 `code << (16 - bps)` up to 16 bits, packed s24 above."""
    a = np.array(chans, dtype=np.int64).T
    if bps <= 16:
        return np.ascontiguousarray((a << (16 - bps)).astype(np.int16)), "s16"
    v = (a << (24 - bps)) & 0xFFFFFF
    return np.ascontiguousarray(np.stack([v & 255, (v >> 8) & 255, (v >> 16) & 255], axis=-1).astype(np.uint8)), "s24"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _through(n_in, bs, roots=None, warm=False, **opts):
    rt = _hip(SR, bs, batch_blocks=8, **opts)
    assert rt.render(*(roots or [el.in_({"channel": c}) for c in range(n_in)]))["result"] == 0
    if warm:        # past the new roots' fade-in: a pass-through then returns its input exactly
        rt.process_blocks_host(np.zeros((n_in, 16384), dtype=np.float32), n_in, 16384)
    return rt


@pytest.fixture(scope="module")
def corpus():
    """The writer's corpus with the reference's decode of it (computed once, never changed)."""
    out = []
    for name, data, chans, bps, bs in fw.corpus():
        got = ref.decode_frames(data)[1]
        assert got == chans
        out.append((name, data, got, bps, bs))
    return out


@pytest.mark.parametrize("bs", [64, 512])
def test_pass_through_equals_pcm_input_of_the_reference_codes(gpu_required, corpus, bs):
    engines = {}
    for name, data, chans, bps, fbs in corpus:
        nch, total = len(chans), len(chans[0])
        if nch not in engines:
            engines[nch] = (_through(nch, bs), _through(nch, bs))
        a, b = engines[nch]
        pcm, fmt = _pcm(chans, bps)
        got = a.process_blocks_pcm_io([_chunk(data, nch, bps, fbs)], "flac", nch, total)
        want = b.process_blocks_pcm_io([pcm], fmt, nch, total)
        assert _same(got, want), (name, int((_bits(got) != _bits(want)).sum()))


@pytest.mark.parametrize("bs", [64, 512])
@pytest.mark.parametrize("out_fmt", ["s16", "s24", "flac"])
def test_pcm_and_flac_outputs_equal_too(gpu_required, corpus, out_fmt, bs):
    """The whole corpus again with the delivery packed or encoded on the GPU: one pair of engines per channel count (the graph is a
    pass-through; both engines of a pair walk the same sample times, which key the dither)."""
    engines = {}
    for name, data, chans, bps, fbs in corpus:
        nch, total = len(chans), len(chans[0])
        if nch not in engines:
            engines[nch] = (_through(nch, bs), _through(nch, bs))
        a, b = engines[nch]
        pcm, fmt = _pcm(chans, bps)
        if out_fmt == "flac":
            got = a.process_blocks_flac([_chunk(data, nch, bps, fbs)], 1, nch, total, bits=24, in_fmt="flac")[0][0] + a.flac_flush()[0]
            want = b.process_blocks_flac([pcm], 1, nch, total, bits=24, in_fmt=fmt)[0][0] + b.flac_flush()[0]
            assert got == want and len(got) > 0, name
            a.flac_reset()
            b.flac_reset()
            continue
        got = a.process_blocks_pcm_io([_chunk(data, nch, bps, fbs)], "flac", None, total, out_fmt, 1, nch, dither_seed=5)
        want = b.process_blocks_pcm_io([pcm], fmt, None, total, out_fmt, 1, nch, dither_seed=5)
        assert _same(got[0][0], want[0][0]), name
        assert np.array_equal(got[1]["peak"], want[1]["peak"])


def _long_stream(nch=2, bps=16, fbs=192, frames=11, tail=17):
    chans = [fw._noise(frames * fbs + tail, bps, 60 + c) for c in range(nch)]
    subs = [dict(kind="LPC", coefs=fw._lpc(8, 12, 9, 3), precision=12, shift=9, porder=0, params=[12]), dict(kind="FIXED", order=3, porder=0, params=[11], method=1)]
    data = fw.write_stream(chans, bps, fbs, assignment="side_right" if nch == 2 else "independent", subs=subs[:nch])
    assert ref.decode_frames(data)[1] == chans
    return data, chans


@pytest.mark.parametrize("bs", [64, 512])
def test_cuts_leave_the_same_bits_and_the_tail_is_silence(gpu_required, bs):
    data, chans = _long_stream()
    total = len(chans[0])
    pcm, fmt = _pcm(chans, 16)
    n = ((total + 3 * bs) // bs) * bs                    # past the stream's end: whole blocks of silence behind it
    b = _through(2, bs)
    padded = np.concatenate([pcm, np.zeros((n - total, 2), dtype=np.int16)])
    want = b.process_blocks_pcm_io([padded], fmt, 2, n)
    whole = _chunk(data, 2, 16, 192)
    one = _through(2, bs).process_blocks_pcm_io([whole], "flac", 2, n)
    assert _same(one, want) and not one[:, total:].any()
    for step in (1 * bs, 7 * bs):                        # calls of 1 block and of 7 blocks: positions inside FLAC frames
        a = _through(2, bs)
        parts = [a.process_blocks_pcm_io([whole.at(k, min(step, n - k))], "flac", 2, min(step, n - k)) for k in range(0, n, step)]
        assert _same(np.concatenate(parts, axis=1), want), step
    # a chunk cut out of the stream (its table starts at a later frame), read from a position inside its first frame
    from elementary_amd.runtime import FlacChunk
    j = 3
    base = int(whole.offsets[j])
    cut = FlacChunk(whole.data[base:], whole.offsets[j:] - np.uint64(base), whole.first_samples[j:], 2, 16, total, j * 192 + 50, 4 * bs)
    got = _through(2, bs).process_blocks_pcm_io([cut], "flac", 2, 4 * bs)
    assert _same(got, _through(2, bs).process_blocks_pcm_io([padded[j * 192 + 50:j * 192 + 50 + 4 * bs]], fmt, 2, 4 * bs))


def test_stateful_graph_and_the_host_decode_under_a_sliced_tap_block(gpu_required):
    data, chans = _long_stream(nch=1)
    total = len(chans[0])
    pcm, fmt = _pcm(chans, 16)
    whole = _chunk(data, 1, 16, 192)
    roots = NODE_CASES["biquad"][0]
    for step in (total, 7 * 64):
        a, b = _through(1, 64, roots()), _through(1, 64, roots())
        got = np.concatenate([a.process_blocks_pcm_io([whole.at(k, min(step, total - k))], "flac", 1, min(step, total - k)) for k in range(0, total, step)], axis=1)
        want = np.concatenate([b.process_blocks_pcm_io([pcm[k:k + step]], fmt, 1, min(step, total - k)) for k in range(0, total, step)], axis=1)
        assert _same(got, want), step
    # host block 700 (two slices of 350) with taps: rendered host block by host block, the FLAC decoded on the host by decode_host
    taps = lambda: [el.tapOut({"name": "fb"}, el.add(el.mul(1.5, el.in_({"channel": 0})), el.mul(0.5, el.tapIn({"name": "fb"}))))]   # noqa: E731
    a, b = _through(1, 700, taps()), _through(1, 700, taps())
    assert _same(a.process_blocks_pcm_io([whole], "flac", 1, total), b.process_blocks_pcm_io([pcm], fmt, 1, total))


def test_input_rate_converter_behind_the_decoder(gpu_required):
    data, chans = _long_stream()
    pcm, fmt = _pcm(chans, 16)
    a, b = _through(2, 64, input_rate=48000.0), _through(2, 64, input_rate=48000.0)
    whole = _chunk(data, 2, 16, 192)
    at = 0
    for n in (5 * 64 + 7, 9 * 64, 64):                   # three calls: the input cursor walks through FLAC frames
        ni = a.input_resample_frames(n)
        assert ni == b.input_resample_frames(n) and at + ni <= len(chans[0])
        got = a.process_blocks_pcm_io([whole.at(at, ni)], "flac", 2, n)
        assert _same(got, b.process_blocks_pcm_io([pcm[at:at + ni]], fmt, 2, n)), n
        at += ni


def _renderer(n, bs, roots):
    core = OfflineRenderer(lambda s, k: _hip(s, k, batch_blocks=8))
    core.initialize(num_input_channels=n, num_output_channels=n, sample_rate=SR, block_size=bs)
    core.render(*roots)
    return core


def test_process_wav_reads_flac_and_a_written_flac_file_returns_its_codes(gpu_required, tmp_path):
    from elementary_amd.flac import FlacReader
    from elementary_amd.wav import WavWriter
    data, chans = _long_stream()
    total = len(chans[0])
    pcm, fmt = _pcm(chans, 16)
    with open(tmp_path / "in.flac", "wb") as f:
        f.write(fw.file_bytes(data, 16, 2, 192, total, rate=44100))
    with WavWriter(str(tmp_path / "in.wav"), "s16", 2, 44100) as w:
        w.write(pcm)
    roots = lambda: [el.mul(0.5, el.in_({"channel": 0})), el.pole(0.5, el.in_({"channel": 1}))]      # noqa: E731
    _renderer(2, 64, roots()).process_wav(str(tmp_path / "in.flac"), str(tmp_path / "a.wav"), "s24", chunk_frames=5 * 64)
    _renderer(2, 64, roots()).process_wav(str(tmp_path / "in.wav"), str(tmp_path / "b.wav"), "s24", chunk_frames=5 * 64)
    assert open(tmp_path / "a.wav", "rb").read() == open(tmp_path / "b.wav", "rb").read() and os.path.getsize(tmp_path / "a.wav") > total * 6
    # write_flac, read back through FlacReader and a pass-through engine: its own codes
    core = _renderer(2, 64, [el.in_({"channel": c}) for c in range(2)])
    x = (np.array(chans, dtype=np.float32) / 32768.0)
    core.write_flac(str(tmp_path / "w.flac"), [x[0], x[1]], total, bits=16)
    r = FlacReader(str(tmp_path / "w.flac"))
    assert (r.frames, r.channels, r.bits) == (total, 2, 16)
    own = ref.decode_file(open(tmp_path / "w.flac", "rb").read())[2]
    back = _through(2, 64, warm=True).process_blocks_pcm_io([r.read(total)], "flac", 2, total)
    assert np.array_equal(back.astype(np.float64) * 32768.0, np.array(own, dtype=np.float64)) and np.array(own).any()


def test_errors_answer_their_codes_and_the_engine_goes_on(gpu_required):
    from elementary_amd.runtime import ElemHipError, FlacChunk
    good, chans = good_frame()
    bad = named_corrupt()
    crc = bytearray(good)
    crc[-1] ^= 1                                          # (one of the corrupt corpus's single-bit flips)
    rt = _through(2, 64, warm=True)

    def chunk(frames, bits=16):
        data = b"".join(frames)
        off = np.cumsum([0] + [len(f) for f in frames])
        return FlacChunk(np.frombuffer(data, dtype=np.uint8), off, 16 * np.arange(len(frames) + 1), 2, bits, 16 * len(frames), 0, 16 * len(frames))

    def fails(c, code, **kw):
        with pytest.raises(ElemHipError) as e:
            rt.process_blocks_pcm_io([c], "flac", 2, c.count, **kw)
        assert e.value.code == code, (e.value.code, code)

    want = np.array(chans, dtype=np.float64)
    for name, frame, reason in (("crc", bytes(crc), 1), ("reserved_type", bad["reserved_type"], 2), ("variable", bad["variable"], 6), ("bps32", bad["bps32"], 6)):
        fails(chunk([good, good, frame, good]), 106)
        err = rt.flac_in_error()
        assert (err["stream"], err["frame"], err["reason"]) == (0, 2, reason), (name, err)
        # the next valid call renders correctly
        ok = rt.process_blocks_pcm_io([chunk([good, good])], "flac", 2, 32)
        assert np.array_equal(ok.astype(np.float64) * 32768.0, np.concatenate([want, want], axis=1)), name
    # a failure in the second launch set (8 blocks of 64 = 512 frames a set): the first set is delivered, zeros behind it
    with pytest.raises(ElemHipError) as e:
        rt.process_blocks_pcm_io([chunk([good] * 35 + [bytes(crc)] + [good] * 4)], "flac", 2, 640)
    assert e.value.code == 106 and rt.flac_in_error()["frame"] == 35
    part = e.value.result
    assert np.array_equal(part[:, :512].astype(np.float64) * 32768.0, np.concatenate([want] * 32, axis=1)) and not part[:, 512:].any()
    fails(chunk([good], bits=32), 8)                      # a 32-bit stream
    fails(chunk([good]), 8, in_channels_per_stream=1)     # channels_per_stream unequal to the stream's channels
    assert np.array_equal(rt.process_blocks_pcm_io([chunk([good])], "flac", 2, 16).astype(np.float64) * 32768.0, want)


def test_host_decode_path_answers_the_code_too(gpu_required):
    """Host block 700 with taps renders block by block and decodes on the host (decode_host): the same code, the same record."""
    from elementary_amd.runtime import ElemHipError, FlacChunk
    good, chans = good_frame()
    crc = bytearray(good)
    crc[-1] ^= 1

    def chunk(frames):
        data = b"".join(frames)
        off = np.cumsum([0] + [len(f) for f in frames])
        return FlacChunk(np.frombuffer(data, dtype=np.uint8), off, 16 * np.arange(len(frames) + 1), 2, 16, 16 * len(frames), 0, 16 * len(frames))

    taps = lambda: [el.tapOut({"name": "fb"}, el.add(el.in_({"channel": 0}), el.mul(0.5, el.tapIn({"name": "fb"})))), el.in_({"channel": 1})]   # noqa: E731
    a, b = _through(2, 700, taps()), _through(2, 700, taps())
    for name, frame, reason in (("crc", bytes(crc), 1), ("reserved_type", named_corrupt()["reserved_type"], 2), ("block_code0", named_corrupt()["block_code0"], 2)):
        with pytest.raises(ElemHipError) as e:
            a.process_blocks_pcm_io([chunk([good, good, frame, good])], "flac", 2, 64)
        err = a.flac_in_error()
        assert e.value.code == 106 and (err["stream"], err["frame"], err["reason"]) == (0, 2, reason), (name, err)
    # nothing was rendered by the failing calls: the next valid call equals a fresh twin's
    ok = chunk([good] * 50)
    assert _same(a.process_blocks_pcm_io([ok], "flac", 2, 800), b.process_blocks_pcm_io([ok], "flac", 2, 800))


def test_master_wav_masters_a_flac_file_like_the_wav_of_the_same_samples(gpu_required, tmp_path):
    from elementary_amd.master import master_wav
    from elementary_amd.runtime import flac_encode
    from elementary_amd.wav import WavWriter
    n = 48000
    t = np.arange(n)
    rng = np.random.RandomState(4)
    codes = np.stack([(9000 * np.sin(t * 0.05) + rng.randint(-300, 301, n)).astype(np.int32), (7000 * np.sin(t * 0.031) + rng.randint(-300, 301, n)).astype(np.int32)])
    data, _ = flac_encode(codes, bits=16, flac_frame=4096, sample_rate=48000)
    with open(tmp_path / "in.flac", "wb") as f:
        f.write(fw.file_bytes(data, 16, 2, 4096, n, rate=48000))
    with WavWriter(str(tmp_path / "in.wav"), "s16", 2, 48000) as w:
        w.write(np.ascontiguousarray(codes.T.astype(np.int16)))
    factory = lambda s, k: _hip(s, k, batch_blocks=8)      # noqa: E731
    ra = master_wav(factory, str(tmp_path / "in.flac"), str(tmp_path / "a.wav"), target_lufs=-16.0, fmt="s24")
    rb = master_wav(factory, str(tmp_path / "in.wav"), str(tmp_path / "b.wav"), target_lufs=-16.0, fmt="s24")
    assert ra == rb and np.isfinite(ra["input_lufs"])
    assert open(tmp_path / "a.wav", "rb").read() == open(tmp_path / "b.wav", "rb").read() and os.path.getsize(tmp_path / "a.wav") > n * 6
