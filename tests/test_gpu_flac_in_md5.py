"""The STREAMINFO MD5 of FLAC inputs and resources on the GPU (option "flac_in_md5"; elementary_amd/csrc/flac_in_md5.hip): behind the
decode kernels of every launch set the decoded samples enter their stream's running digest, each stream sample once.

Every expected digest is hashlib.md5 over the reference samples packed by numpy as libFLAC hashes them (test_flac_in_md5_host.packed),
so nothing here has a tolerance. Engines are created with batch_blocks=8, so launch-set boundaries fall inside FLAC frames and the
boundary frames are decoded twice."""
import hashlib
import os

import numpy as np
import pytest

import flac_reference as ref
import flac_writer as fw
from elementary_amd import el
from elementary_amd.offline import OfflineRenderer
from test_flac_in_host import good_frame
from test_flac_in_md5_host import packed
from test_gpu_flac_in import _chunk, _long_stream, _same, _through
from test_gpu_pcm import _hip

pytestmark = pytest.mark.gpu
SR = 44100.0
ZERO = bytes(16)


def md5_of(chans, bps):
    return hashlib.md5(packed(chans, bps)).digest()


@pytest.fixture(scope="module")
def corpus():
    """The writer's corpus with the reference's decode of it and hashlib's digest (computed once, never changed)."""
    out = []
    for name, data, chans, bps, bs in fw.corpus():
        got = ref.decode_frames(data)[1]
        assert got == chans
        out.append((name, data, got, bps, bs, md5_of(got, bps)))
    return out


@pytest.fixture(scope="module")
def long_stream():
    data, chans = _long_stream()          # 2 channels of 16 bits: eleven frames of 192 samples and a tail of 17
    assert len(chans[0]) == 11 * 192 + 17 and len(packed(chans, 16)) > 2 * 4096          # (crosses the schedule's 4096-byte chunks)
    return data, chans, md5_of(chans, 16)


# ---- 1. the corpus ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [64, 512])
def test_corpus_digests_equal_hashlib_and_the_floats_do_not_change(gpu_required, corpus, bs):
    engines = {}
    for name, data, chans, bps, fbs, want in corpus:
        nch, total = len(chans), len(chans[0])
        if nch not in engines:
            engines[nch] = (_through(nch, bs, flac_in_md5=1), _through(nch, bs))
        on, off = engines[nch]
        on.flac_in_md5_reset()
        got = on.process_blocks_pcm_io([_chunk(data, nch, bps, fbs)], "flac", nch, total)
        slots = on.flac_in_md5()
        assert slots == {"state": [2], "md5": [want], "hashed": [total]}, (name, slots, want.hex())
        assert _same(got, off.process_blocks_pcm_io([_chunk(data, nch, bps, fbs)], "flac", nch, total)), name


# ---- 2. cuts ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [64, 512])
def test_cuts_hash_every_sample_once(gpu_required, long_stream, bs):
    data, chans, want = long_stream
    total = len(chans[0])
    whole = _chunk(data, 2, 16, 192)
    assert bs % 192 != 0                              # calls of whole engine blocks start and end inside FLAC frames
    n = ((total + bs - 1) // bs) * bs
    for step in (n, 1 * bs, 3 * bs, 7 * bs):
        a = _through(2, bs, flac_in_md5=1)
        for k in range(0, n, step):
            a.process_blocks_pcm_io([whole.at(k, min(step, n - k))], "flac", 2, min(step, n - k))
            if k + step < total - 192:
                assert a.flac_in_md5()["state"] == [1]
        assert a.flac_in_md5() == {"state": [2], "md5": [want], "hashed": [total]}, step


# ---- 3. ragged jobs -------------------------------------------------------------------------------------------------------------------------
def test_streams_of_different_lengths_complete_in_different_sets(gpu_required):
    lens = (2 * 192 + 17, 5 * 192 + 3, 11 * 192 + 17)          # sets of 8 blocks of 64: they end in sets 0, 1 and 4
    streams = [[fw._noise(n, 16, 70 + i)] for i, n in enumerate(lens)]
    chunks = [_chunk(fw.write_stream(c, 16, 192, subs=[dict(kind="FIXED", order=2, porder=0, params=[11])]), 1, 16, 192) for c in streams]
    a, b = _through(3, 64, flac_in_md5=1), _through(3, 64)
    n = 36 * 64
    got = a.process_blocks_pcm_io(chunks, "flac", 3, n)
    assert a.flac_in_md5() == {"state": [2, 2, 2], "md5": [md5_of(c, 16) for c in streams], "hashed": list(lens)}
    assert _same(got, b.process_blocks_pcm_io(chunks, "flac", 3, n))
    # cut after the first stream's end and before the others': one complete, two running
    a.flac_in_md5_reset()
    a.process_blocks_pcm_io([c.at(0, 512) for c in chunks], "flac", 3, 512)
    got = a.flac_in_md5()
    assert got["state"] == [2, 1, 1] and got["md5"] == [md5_of(streams[0], 16), ZERO, ZERO] and got["hashed"] == [lens[0], 576, 576]


# ---- 4. frame bytes that do not divide 64 ----------------------------------------------------------------------------------------------------
def test_three_channels_of_24_bits(gpu_required):
    chans = [fw._noise(7 * 64 + 5, 24, 80 + c, amp=0.9) for c in range(3)]
    data = fw.write_stream(chans, 24, 64, subs=[dict(kind="FIXED", order=1, porder=0, params=[18], method=1)] * 3)
    a = _through(3, 64, flac_in_md5=1)
    a.process_blocks_pcm_io([_chunk(data, 3, 24, 64)], "flac", 3, len(chans[0]))
    assert a.flac_in_md5() == {"state": [2], "md5": [md5_of(chans, 24)], "hashed": [len(chans[0])]}


# ---- 5. the state rules ----------------------------------------------------------------------------------------------------------------------
def test_state_rules(gpu_required, long_stream):
    from elementary_amd.runtime import ElemHipError, FlacChunk
    data, chans, want = long_stream
    total = len(chans[0])
    whole = _chunk(data, 2, 16, 192)
    a = _through(2, 64, flac_in_md5=1)
    broken = {"state": [3], "md5": [ZERO]}

    def slots():
        got = a.flac_in_md5()
        return {"state": got["state"], "md5": got["md5"]}

    # a render that starts behind the stream's first frame
    a.process_blocks_pcm_io([whole.at(300, 640)], "flac", 2, 640)
    assert slots() == broken
    a.process_blocks_pcm_io([whole.at(0, total)], "flac", 2, total)        # ... stays broken until the reset
    assert slots() == broken
    # a skipped range
    a.flac_in_md5_reset()
    assert a.flac_in_md5() == {"state": [], "md5": [], "hashed": []}
    a.process_blocks_pcm_io([whole.at(0, 256)], "flac", 2, 256)
    assert a.flac_in_md5() == {"state": [1], "md5": [ZERO], "hashed": [384]}          # (the covered frames, whole)
    a.process_blocks_pcm_io([whole.at(1024, 256)], "flac", 2, 256)
    assert slots() == broken
    # a frame that answers 106
    good, _ = good_frame()
    crc = bytearray(good)
    crc[-1] ^= 1
    frames = [good] * 3 + [bytes(crc)] + [good] * 2
    bad = FlacChunk(np.frombuffer(b"".join(frames), dtype=np.uint8), np.cumsum([0] + [len(f) for f in frames]), 16 * np.arange(len(frames) + 1),
                    2, 16, 16 * len(frames), 0, 16 * len(frames))
    a.flac_in_md5_reset()
    with pytest.raises(ElemHipError) as e:
        a.process_blocks_pcm_io([bad], "flac", 2, bad.count)
    assert e.value.code == 106 and slots() == broken
    # after the reset a full run completes; feeding the stream again from 0 without a reset changes nothing
    a.flac_in_md5_reset()
    a.process_blocks_pcm_io([whole], "flac", 2, total)
    assert a.flac_in_md5() == {"state": [2], "md5": [want], "hashed": [total]}
    a.process_blocks_pcm_io([whole], "flac", 2, total)
    a.process_blocks_pcm_io([whole.at(0, 200)], "flac", 2, 200)
    assert a.flac_in_md5() == {"state": [2], "md5": [want], "hashed": [total]}
    # a render that stops before the end
    a.flac_in_md5_reset()
    a.process_blocks_pcm_io([whole.at(0, 1000)], "flac", 2, 1000)
    assert a.flac_in_md5() == {"state": [1], "md5": [ZERO], "hashed": [1152]}
    # another stream under the running slot
    other = fw.write_stream([c[:500] for c in chans], 16, 192)
    a.process_blocks_pcm_io([_chunk(other, 2, 16, 192)], "flac", 2, 500)
    assert slots() == broken


# ---- 6. both render paths -----------------------------------------------------------------------------------------------------------------------
def test_the_block_by_block_host_path_gives_the_launch_sets_digest(gpu_required):
    data, chans = _long_stream(nch=1)
    total, want = len(chans[0]), md5_of(chans, 16)
    whole = _chunk(data, 1, 16, 192)
    sets = _through(1, 64, flac_in_md5=1)
    sets.process_blocks_pcm_io([whole], "flac", 1, total)
    assert sets.flac_in_md5() == {"state": [2], "md5": [want], "hashed": [total]}
    # host block 700 (two slices of 350) with taps: rendered host block by host block, the FLAC decoded and hashed on the host
    taps = lambda: [el.tapOut({"name": "fb"}, el.add(el.mul(1.5, el.in_({"channel": 0})), el.mul(0.5, el.tapIn({"name": "fb"}))))]   # noqa: E731
    a, b = _through(1, 700, taps(), flac_in_md5=1), _through(1, 700, taps())
    got = a.process_blocks_pcm_io([whole.at(0, 1400)], "flac", 1, 1400)
    assert a.flac_in_md5() == {"state": [1], "md5": [ZERO], "hashed": [1400]}
    got = np.concatenate([got, a.process_blocks_pcm_io([whole.at(1400, total - 1400)], "flac", 1, total - 1400)], axis=1)
    assert a.flac_in_md5() == sets.flac_in_md5()
    assert _same(got, b.process_blocks_pcm_io([whole], "flac", 1, total))


# ---- 7. behind the input-rate converter -----------------------------------------------------------------------------------------------------------
def test_input_rate_converter_behind_the_decoder(gpu_required, long_stream):
    data, chans, want = long_stream
    total = len(chans[0])
    a, b = _through(2, 64, input_rate=48000.0, flac_in_md5=1), _through(2, 64, input_rate=48000.0)
    whole = _chunk(data, 2, 16, 192)
    at = 0
    for n in (5 * 64 + 7, 9 * 64, 24 * 64):              # three calls: the input cursor walks through FLAC frames and past the end
        ni = a.input_resample_frames(n)
        assert ni == b.input_resample_frames(n)
        assert _same(a.process_blocks_pcm_io([whole.at(at, ni)], "flac", 2, n), b.process_blocks_pcm_io([whole.at(at, ni)], "flac", 2, n)), n
        at += ni
    assert at > total and a.flac_in_md5() == {"state": [2], "md5": [want], "hashed": [total]}


# ---- 8. files --------------------------------------------------------------------------------------------------------------------------------
def _renderer(n, bs, roots=None):
    core = OfflineRenderer(lambda s, k: _hip(s, k, batch_blocks=8))
    core.initialize(num_input_channels=n, num_output_channels=n, sample_rate=SR, block_size=bs)
    core.render(*(roots or [el.in_({"channel": c}) for c in range(n)]))
    return core


def _file(path, data, total, md5=None, rate=44100):
    raw = bytearray(fw.file_bytes(data, 16, 2, 192, total, rate=rate))
    if md5 is not None:
        raw[26:42] = md5
    path.write_bytes(bytes(raw))
    return str(path)


def test_process_wav_and_master_wav_verify_their_inputs(gpu_required, tmp_path, long_stream):
    from elementary_amd.master import master_wav
    from elementary_amd.runtime import FlacMd5Mismatch
    data, chans, want = long_stream
    total = len(chans[0])
    good = _file(tmp_path / "good.flac", data, total, want)
    stats = _renderer(2, 64).process_wav(good, str(tmp_path / "good.wav"), "s24", chunk_frames=5 * 64, verify_input=True)
    assert stats["input_md5"] == ["ok"]
    plain = _renderer(2, 64).process_wav(good, str(tmp_path / "plain.wav"), "s24", chunk_frames=5 * 64)
    assert "input_md5" not in plain and open(tmp_path / "good.wav", "rb").read() == open(tmp_path / "plain.wav", "rb").read()
    stats = _renderer(2, 64).process_wav(_file(tmp_path / "none.flac", data, total), str(tmp_path / "none.wav"), "s16", verify_input=True)
    assert stats["input_md5"] == ["absent"]
    stats = _renderer(2, 64).process_wav(good, str(tmp_path / "short.wav"), "s16", num_frames=640, verify_input=True)
    assert stats["input_md5"] == ["incomplete"]
    # a flipped bit in the announced digest
    flipped = bytearray(want)
    flipped[5] ^= 0x10
    with pytest.raises(FlacMd5Mismatch) as e:
        _renderer(2, 64).process_wav(_file(tmp_path / "flip.flac", data, total, bytes(flipped)), str(tmp_path / "flip.wav"), "s16", verify_input=True)
    assert (e.value.stream, e.value.expected, e.value.computed) == (0, bytes(flipped), want)
    assert e.value.output == [str(tmp_path / "flip.wav")] and os.path.getsize(tmp_path / "flip.wav") > total * 4          # closed, left in place
    # a stream written from altered samples — every CRC valid — that announces the original samples' digest
    altered = [list(c) for c in chans]
    altered[1][700] += 1
    subs = [dict(kind="FIXED", order=2, porder=0, params=[12]), dict(kind="FIXED", order=3, porder=0, params=[12], method=1)]
    redone = fw.write_stream(altered, 16, 192, subs=subs)
    assert ref.decode_frames(redone)[1] == altered
    forged = _file(tmp_path / "forged.flac", redone, total, want)
    with pytest.raises(FlacMd5Mismatch) as e:
        _renderer(2, 64).process_wav(forged, str(tmp_path / "forged.wav"), "s16", verify_input=True)
    assert (e.value.expected, e.value.computed) == (want, md5_of(altered, 16)) and os.path.exists(tmp_path / "forged.wav")
    # master_wav verifies in its metering pass and raises before the second pass opens the output
    factory = lambda s, k: _hip(s, k, batch_blocks=8)      # noqa: E731
    with pytest.raises(FlacMd5Mismatch) as e:
        master_wav(factory, forged, str(tmp_path / "mastered.wav"), target_lufs=-20.0, fmt="s16", block_size=64, verify_input=True)
    assert e.value.computed == md5_of(altered, 16) and not os.path.exists(tmp_path / "mastered.wav")
    # ... and masters a file that verifies (long enough for a loudness gate: 0.6 s, encoded by the host twin)
    from elementary_amd.runtime import flac_encode
    n = 26000
    t = np.arange(n)
    codes = np.stack([(9000 * np.sin(t * 0.05)).astype(np.int32), (7000 * np.sin(t * 0.031)).astype(np.int32)])
    raw = bytearray(fw.file_bytes(flac_encode(codes, bits=16, flac_frame=4096, sample_rate=44100)[0], 16, 2, 4096, n, rate=44100))
    raw[26:42] = md5_of(codes, 16)
    (tmp_path / "long.flac").write_bytes(bytes(raw))
    done = master_wav(factory, str(tmp_path / "long.flac"), str(tmp_path / "mastered.wav"), target_lufs=-20.0, fmt="s16", verify_input=True)
    assert done["input_md5"] == ["ok"] and os.path.getsize(tmp_path / "mastered.wav") > n * 4


def test_process_pcm_io_and_process_flac_verify_chunks(gpu_required, tmp_path, long_stream):
    from elementary_amd.flac import FlacReader
    from elementary_amd.runtime import FlacMd5Mismatch
    data, chans, want = long_stream
    total = len(chans[0])
    rd = FlacReader(_file(tmp_path / "good.flac", data, total, want))
    core = _renderer(2, 64)
    _, stats, _ = core.process_pcm_io([rd.read(total)], "flac", total, "s16", 1, 2, verify_input=True)
    assert stats["input_md5"] == ["ok"] == core.input_md5
    rd.seek(0)
    core.process_pcm_io([rd.read(total)], "flac", total, verify_input=True)          # floats back: the verdicts are the renderer's
    assert core.input_md5 == ["ok"]
    rd.seek(0)
    _, stats = core.process_flac([rd.read(total)], 1, 2, total, 16, in_fmt="flac", verify_input=True)
    assert stats["input_md5"] == ["ok"]
    bad = FlacReader(_file(tmp_path / "bad.flac", data, total, want[::-1]))
    with pytest.raises(FlacMd5Mismatch):
        core.process_pcm_io([bad.read(total)], "flac", total, verify_input=True)


# ---- 9. resources ------------------------------------------------------------------------------------------------------------------------------
def test_resources_carry_the_files_digest(gpu_required, tmp_path, long_stream):
    from elementary_amd.runtime import FlacMd5Mismatch
    data, chans, want = long_stream
    total = len(chans[0])
    whole = _chunk(data, 2, 16, 192)
    on, off = _hip(SR, 64, resource_load_frames=100, flac_in_md5=1), _hip(SR, 64, resource_load_frames=100)      # pieces that cut FLAC frames
    for name, rate in (("same", None), ("converted", 48000.0)):
        assert on.add_shared_resource_pcm(name, whole, sample_rate=rate) and off.add_shared_resource_pcm(name, whole, sample_rate=rate)
        assert on.shared_resource_md5(name) == {"state": 2, "md5": want}, name
        assert off.shared_resource_md5(name) == {"state": 0, "md5": ZERO}
        assert _same(on.shared_resource_read(name), off.shared_resource_read(name)), name
    assert on.shared_resource_info("converted")["frames"] != total
    assert on.add_shared_resource_pcm("part", whole.at(0, 1000)) and on.shared_resource_md5("part") == {"state": 1, "md5": ZERO}
    assert on.add_shared_resource_pcm("late", whole.at(400, total - 400)) and on.shared_resource_md5("late")["state"] != 2
    assert on.flac_in_md5() == {"state": [], "md5": [], "hashed": []}          # (a load has a record of its own: no input slot is touched)
    # files
    core = OfflineRenderer(lambda s, k: _hip(s, k, resource_load_frames=100))
    core.initialize(num_input_channels=0, num_output_channels=1, sample_rate=SR, block_size=64)
    good, bad = _file(tmp_path / "good.flac", data, total, want), _file(tmp_path / "bad.flac", data, total, want[::-1])
    assert core.update_virtual_file_system_files({"good": good}, verify=True) == {"good": True} and core.resource_md5 == {"good": "ok"}
    with pytest.raises(FlacMd5Mismatch) as e:
        core.update_virtual_file_system_files({"bad": bad}, verify=True)
    assert (e.value.stream, e.value.computed) == ("bad", want)
    assert core.runtime.shared_resource_info("bad")["frames"] == total          # the resource stays under its name


# ---- 10. off -------------------------------------------------------------------------------------------------------------------------------------
def test_off_every_slot_reports_state_0(gpu_required, long_stream):
    data, chans, _ = long_stream
    total = len(chans[0])
    a = _through(2, 64)
    a.process_blocks_pcm_io([_chunk(data, 2, 16, 192)], "flac", 2, total)
    assert a.flac_in_md5() == {"state": [0], "md5": [ZERO], "hashed": [0]}
    a.set_option("flac_in_md5", 0)
    a.process_blocks_pcm_io([_chunk(data, 2, 16, 192)], "flac", 2, total)
    assert a.flac_in_md5() == {"state": [0], "md5": [ZERO], "hashed": [0]}
