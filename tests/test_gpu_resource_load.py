"""Shared resources made on the GPU from a file's bytes (elemhip_add_shared_resource_pcm; elementary_amd/csrc/resource_load.hip). The
main checks need no tolerance: what ``shared_resource_read`` brings back equals, bit for bit, what a handle without a device makes of
the same bytes with the header's scalar loop (tests/test_resource_load_host.py holds that loop to a float64 restatement), and graphs
that read such a resource render the very floats of a twin engine that was handed ``add_shared_resource(decoded floats)``. The renders
are additionally held to the reference checker within the suite's tolerance, as tests/test_gpu_pcm_in.py does."""
import numpy as np
import pytest

import flac_writer as fw
import pcm_unpack_reference as uref
import resource_load_reference as rref
from elementary_amd import el
from test_gpu_events import TOL
from test_gpu_pcm import _checker, _hip

pytestmark = pytest.mark.gpu
SR, BS = 44100, 128


def _dry(sr=SR, bs=BS):
    from elementary_amd.runtime import Runtime
    return Runtime(sr, bs, device=-1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("rates", [(None, SR), (48000, SR), (44100, 96000)], ids=["same", "48000-44100", "44100-96000"])
@pytest.mark.parametrize("fmt", ["s16", "s24", "f32"])
def test_resource_equals_the_scalar_twin_bit_for_bit(gpu_required, fmt, rates):
    """G = 1, 2, 3 and N = 1, 255, 256, 257, 4099 with pieces of 256 source frames (seams inside tiles and tap windows) and the default
    (one piece); the floats behind a short resource's last frame, up to the block size, are zero."""
    fin, sr = rates
    cut, whole, twin = _hip(sr, BS, resource_load_frames=256), _hip(sr, BS), _dry(sr)
    for G in (1, 2, 3):
        for N in (1, 255, 256, 257, 4099):
            stream = uref.random_streams(fmt, N, G, 1, 1000 * G + N)[0]
            name = f"r{G}_{N}"
            assert twin.add_shared_resource_pcm(name, stream, fmt, G, sample_rate=fin) is True
            want = twin.shared_resource_read(name)
            frames = N if fin is None else rref.out_frames(N, fin, sr)
            assert want.shape == (G, frames)
            for rt in (cut, whole):
                assert rt.add_shared_resource_pcm(name, stream, fmt, G, sample_rate=fin) is True
                assert rt.shared_resource_info(name) == {"channels": G, "frames": frames}
                got = rt.shared_resource_read(name)
                assert np.array_equal(_bits(got), _bits(want)), (fmt, rates, G, N, int((_bits(got) != _bits(want)).sum()))
                if frames < BS:
                    for g in range(G):
                        pad = rt.shared_resource_read(name, g, frames, BS - frames)
                        assert pad.shape == (BS - frames,) and not _bits(pad).any(), (G, N, g)


def _flac(bits, n=1000, seed=5):
    from elementary_amd.runtime import FlacChunk, flac_index
    chans = [fw._noise(n, bits, seed + c) for c in range(2)]
    data = fw.write_stream(chans, bits, 256)
    off, first = flac_index(data, 2, bits, 256)
    pcm = np.array(chans, dtype=np.int32).T
    stream = pcm.astype(np.int16) if bits == 16 else uref.s24_bytes(pcm)
    return data, off, stream, lambda d: FlacChunk(np.frombuffer(bytes(d), dtype=np.uint8), off, first, 2, bits, n, 0, n)


@pytest.mark.parametrize("bits", [16, 24])
def test_flac_source_equals_the_pcm_of_the_same_samples(gpu_required, bits):
    """Stereo, FLAC blocks of 256, 1000 samples (a cut last frame), as one piece and in pieces of 256 frames that end inside FLAC
    frames' neighbours' tap windows; at the engine's rate and from 48000 Hz."""
    data, off, stream, chunk = _flac(bits)
    fmt = "s16" if bits == 16 else "s24"
    for frames in (256, 1 << 20):
        rt = _hip(SR, BS, resource_load_frames=frames)
        for rate in (None, 48000):
            assert rt.add_shared_resource_pcm(f"f{rate}", chunk(data), sample_rate=rate) and rt.add_shared_resource_pcm(f"p{rate}", stream, fmt, 2, sample_rate=rate)
            a, b = rt.shared_resource_read(f"f{rate}"), rt.shared_resource_read(f"p{rate}")
            assert a.shape == (2, 1000 if rate is None else rref.out_frames(1000, 48000, SR))
            assert np.array_equal(_bits(a), _bits(b)), (bits, frames, rate)
            assert np.abs(a).max() > 0.01


def test_a_broken_flac_crc_gives_106_and_no_resource(gpu_required):
    from elementary_amd.runtime import ElemHipError
    data, off, stream, chunk = _flac(16)
    bad = bytearray(data)
    bad[int(off[3]) - 1] ^= 1                                 # the CRC-16 of frame 2
    for frames in (256, 1 << 20):
        rt = _hip(SR, BS, resource_load_frames=frames)
        with pytest.raises(ElemHipError) as e:
            rt.add_shared_resource_pcm("broken", chunk(bad))
        err = rt.flac_in_error()
        assert e.value.code == 106 and err["frame"] == 2 and err["reason"] == 1, err
        with pytest.raises(ElemHipError) as e:
            rt.shared_resource_info("broken")
        assert e.value.code == 6
        assert rt.add_shared_resource_pcm("broken", chunk(data)) is True          # the engine stays usable, the name free


# ---- render parity ----------------------------------------------------------------------------------------------------------------------
def _graphs():
    rng = np.random.default_rng(11)
    ir = (rng.uniform(-1, 1, size=(300, 1)) * np.exp(-np.arange(300) / 60.0)[:, None] * 0.2)
    return {
        "table": (1, 512, lambda: [el.table({"path": "/r/x"}, el.phasor(130.0))]),
        "sample": (1, 700, lambda: [el.sample({"path": "/r/x"}, el.train(90.0), 1.0)]),
        "mc.sample": (2, 700, lambda: el.mc.sample({"path": "/r/x", "channels": 2, "mode": "loop", "playbackRate": 0.75}, el.train(2.0))),
        "convolve": (1, 300, lambda: [el.convolve({"path": "/r/x"}, el.mul(0.5, el.cycle(440.0)))], ir),
    }


@pytest.mark.parametrize("kind", ["table", "sample", "mc.sample", "convolve"])
def test_render_equals_the_float_path_bit_for_bit(gpu_required, kind):
    """8 blocks of 128: one engine loads s16 bytes on the GPU, its twin is handed the decoded floats; mc.sample reads the second
    channel's row, convolve builds its spectra from the lazily fetched host mirror."""
    spec = _graphs()[kind]
    G, N, roots = spec[0], spec[1], spec[2]
    if len(spec) > 3:
        stream = np.rint(spec[3] * 32767).astype(np.int16)
    else:
        stream = uref.random_streams("s16", N, G, 1, 21)[0]
    floats = rref.decode(stream, "s16")
    import oracle
    # (`convolve` is the wasm build's node: the suite holds it to the CPU restatement, as tests/test_gpu_convolve.py does)
    a, b, c = _hip(SR, BS), _hip(SR, BS), (oracle.PortRuntime(SR, BS) if kind == "convolve" else _checker(SR, BS))
    assert a.add_shared_resource_pcm("/r/x", stream, "s16", G) is True
    assert b.add_shared_resource("/r/x", floats) and c.add_shared_resource("/r/x", floats)
    n_out = len(roots())
    for rt in (a, b, c):
        assert rt.render(*roots())["result"] == 0
    got, twin = a.process_blocks_host(None, n_out, 8 * BS), b.process_blocks_host(None, n_out, 8 * BS)
    assert got.shape == (n_out, 8 * BS) and np.array_equal(_bits(got), _bits(twin)), (kind, int((_bits(got) != _bits(twin)).sum()))
    want = np.concatenate([c.process(None, n_out, BS) for _ in range(8)], axis=1)
    worst = float(np.abs(got - want).max())
    print(kind, "max abs err vs the reference engine", worst, "peak", float(np.abs(want).max()))
    assert np.abs(want).max() > 0.01 and worst <= TOL * max(1.0, float(np.abs(want).max())), kind


def test_an_engine_that_never_makes_the_call_is_untouched(gpu_required):
    """The `sample` graph on two engines fed with floats — one of them has loaded ANOTHER resource through the new call: the same
    floats, the same launch and plan counts."""
    spec = _graphs()["sample"]
    floats = rref.decode(uref.random_streams("s16", spec[1], 1, 1, 21)[0], "s16")
    a, b = _hip(SR, BS), _hip(SR, BS)
    assert b.add_shared_resource_pcm("/r/other", uref.random_streams("s24", 500, 2, 1, 3)[0], "s24", 2, sample_rate=48000)
    for rt in (a, b):
        assert rt.add_shared_resource("/r/x", floats) and rt.render(*spec[2]())["result"] == 0
    ya, yb = a.process_blocks_host(None, 1, 8 * BS), b.process_blocks_host(None, 1, 8 * BS)
    assert np.array_equal(_bits(ya), _bits(yb))
    sa, sb = a.stats(), b.stats()
    keys = [k for k in sa if "ms" not in k]
    assert keys and all(sa[k] == sb[k] for k in keys), {k: (sa[k], sb[k]) for k in keys if sa[k] != sb[k]}


def test_a_resource_loaded_into_a_running_engine(gpu_required):
    """Between two host-buffer calls of a running graph a resource is loaded and a graph that plays it rendered: the second call's
    output is that of an engine which had the resource from the start."""
    stream = uref.random_streams("s16", 600, 1, 1, 8)[0]
    first = lambda: [el.mul(0.3, el.cycle(220.0))]                                      # noqa: E731
    second = lambda: [el.add(el.mul(0.3, el.cycle(220.0)), el.table({"path": "/r/late"}, el.phasor(50.0)))]   # noqa: E731
    live, had = _hip(SR, BS), _hip(SR, BS)
    assert had.add_shared_resource_pcm("/r/late", stream, "s16", 1)
    for rt in (live, had):
        assert rt.render(*first())["result"] == 0
    y0, z0 = live.process_blocks_host(None, 1, 4 * BS), had.process_blocks_host(None, 1, 4 * BS)
    assert np.array_equal(_bits(y0), _bits(z0))
    assert live.add_shared_resource_pcm("/r/late", stream, "s16", 1)
    for rt in (live, had):
        assert rt.render(*second())["result"] == 0
    y1, z1 = live.process_blocks_host(None, 1, 4 * BS), had.process_blocks_host(None, 1, 4 * BS)
    assert np.array_equal(_bits(y1), _bits(z1)) and not np.array_equal(_bits(y1), _bits(y0))


def test_files_through_the_offline_renderer(gpu_required, tmp_path):
    """update_virtual_file_system_files: a 48 kHz WAV and the FLAC of the same samples give one resource, converted; resample=False
    takes the samples as they are."""
    from elementary_amd.offline import OfflineRenderer
    from elementary_amd.runtime import Runtime
    from elementary_amd.wav import WavWriter
    data, off, stream, chunk = _flac(16)
    with open(tmp_path / "a.flac", "wb") as f:
        f.write(fw.file_bytes(data, 16, 2, 256, 1000, rate=48000))
    with WavWriter(str(tmp_path / "a.wav"), "s16", 2, 48000) as w:
        w.write(np.ascontiguousarray(stream))
    core = OfflineRenderer(lambda sr, bs: Runtime(sr, bs, device=0))
    core.initialize(num_input_channels=0, num_output_channels=1, sample_rate=SR, block_size=BS)
    assert core.update_virtual_file_system_files({"wav": str(tmp_path / "a.wav"), "flac": str(tmp_path / "a.flac")}) == {"wav": True, "flac": True}
    assert core.update_virtual_file_system_files({"raw": str(tmp_path / "a.wav")}, resample=False) == {"raw": True}
    rt = core.runtime
    a, b, raw = rt.shared_resource_read("wav"), rt.shared_resource_read("flac"), rt.shared_resource_read("raw")
    assert a.shape == (2, rref.out_frames(1000, 48000, SR)) and np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(raw), _bits(rref.decode(stream, "s16")))
