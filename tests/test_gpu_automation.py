"""Breakpoint automation on the GPU (elementary_amd/csrc/automation.hip, elemhip_automation_set): lanes bound to engine input channels
are expanded by a kernel in front of every launch set. The criterion everywhere is bit-for-bit equality with a second engine, built
identically, whose lane channels are fed the dense float32 arrays of tests/automation_reference.py as ordinary planar inputs.

Block size 64 and batch_blocks 8 (the smallest value that still renders launch sets): a set is 512 frames, and the render of
N = 27 * 64 + 37 frames spans four sets, the last one short and its last block cut."""
import numpy as np
import pytest

import automation_reference as ref
from elementary_amd import automation as au
from elementary_amd import el
from elementary_amd.offline import OfflineRenderer
from elementary_amd.runtime import ElemHipError, automation_launches
from helpers import lcg_noise_fast

pytestmark = pytest.mark.gpu

SR, BS, SET = 48000.0, 64, 8 * 64
N = 27 * BS + 37
H, L = au.HOLD, au.LINEAR


def _engine(lanes=None, bs=BS, roots=None, warm=True, **opts):
    """An engine with the graph committed and — `warm` — 2048 frames rendered, so that the roots have faded in (a call renders whole
    blocks, so the fade would otherwise depend on how a render is cut); then the lanes."""
    from elementary_amd.runtime import Runtime
    rt = Runtime(SR, bs, device=0)
    for k, v in dict(batch_blocks=8, **opts).items():
        rt.set_option(k, v)
    roots = roots or _roots()
    assert rt.render(*roots)["result"] == 0
    if warm:
        rt.process_blocks_host(np.zeros((1, 2048), dtype=np.float32), len(roots), 2048, sample_time=-4096)
    for c, p in (lanes or {}).items():
        rt.automation(c, p)
    return rt


def _roots():
    return [el.mul(el.in_({"channel": 0}), el.in_({"channel": 1})), el.in_({"channel": 2})]


def _x(frames=N):
    return lcg_noise_fast(frames, 17, 0.9).astype(np.float32)[None, :]


def _lanes(T=0):
    """Lane 1 — points on a block's first and last frame (64, 127), a linear
    segment that spans three sets (300 .. 1400), a jump in the middle of a row (1450: block 22 is frames 1408 .. 1471), a ramp that
    ends behind the render. Lane 2 — a point in front of the render, 190 points inside row 24 (frames 1536 .. 1599: three to a frame,
    more points than the row has frames), then a point on every frame of row 25 and beyond the render's last frame."""
    # (nothing lies between 300 and 1400, so the points on the sets' edges are a lane of their own: _set_edges)
    one = [(0, 0.25, L), (64, 0.5, H), (127, -0.5, L), (300, 1.0, L), (1400, -1.0, L), (1450, 0.75, L), (1450, -0.125, H), (1451, 0.3, L),
           (1500, 0.2, L), (N + 400, 2.0, H)]
    two = [(-1000, -1.0, L)] + [(1536 + k // 3, float(np.float32(np.cos(0.7 * k))), k % 2) for k in range(190)]
    two += [(1600 + k, float(np.float32(0.01 * k - 0.5)), (k + 1) % 2) for k in range(N - 1600 + 30)]
    return {1: [(f + T, v, c) for f, v, c in one], 2: [(f + T, v, c) for f, v, c in two]}


def _set_edges(T=0):
    """Points on the last and first frames of sets 0 | 1 and 1 | 2, linear through the boundary."""
    return [(f + T, v, c) for f, v, c in [(500, 0.0, L), (511, 1.0, L), (512, -1.0, L), (513, 0.5, H), (1023, 0.25, L), (1024, -0.75, L), (1100, 0.0, H)]]


def _dense(lanes, T, frames=N):
    return ref.dense(lanes, T, frames)


def _dense_in(x, lanes, T, channels=3, frames=N):
    """[channels, frames]: x's rows, then the lanes' dense arrays on their channels, zeros elsewhere."""
    out = np.zeros((channels, frames), dtype=np.float32)
    out[:x.shape[0]] = x[:, :frames]
    for c, v in _dense(lanes, T, frames).items():
        out[c] = v
    return out


def _same_stats(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("peak", "over", "nonfinite"))


def test_the_lanes_hold_what_the_docstring_says():
    """(no GPU work: the fixture's own shape)"""
    lanes = _lanes()
    for p in lanes.values():
        assert [q[0] for q in p] == sorted(q[0] for q in p)
    f1 = [q[0] for q in lanes[1]]
    assert {64, 127, 300, 1400, 1450, 1451}.issubset(f1) and f1.count(1450) == 2 and not any(300 < f < 1400 for f in f1)
    assert sum(1536 <= q[0] < 1600 for q in lanes[2]) == 190 > BS
    assert 300 // SET == 0 and 1400 // SET == 2


@pytest.mark.parametrize("T", [0, 1 << 33])
def test_process_blocks_host_parity(gpu_required, T):
    """Both lanes, the set-boundary lane in lane 2's place in a second round; sample times 0 and 2^33 with the lanes moved along give the
    same bytes."""
    x = _x()
    for lanes in (_lanes(T), {1: _set_edges(T), 2: _lanes(T)[1]}):
        a, d = _engine(lanes), _engine()
        before = automation_launches()
        got = a.process_blocks_host(x, 2, N, sample_time=T)
        assert automation_launches() - before == 4                 # one launch per set
        want = d.process_blocks_host(_dense_in(x, lanes, T), 2, N, sample_time=T)
        assert got.tobytes() == want.tobytes(), np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=0))[:8]
        assert got[0].any() and got[1].tobytes() == _dense(lanes, T)[2].tobytes()    # root1 = in2: the lane itself
        if T:
            base = {c: [(f - T, v, k) for f, v, k in p] for c, p in lanes.items()}
            assert _engine(base).process_blocks_host(x, 2, N, sample_time=0).tobytes() == got.tobytes()
        a.close(); d.close()


def test_process_blocks_pcm_parity(gpu_required):
    x, lanes, T = _x(), _lanes(), 0
    a, d = _engine(lanes), _engine()
    got = a.process_blocks_pcm(x, 1, 2, N, "s16", dither_seed=5, want_float=True, sample_time=T)
    want = d.process_blocks_pcm(_dense_in(x, lanes, T), 1, 2, N, "s16", dither_seed=5, want_float=True, sample_time=T)
    assert got[0][0].tobytes() == want[0][0].tobytes() and _same_stats(got[1], want[1]) and got[2].tobytes() == want[2].tobytes()
    assert got[0][0].any()


def test_process_blocks_pcm_io_parity(gpu_required):
    """in0 arrives as an s16 stream; the dense engine takes the floats that stream decodes to (code * 2^-15) next to the dense lanes."""
    x, lanes, T = _x(), _lanes(), 128
    codes = np.round(x[0] * 32767.0).astype(np.int16)[:, None]
    xf = (codes[:, 0].astype(np.float32) / np.float32(32768.0))[None, :]
    a, d = _engine(lanes), _engine()
    got = a.process_blocks_pcm_io([codes], "s16", num_outputs=2, num_frames=N, sample_time=T)
    want = d.process_blocks_host(_dense_in(xf, lanes, T), 2, N, sample_time=T)
    assert got.tobytes() == want.tobytes()
    got = a.process_blocks_pcm_io([codes], "s16", num_frames=N, out_fmt="s16", num_streams=2, channels_per_stream=1, dither_seed=9, want_float=True,
                                  sample_time=T)
    want = d.process_blocks_pcm(_dense_in(xf, lanes, T), 2, 1, N, "s16", dither_seed=9, want_float=True, sample_time=T)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got[0], want[0])) and _same_stats(got[1], want[1]) and got[2].tobytes() == want[2].tobytes()


def test_process_blocks_flac_parity(gpu_required):
    x, lanes, T = _x(), _lanes(), 0
    a, d = _engine(lanes, flac_frame=256), _engine(flac_frame=256)
    got = a.process_blocks_flac(x, 1, 2, N, bits=16, dither_seed=3, sample_time=T)
    want = d.process_blocks_flac(_dense_in(x, lanes, T), 1, 2, N, bits=16, dither_seed=3, sample_time=T)
    assert got[0] == want[0] and len(got[0][0]) > 0 and _same_stats(got[1], want[1])


def test_cuts_do_not_change_the_bits(gpu_required):
    """One call of N frames equals calls of 1, 63, 64, 65 and the rest, the caller advancing sample_time by the frames of each call."""
    x, lanes, T = _x(), _lanes(7), 7
    whole = _engine(lanes).process_blocks_host(x, 2, N, sample_time=T)
    a, at, parts = _engine(lanes), 0, []
    for n in (1, 63, 64, 65, N - 193):
        parts.append(a.process_blocks_host(x[:, at:at + n], 2, n, sample_time=T + at))
        at += n
    assert at == N and np.concatenate(parts, axis=1).tobytes() == whole.tobytes()
    assert whole.tobytes() == _engine().process_blocks_host(_dense_in(x, lanes, T), 2, N, sample_time=T).tobytes()


def test_unbound_channels_between_read_zeros(gpu_required):
    """A lane on channel 5, channels 3 and 4 unbound: the engine takes six inputs, 3 and 4 read zeros."""
    roots = _roots() + [el.add(el.in_({"channel": 3}), el.in_({"channel": 4})), el.in_({"channel": 5})]
    lanes = {**_lanes(), 5: _set_edges()}
    x = _x()
    a, d = _engine(lanes, roots=roots), _engine(roots=roots)
    assert a.automation_read(5)["inputs"] == 6
    # (stale rows first: a dense render through the same engine fills every row of both input halves)
    a.automation_reset()
    a.process_blocks_host(np.full((6, N), 0.5, dtype=np.float32), 4, N, sample_time=0)
    for c, p in lanes.items():
        a.automation(c, p)
    got = a.process_blocks_host(x, 4, N, sample_time=0)
    want = d.process_blocks_host(_dense_in(x, lanes, 0, channels=6), 4, N, sample_time=0)
    assert got.tobytes() == want.tobytes() and not got[2].any() and got[3].tobytes() == _dense(lanes, 0)[5].tobytes()


def test_supplying_a_bound_channel_is_refused(gpu_required):
    x, lanes = _x(), _lanes()
    a, d = _engine(lanes), _engine()
    rendered = a.stats()["blocks_rendered"]
    out = np.full((2, N), 7.0, dtype=np.float32)
    with pytest.raises(ElemHipError) as e:
        a.process_blocks_host(np.concatenate([x, x]), 2, N, out=out, sample_time=0)
    assert e.value.code == 6 and (out == 7.0).all() and a.stats()["blocks_rendered"] == rendered
    with pytest.raises(ElemHipError) as e:
        a.process_blocks_pcm(np.concatenate([x, x, x]), 1, 2, N, "s16", sample_time=0)
    assert e.value.code == 6 and a.stats()["blocks_rendered"] == rendered
    got = a.process_blocks_host(x, 2, N, sample_time=0)
    assert got.tobytes() == d.process_blocks_host(_dense_in(x, lanes, 0), 2, N, sample_time=0).tobytes()


def test_the_block_by_block_host_path_gives_the_launch_sets_bits(gpu_required):
    """A host block of 521 frames renders as ragged slices (512 + 9), host block by host block through process(): the lane channels come
    from the scalar twin there. Same bits as the dense inputs on that engine, and — the graph is stateless — as the launch sets of
    the 64-frame engine."""
    x, lanes, T = _x(), _lanes(3), 3
    a, d = _engine(lanes, bs=521), _engine(bs=521)
    before = automation_launches()
    got = a.process_blocks_host(x, 2, N, sample_time=T)
    assert automation_launches() == before                          # (no kernel on this path)
    assert got.tobytes() == d.process_blocks_host(_dense_in(x, lanes, T), 2, N, sample_time=T).tobytes()
    assert got.tobytes() == _engine(lanes).process_blocks_host(x, 2, N, sample_time=T).tobytes()
    s1 = a.process_blocks_pcm(x, 1, 2, N, "s16", dither_seed=5, sample_time=T)
    s2 = _engine(lanes).process_blocks_pcm(x, 1, 2, N, "s16", dither_seed=5, sample_time=T)
    assert s1[0][0].tobytes() == s2[0][0].tobytes() and _same_stats(s1[1], s2[1])


def test_input_rate_leaves_the_lanes_at_the_engine_rate(gpu_required):
    """Option input_rate on: in0 arrives at 44100 and is converted, the lanes bypass the converter — frame f of a call is still evaluated
    at sample_time + f in ENGINE frames. Against the same engine fed in0 alone, in the second call of a programme (the roots have
    faded in by then): root1 is the lane itself, and root0 is that engine's converted in0 times the dense lane, rounded once."""
    T = 11
    lanes = _lanes(T + 2048)
    a, d = _engine(lanes, warm=False, input_rate=44100), _engine(warm=False, input_rate=44100, roots=[el.in_({"channel": 0})])
    n1, n2 = a.input_resample_frames(2048), 0
    a.process_blocks_host(_x(n1), 2, 2048, sample_time=T)
    d.process_blocks_host(_x(n1), 1, 2048, sample_time=T)
    n2 = a.input_resample_frames(N)
    assert n2 == d.input_resample_frames(N) and n2 != N
    x = _x(n1 + n2)[:, n1:]
    got = a.process_blocks_host(x, 2, N, sample_time=T + 2048)
    conv = d.process_blocks_host(x, 1, N, sample_time=T + 2048)
    dense = _dense(lanes, T + 2048)
    assert got[1].tobytes() == dense[2].tobytes()
    assert got[0].tobytes() == (conv[0] * dense[1]).astype(np.float32).tobytes() and conv[0].any()


def test_off_means_no_launch_and_reset_means_off(gpu_required):
    x = _x()
    fresh = _engine()
    before = automation_launches()
    want = fresh.process_blocks_host(x, 2, N, sample_time=0)
    assert automation_launches() == before
    a = _engine(_lanes())
    a.process_blocks_host(x, 2, N, sample_time=0)
    assert automation_launches() > before
    a.automation_reset()
    before = automation_launches()
    got = a.process_blocks_host(x, 2, N, sample_time=0)
    assert automation_launches() == before and got.tobytes() == want.tobytes() and not got.any()      # (in1 and in2 are missing: zeros)


def test_offline_renderer_automate_in_seconds_writes_the_dense_file(gpu_required, tmp_path):
    """automate(unit="seconds") and write_wav in engine calls of 640 frames: the file of the render fed the dense arrays."""
    x = _x()
    secs = {1: [(0.0, 0.0, "linear"), (0.0101, 1.0, "linear"), (0.0250, 0.25, "hold"), (0.0301, -0.5, "linear"), (0.5, 1.0, "hold")],
            2: [(-0.001, 1.0, "linear"), (0.02, -1.0, "hold")]}
    frames = {c: au.normalise([(int(round(s * SR)), v, k) for s, v, k in p]) for c, p in secs.items()}
    assert frames[1][1][0] == 485 and frames[1][3][0] == 1445
    paths = []
    for lanes_on in (True, False):
        r = OfflineRenderer(lambda sr, bs: _engine(bs=bs))
        r.initialize(num_input_channels=1 if lanes_on else 3, num_output_channels=2, sample_rate=SR, block_size=BS)
        r.render(*_roots())
        if lanes_on:
            r.automate(secs, unit="seconds")
            with pytest.raises(ValueError):
                r.automate({0: [(0.0, 1.0)]})                       # channel 0 is supplied
        ins = [x[0]] if lanes_on else list(_dense_in(x, frames, 0))
        paths.append(str(tmp_path / f"lanes{int(lanes_on)}.wav"))
        r.write_wav(paths[-1], ins, N, "s16", dither_seed=21, chunk_frames=640)
    a, b = open(paths[0], "rb").read(), open(paths[1], "rb").read()
    assert a == b and len(a) > 44 + 4 * N - 1 and any(a[44:])
