"""The inspector on the GPU (Runtime.qc; elementary_amd/csrc/qc.hip): every launch set of the host-buffer render calls inspected behind
its last level, the programme's summaries carried on the device from set to set, half to half and call to call. Every comparison is
against tests/qc_reference.py — numpy, a restatement of the definitions, not of the header — applied to the planar floats the SAME
calls returned: the exact fields with ==, the float64 sums within the bound that file derives. Graphs of gains over planar inputs,
after a settling call, so that what is planted in the inputs survives; every test asserts that what it planted was found."""
import numpy as np
import pytest

import qc_reference as ref
from elementary_amd import el
from elementary_amd.runtime import ElemHipError, qc_host, qc_launches
from test_gpu_noise_shape import GAINS, _roots as _gain_roots
from test_gpu_pcm import _hip, _inputs

pytestmark = pytest.mark.gpu

SR = 44100.0
CLIP = 4.0                  # above every gain times the noise; channel 3's gain 0.5 times 8.0 is exactly it
KW = dict(clip_level=CLIP, clip_run=3, dropout_frames=64)


def _planted(bs, n_out, frames, cut=None, S=None):
    """Inputs [n_out, frames], one per output channel (channel c = GAINS[c] * in[c]). Channel 0 carries the quiet plants, channel 1 the
    clipped ones and the non-finite samples, channel 2 is channel 0 again (gain -1.3 against 1.7: anti-phase), channel 3 is constant
    at clip_level, channel 4 silent. Offsets in set lengths S = 8 * bs (or the caller's, for a short programme: 7 S + 201 frames at
    least). Returns the inputs and what was planted."""
    S = 8 * bs if S is None else S
    assert frames > 7 * S + 201
    x = _inputs(frames, n_out)
    x[np.abs(x) < 1e-4] = np.float32(0.01)            # (no accidental digital silence)
    cut = 9 * bs + 5 if cut is None else cut
    plan = {}
    q = [(0, 2 * 64 + 5), (S - 3, S + 70), (3 * S + 11, 3 * S + 11 + 5 * S // 2), (6 * S + 20, 6 * S + 20 + 64), (6 * S + 120, 6 * S + 120 + 63)]
    for lo, hi in q:
        x[0, lo:hi] = 0.0
    plan["dropouts"] = 3                               # the three inner runs of at least 64 frames (the head is none, 63 too short)
    plan["quiet"] = sum(hi - lo for lo, hi in q)
    if n_out > 1:
        c = [(0, 4), (7 * S + 5, 7 * S + 7), (7 * S + 30, 7 * S + 33), (cut - 2, cut + 3), (frames - 6, frames)]
        for lo, hi in c:
            x[1, lo:hi] = 100.0
        x[1, 7 * S + 100] = np.nan
        x[1, 7 * S + 200] = np.inf
        plan["clip_events"] = 4                        # at frame 0, clip_run, across the call boundary, to the last frame (not clip_run - 1)
        plan["clipped"] = sum(hi - lo for lo, hi in c)          # (NaN and +inf are counted and then inspect as 0.0: not clipped)
    if n_out > 2:
        x[2] = x[0]
    if n_out > 3:
        x[3] = 8.0
    if n_out > 4:
        x[4] = 0.0
    return x, plan


def _pairs(n_out):
    return [(0, 2), (0, 1)] if n_out >= 3 else []


def _engine(bs, n_out, batch=8, **opts):
    a = _hip(SR, bs, batch_blocks=batch, **opts)
    assert a.render(*_gain_roots(n_out, n_out))["result"] == 0
    a.process_blocks_host(_inputs(32 * bs, n_out), n_out, 32 * bs)        # (the root fades settle: from here on the floats are gain * input)
    return a


def _found(got, plan, n_out, frames, what):
    """What was planted is what was found: non-zero and equal."""
    assert got["head_silence"][0] == 133 and got["dropouts"]["count"][0] == plan["dropouts"] > 0, (what, got["dropouts"])
    assert got["quiet_frames"][0] == plan["quiet"] > 0 and got["dropouts"]["longest"][0] == 5 * (8 * what[0]) // 2, what
    if n_out > 1:
        assert got["clip_events"]["count"][1] == plan["clip_events"] > 0 and got["clipped_frames"][1] == plan["clipped"], (what, got["clip_events"])
        assert got["clip_events"]["first_at"][1] == 0 and got["clip_events"]["longest"][1] == 6 and got["clip_events"]["longest_at"][1] == frames - 6
        assert got["nonfinite"][1] == 2 and got["nonfinite"][0] == 0
    if n_out > 2:
        # outputs are fl(g x), relative error <= u = 2^-24 each: sum_xy and both sum_sq are within (1 +- u)^2 of g_a g_b sum x^2 etc., so
        # the correlation is within about 8 u of -1; the summation errors (n 2^-53) vanish beside that
        assert abs(ref.correlation(got, 0) + 1.0) <= 8 * 2.0 ** -24 + 1e-9, ref.correlation(got, 0)
        assert abs(ref.correlation(got, 1)) < 0.2          # independent noise
    if n_out > 3:
        assert got["clipped_frames"][3] == frames and got["clip_events"]["count"][3] == 1 and got["clip_events"]["longest"][3] == frames
        assert got["min"][3] == got["max"][3] == np.float32(CLIP)
    if n_out > 4:
        assert got["head_silence"][4] == got["tail_silence"][4] == got["quiet_frames"][4] == frames and got["dropouts"]["count"][4] == 0


@pytest.mark.parametrize("n_out", [1, 3, 5])
@pytest.mark.parametrize("bs", [64, 512])
def test_planted_findings(gpu_required, bs, n_out):
    """75 blocks + 37 frames in sets of 8 blocks: ten sets, both halves, a cut last block; buckets of 96 and 1000 (dividing neither the
    block nor the set) and none; planar floats and s16 delivery. Whole sets of silence, a run across a set boundary, runs at the
    thresholds, clipped runs at frame 0 and to the last frame, NaN and inf, a silent and a constant channel, an anti-phase pair."""
    frames = 75 * bs + 37
    x, plan = _planted(bs, n_out, frames)
    a = _engine(bs, n_out)
    for bucket in (96, 1000, 0):
        a.qc(bucket=bucket, pairs=_pairs(n_out), **KW)
        before = qc_launches()
        if bucket == 1000 and n_out == 3:
            planar = a.process_blocks_pcm(x, 1, 3, frames, "s16", dither_seed=5, want_float=True)[2]
        else:
            planar = a.process_blocks_host(x, n_out, frames)
        got = a.qc_read()
        assert qc_launches() - before >= 20                # (ten sets, two or three kernels each)
        want = ref.inspect(planar, bucket=bucket, pairs=_pairs(n_out), **KW)
        ref.compare(got, want, (bs, n_out, bucket), overview=got["overview"])
        _found(got, plan, n_out, frames, (bs, n_out, bucket))
        assert got["delivered"] == got["programme_frames"] == frames
        again = a.qc_read()                                # a read does not disturb the programme; the buckets were drained
        assert ref.exact_bytes(again) == ref.exact_bytes(got) and again["overview"].shape[1] == 0 and again["first_bucket"] == (frames // bucket if bucket else 0)


def test_a_bucket_longer_than_a_set_and_sets_of_1024(gpu_required):
    """Block 64, bucket 65536: a bucket spans 128 sets of 8 blocks; then the same programme in one set of 1100 blocks."""
    bs, n_out, frames = 64, 3, 1100 * 64 + 37
    x, plan = _planted(bs, n_out, frames)
    seen = []
    for batch in (8, 1024):
        a = _engine(bs, n_out, batch)
        a.qc(bucket=65536, pairs=_pairs(n_out), **KW)
        planar = a.process_blocks_host(x, n_out, frames)
        got = a.qc_read()
        ref.compare(got, ref.inspect(planar, bucket=65536, pairs=_pairs(n_out), **KW), ("long bucket", batch), overview=got["overview"])
        assert got["overview"].shape[1] == 1 and got["open_bucket"]["frames"][0] == frames - 65536
        _found(got, plan, n_out, frames, (bs, n_out, 65536))
        seen.append((ref.exact_bytes(got), got["overview"].tobytes(), planar.tobytes()))
    assert seen[0] == seen[1]


def test_the_cut_into_calls_and_sets_changes_no_bit(gpu_required):
    """One call; after a reset three calls of 9 blocks + 5 frames, 41 blocks and the rest, with a read between them (the clipped run
    across the first boundary); once more in sets of 1024 blocks; and a second engine: the same bytes — every field, the sums, the
    overview."""
    bs, n_out, bucket = 512, 3, 1000
    frames = 75 * bs + 37
    cuts = [0, 9 * bs + 5, 9 * bs + 5 + 41 * bs, frames]
    x, plan = _planted(bs, n_out, frames)
    seen = []
    for batch in (8, 8, 1024):
        a = _engine(bs, n_out, batch)
        a.qc(bucket=bucket, pairs=_pairs(n_out), **KW)
        one = a.process_blocks_host(x, n_out, frames)
        r1 = a.qc_read()
        ref.compare(r1, ref.inspect(one, bucket=bucket, pairs=_pairs(n_out), **KW), ("one call", batch), overview=r1["overview"])
        a.qc_reset()
        empty = a.qc_read()
        assert empty["programme_frames"] == 0 and empty["overview"].shape[1] == 0 and empty["channels"] == 0
        parts, ov, r3 = [], [], None
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            parts.append(a.process_blocks_host(x[:, lo:hi], n_out, hi - lo))
            r3 = a.qc_read()
            ov.append(r3["overview"])
            sofar = np.concatenate(parts, axis=1)
            ref.compare(r3, ref.inspect(sofar, bucket=bucket, pairs=_pairs(n_out), **KW), ("call ending at", hi, batch), overview=np.concatenate(ov, axis=1))
        assert np.concatenate(parts, axis=1).tobytes() == one.tobytes()
        _found(r3, plan, n_out, frames, (bs, n_out, bucket))
        assert ref.exact_bytes(r3) == ref.exact_bytes(r1) and np.concatenate(ov, axis=1).tobytes() == r1["overview"].tobytes()
        seen.append((ref.exact_bytes(r1), r1["overview"].tobytes()))
    assert seen[0] == seen[1] == seen[2]


def test_it_only_reads(gpu_required):
    """With the inspector on and off: the s16 bytes with dither, the FLAC16 frames and the meter's sub-block sums are the same bytes;
    an engine whose inspector is off launches none of its kernels and refuses a read."""
    bs, n_out, frames = 512, 4, 40 * 512 + 11
    x, _ = _planted(bs, n_out, frames, S=1024)
    seen = []
    for mode in ("never", "off again", "on"):
        a = _engine(bs, n_out, loudness_meter=1)
        if mode != "never":
            a.qc(bucket=96, pairs=[(0, 1)], **KW)
        if mode == "off again":
            a.qc(None)
        before = qc_launches()
        streams, stats, planar = a.process_blocks_pcm(x, 2, 2, frames, "s16", dither_seed=3, want_float=True)
        a.set_option("flac_bits", 16)
        flac = a.process_blocks_flac(x, 2, 2, frames, dither_seed=3)
        tail = a.flac_flush()
        loud = a.loudness_read()
        seen.append(([s.tobytes() for s in streams], planar.tobytes(), {k: v.tobytes() for k, v in stats.items()}, list(flac[0]), list(tail),
                     loud["mean_squares"].tobytes(), loud["true_peak"].tobytes()))
        assert sum(len(f) for f in flac[0]) > 1000
        if mode == "on":
            assert qc_launches() > before
            got = a.qc_read()
            assert got["programme_frames"] == 2 * frames and got["clipped_frames"][3] == 2 * frames
        else:
            assert qc_launches() == before
            with pytest.raises(ElemHipError):
                a.qc_read()
    assert seen[0] == seen[1] == seen[2]


def test_behind_the_converter_with_a_window(gpu_required):
    """44100 -> 22050: `frames` is the delivered count and the report that of the delivered floats; with skip / limit, of that slice."""
    bs, n_out, frames = 512, 3, 30 * 512 + 99
    x, _ = _planted(bs, n_out, frames, S=1024)
    for skip, limit in ((0, 0), (301, 5000), (100, 0)):
        a = _engine(bs, n_out, resample_rate=22050)
        a.qc(bucket=96, pairs=_pairs(n_out), skip=skip, limit=limit, **KW)
        parts = [a.process_blocks_host(x[:, :13 * bs + 7], n_out, 13 * bs + 7), a.process_blocks_host(x[:, 13 * bs + 7:], n_out, frames - 13 * bs - 7)]
        planar = np.concatenate(parts, axis=1)
        assert planar.shape[1] != frames and abs(planar.shape[1] - frames // 2) < 200
        got = a.qc_read()
        want = ref.inspect(planar, bucket=96, pairs=_pairs(n_out), skip=skip, limit=limit, **KW)
        ref.compare(got, want, ("converter", skip, limit), overview=got["overview"])
        assert got["delivered"] == planar.shape[1] and got["frames"][0] == (min(limit, planar.shape[1] - skip) if limit else planar.shape[1] - skip) > 0
        assert got["quiet_frames"][0] > 0


def test_the_host_block_path(gpu_required):
    """Block 700 renders as two slices of 350 frames; a tap graph there goes host block by host block through the scalar twin, on the
    same carried state: the programme a launch-set call began goes on through it, and back — and the results are the twin's bytes for
    the same delivered floats."""
    bs, frames = 700, 9 * 700 + 211
    taps = [el.tapOut({"name": "fb"}, el.add(el.mul(1.5, el.in_({"channel": 0})), el.mul(0.5, el.tapIn({"name": "fb"})))),
            el.mul(0.9, el.in_({"channel": 1}))]
    gains = [el.mul(GAINS[c], el.in_({"channel": c})) for c in range(2)]
    kw = dict(bucket=96, pairs=[(1, 0)], clip_level=1.0, clip_run=3, dropout_frames=64)
    a = _hip(SR, bs, batch_blocks=8)
    assert a.render(*gains)["result"] == 0
    a.process_blocks_host(_inputs(8 * bs), 2, 8 * bs)
    a.qc(**kw)
    start = qc_launches()
    x = _inputs(frames)
    x[0, 1000:1100] = 0.0
    x[1, 50:60] = 3.0
    p0 = a.process_blocks_host(x, 2, frames)
    sets, launched = a.stats()["batch_launches"], qc_launches()
    assert launched > start                                # (launch sets, the kernels)
    assert a.render(*taps)["result"] == 0
    p1 = a.process_blocks_pcm(x, 1, 2, frames, "s16", want_float=True)[2]
    assert a.stats()["batch_launches"] == sets and qc_launches() == launched       # (the block-by-block path, the twin)
    mid = a.qc_read()
    assert a.render(*gains)["result"] == 0
    p2 = a.process_blocks_host(x, 2, frames)              # (sets again, or host blocks still while the taps fade out: the engine's choice)
    got = a.qc_read()
    planar = np.concatenate([p0, p1, p2], axis=1)
    ov = np.concatenate([mid["overview"], got["overview"]], axis=1)
    ref.compare(got, ref.inspect(planar, **kw), "sets, host blocks, sets", overview=ov)
    twin = qc_host(planar, **kw)[0]
    assert ref.exact_bytes(got) == ref.exact_bytes(twin) and ov.tobytes() == twin["overview"].tobytes()
    assert got["dropouts"]["count"][0] >= 2 and got["clip_events"]["count"][1] >= 2 and got["clip_events"]["first_at"][1] == 50


def test_a_refused_spec_changes_nothing_and_pairs_must_exist(gpu_required):
    bs, n_out, frames = 64, 2, 20 * 64
    a = _engine(bs, n_out)
    a.qc(clip_level=0.5, clip_run=1)
    with pytest.raises(ElemHipError) as e:
        a.qc(clip_level=0.0)
    assert e.value.code == 6
    planar = a.process_blocks_host(_inputs(frames, n_out), n_out, frames)
    got = a.qc_read()
    ref.compare(got, ref.inspect(planar, clip_level=0.5, clip_run=1), "the previous spec")
    assert got["clipped_frames"][0] > 0
    a.qc(pairs=[(0, 2)])
    with pytest.raises(ElemHipError) as e:
        a.process_blocks_host(_inputs(frames, n_out), n_out, frames)
    assert e.value.code == 6


def test_offline_renderer_and_the_report(gpu_required):
    from elementary_amd import qc as qcmod
    from elementary_amd.offline import OfflineRenderer
    bs, n_out, frames = 512, 3, 20 * 512 + 123
    core = OfflineRenderer(lambda s, n: _hip(s, n, batch_blocks=8))
    core.initialize(num_input_channels=n_out, num_output_channels=n_out, sample_rate=SR, block_size=bs, qc=dict(pairs=[(0, 2)], bucket=1000, **KW))
    core.render(*_gain_roots(n_out, n_out))
    x, _ = _planted(bs, n_out, frames, S=1024)
    _, _, planar = core.process_pcm(list(x), 1, 3, frames, "s16", want_float=True)
    got = core.qc()
    want = ref.inspect(planar, pairs=[(0, 2)], bucket=1000, **KW)
    ref.compare(got, want, "offline", overview=got["overview"])
    rep = qcmod.report(got, SR)
    assert rep["dc"].shape == (n_out,) and abs(rep["dc"][0] - want["sum"][0] / frames) <= 1e-12 and rep["head_silence_s"][0] > 0
    found = qcmod.findings(got, SR, max_head_s=0.001, max_tail_s=1.0, max_dc=1.0, min_correlation=0.0)
    kinds = {f["kind"] for f in found}
    assert {"head_silence", "dropout", "clip", "correlation"} <= kinds, kinds
    plain = OfflineRenderer(lambda s, n: _hip(s, n, batch_blocks=8))
    plain.initialize(num_input_channels=2, num_output_channels=2, sample_rate=SR, block_size=bs)
    with pytest.raises(RuntimeError):
        plain.qc()
