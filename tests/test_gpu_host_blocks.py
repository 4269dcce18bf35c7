"""The block-by-block host render (elementary_amd/csrc/engine_host_blocks.cpp) with EVERY delivery stage on at once: a tap graph under
a sliced host block goes through process() host block by host block, and the input decode, both rate converters, the limiter, the
meter, the PCM pack and the FLAC encode run on the host through the headers' scalar twins, their carried state brought over from the
device for the call. The yardstick is the launch-set path of the same engine: a channel that does not depend on the taps carries the
same bits whichever path rendered it. And a call that fails leaves the programmes as the unwind says: the meter's kept, the others' new."""
import numpy as np
import pytest

import flac_reference as fref
import limiter_reference as lref
import loudness_reference as loud_ref
from elementary_amd import el
from elementary_amd.runtime import ElemHipError, FlacChunk
from test_flac_in_host import good_frame
from test_gpu_limiter import _limited
from test_gpu_loudness import _check as _check_meter
from test_gpu_pcm import _check_call, _hip, _inputs
from test_gpu_resample_in import _encode, _same_bits
from test_resample_in_host import need
import resample_reference as rref

pytestmark = pytest.mark.gpu

SR, FIN, FOUT, HB = 48000.0, 44100, 44100, 700          # host block 700: two engine slices of 350
PARAMS = dict(ceiling_dbtp=-1.0, release_ms=50.0, lookahead_ms=1.5, link=1)
OPTS = dict(input_rate=FIN, resample_rate=FOUT, loudness_meter=1, flac_frame=256, batch_blocks=8)
# the inputs are _inputs() as it stands (scale 1.0): behind both converters and the 0.9 gain channel 1 peaks at 1.05 against a
# ceiling of 0.891, so the reference limiter works on most frames and idles on some — asserted below
SCALE = 1.0


def _plain():
    return [el.mul(1.7, el.in_({"channel": 0})), el.mul(0.9, el.in_({"channel": 1}))]


def _taps():
    """Channel 0 is the feedback tap; channel 1 the stateless root of _plain()."""
    return [el.tapOut({"name": "fb"}, el.add(el.mul(1.5, el.in_({"channel": 0})), el.mul(0.5, el.tapIn({"name": "fb"})))),
            el.mul(0.9, el.in_({"channel": 1}))]


def _reset_all(rt):
    rt.loudness_reset(); rt.resample_reset(); rt.input_resample_reset(); rt.limiter_reset(); rt.flac_reset()


def _reads(rt):
    """The programmes' read-outs: (what belongs to channel 1 — the meter's peaks, the limiter's group —, the programme-wide counters, the
    meter's series of channel 1)."""
    loud, lim, res, inp = rt.loudness_read(), rt.limiter_read(), rt.resample_read(), rt.input_resample_read()
    assert lim["groups"] == 2 and loud["channels"] == 2
    own = (loud["true_peak"][1].tobytes(), loud["sample_peak"][1].tobytes(), float(lim["max_reduction"][1]), int(lim["limited_frames"][1]))
    counters = (res["frames_in"], res["frames_out"], inp["frames_in"], inp["frames_out"], lim["frames"], loud["frames"])
    return own, counters, loud["mean_squares"][1].copy()


def test_every_stage_on_the_block_by_block_path_leaves_the_launch_sets_bits(gpu_required):
    """Input conversion 44100 -> 48000, delivery conversion back to 44100, the limiter (one group per channel), the meter, and FLAC or
    s24 delivery in mono streams: nothing of channel 1 depends on channel 0, so its FLAC bytes, PCM bytes, floats, meter peaks and
    limiter statistics under the tap graph (block by block, on the host) equal those under the plain graph (launch sets, on the GPU),
    and so do the programmes' clocks; the meter's series, sums, agree within the reference's bound. Two calls of 9 host blocks + 211
    frames: carried state crosses a call on both paths."""
    frames = 9 * HB + 211
    pl = rref.plan(FIN, int(SR))
    total = need(2 * frames, pl["L"], pl["M"])
    stream = _encode(SCALE * _inputs(total), "s16", 2)[0][0]
    settle = [np.zeros((need(frames, pl["L"], pl["M"]) + 8, 2), dtype=np.int16)]
    a = _limited(SR, HB, PARAMS, **OPTS)
    seen = {}

    def two_calls(rt, call):
        at, parts = 0, []
        for _ in range(2):
            ni = rt.input_resample_frames(frames)
            parts.append(call([stream[at:at + ni]]))
            at += ni
        assert at == total
        return parts

    for name, roots in (("sets", _plain()), ("taps", _taps())):
        assert a.render(*roots)["result"] == 0
        a.process_blocks_pcm_io(settle, "s16", num_outputs=2, num_frames=frames)          # (the roots' fade: 20 ms)
        got = {}
        # delivered as FLAC
        _reset_all(a)
        sets = a.stats()["batch_launches"]
        parts = two_calls(a, lambda ins: a.process_blocks_flac(ins, 2, 1, frames, 16, dither_seed=3, in_fmt="s16"))
        got["flac_samples"] = a.flac_read()["total_samples"]
        tail = a.flac_flush()
        got["flac"] = b"".join(p[0][1] for p in parts) + tail[1]
        got["flac_stats"] = [(p[1]["peak"][1].tobytes(), int(p[1]["over"][1]), int(p[1]["nonfinite"][1])) for p in parts]
        got["flac_own"], got["flac_counters"], got["flac_series"] = _reads(a)
        assert (a.stats()["batch_launches"] > sets) == (name == "sets")
        # delivered as s24 with the floats
        _reset_all(a)
        sets = a.stats()["batch_launches"]
        parts = two_calls(a, lambda ins: a.process_blocks_pcm_io(ins, "s16", num_frames=frames, out_fmt="s24", num_streams=2, channels_per_stream=1,
                                                                 dither_seed=3, want_float=True))
        assert (a.stats()["batch_launches"] > sets) == (name == "sets")                   # (the tap graph did take the block-by-block path)
        t0 = 0
        for streams, stats, planar in parts:
            _check_call(streams, stats, planar, 1, "s24", 3, t0)                          # (the dither's key: the programme's output frame)
            t0 += planar.shape[1]
        got["pcm"] = b"".join(p[0][1].tobytes() for p in parts)
        got["floats"] = np.concatenate([p[2][1] for p in parts])
        got["pcm_stats"] = [(p[1]["peak"][1].tobytes(), int(p[1]["over"][1]), int(p[1]["nonfinite"][1])) for p in parts]
        got["pcm_own"], got["pcm_counters"], got["pcm_series"] = _reads(a)
        _check_meter(a, np.concatenate([p[2] for p in parts], axis=1), float(FOUT), None, name)      # each path's meter against the reference
        seen[name] = got
    s, t = seen["sets"], seen["taps"]
    assert t["flac"] == s["flac"], (len(t["flac"]), len(s["flac"]))
    assert t["pcm"] == s["pcm"]
    assert _same_bits(t["floats"], s["floats"]), int((t["floats"].view(np.uint32) != s["floats"].view(np.uint32)).sum())
    for key in ("flac_stats", "pcm_stats", "flac_own", "pcm_own", "flac_counters", "pcm_counters", "flac_samples"):
        assert t[key] == s[key], (key, t[key], s[key])
    # The meter's sub-block sums are float64 sums whose order follows the cut into sets, segments and host blocks: the launch sets' series
    # is not the scalar loop's to the bit, nor one set size's another's (test_gpu_loudness.py::test_set_size_does_not_matter). Each is
    # within the reference's bound of the reference over the same floats, so the two are within twice that of each other; the peaks,
    # which are maxima, are equal (above).
    for key in ("flac_series", "pcm_series"):
        assert t[key].shape == s[key].shape and t[key].shape[0] >= 2 and s[key].min() > 0.0
        assert (np.abs(t[key] - s[key]) <= 2.0 * (loud_ref.BOUND_REL * s[key] + loud_ref.BOUND_ABS)).all(), (key, t[key].tolist(), s[key].tolist())
    delivered = s["floats"].shape[0]
    assert s["pcm_counters"] == (2 * frames, delivered, total, 2 * frames, delivered, delivered)
    assert s["flac_samples"] == [delivered // 256 * 256] * 2
    # the FLAC stream decodes, and to something
    decoded = fref.decode_frames(s["flac"], {"rate": FOUT, "bps": 16})[1]
    assert len(decoded) == 1 and len(decoded[0]) == delivered and np.array(decoded[0]).any()
    # not two idle limiters: over what a twin without the limiter delivers, the reference reduces some frames and leaves some alone
    twin = _hip(SR, HB, input_rate=FIN, resample_rate=FOUT, batch_blocks=8)
    assert twin.render(*_plain())["result"] == 0
    twin.process_blocks_pcm_io(settle, "s16", num_outputs=2, num_frames=frames)
    twin.resample_reset(); twin.input_resample_reset()
    floats = np.concatenate(two_calls(twin, lambda ins: twin.process_blocks_pcm_io(ins, "s16", num_outputs=2, num_frames=frames)), axis=1)
    want, g, _ = lref.limit(floats[1:2], float(FOUT), **PARAMS)
    print("limited share", float((g < 1.0).mean()), "idle share", float((g == 1.0).mean()), "peak in", float(np.abs(floats[1]).max()))
    assert (g < 1.0).any() and (g == 1.0).any()
    assert lref.within(s["floats"][None, :], want).all()


def test_a_failing_call_keeps_the_meter_and_starts_the_other_programmes_anew(gpu_required):
    """The tap graph at host block 700, fed FLAC through the input converter: a frame with a flipped CRC bit inside the first host
    block ends the call with code 106 before anything is rendered. The converters' and the limiter's programmes are then new, the
    meter's is what it was — and the engine goes on like a twin whose three programmes were reset by hand."""
    good, _ = good_frame()
    crc = bytearray(good)
    crc[-1] ^= 1
    n = 2 * HB + 211

    def chunk(frames):
        data = b"".join(frames)
        off = np.cumsum([0] + [len(f) for f in frames])
        return FlacChunk(np.frombuffer(data, dtype=np.uint8), off, 16 * np.arange(len(frames) + 1), 2, 16, 16 * len(frames), 0, 16 * len(frames))

    ok, broken = chunk([good] * 100), chunk([good, good, bytes(crc)] + [good] * 97)

    def call(rt, c):
        ni = rt.input_resample_frames(n)
        assert ni <= 1600
        streams, stats, planar = rt.process_blocks_pcm_io([c.at(0, ni)], "flac", num_frames=n, out_fmt="s24", num_streams=2, channels_per_stream=1,
                                                          dither_seed=3, want_float=True)
        return [s.tobytes() for s in streams], planar.tobytes(), [stats[k].tobytes() for k in ("peak", "over", "nonfinite")]

    def reads(rt):
        loud, lim = rt.loudness_read(), rt.limiter_read()
        return ({k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in loud.items()},
                {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in lim.items()}, rt.resample_read(), rt.input_resample_read())

    a, b = _limited(SR, HB, PARAMS, **OPTS), _limited(SR, HB, PARAMS, **OPTS)
    for rt in (a, b):
        assert rt.render(*_taps())["result"] == 0
        call(rt, ok)                                      # (the roots' fade: 20 ms)
    assert call(a, ok) == call(b, ok) and reads(a) == reads(b)
    before = reads(a)
    assert before[0]["frames"] > 0 and before[1]["frames"] > 0 and before[2]["frames_in"] == 2 * n and before[3]["frames_out"] == 2 * n
    with pytest.raises(ElemHipError) as e:
        call(a, broken)
    err = a.flac_in_error()
    assert e.value.code == 106 and (err["stream"], err["frame"], err["reason"]) == (0, 2, 1), (e.value.code, err)
    after = reads(a)
    assert after[2]["frames_in"] == 0 and after[2]["frames_out"] == 0 and after[3]["frames_in"] == 0 and after[3]["frames_out"] == 0
    assert after[1]["frames"] == 0
    assert after[0] == before[0]                          # the meter: frames, series and peaks
    assert a.stats()["batch_launches"] == 0
    b.resample_reset(); b.input_resample_reset(); b.limiter_reset()
    assert call(a, ok) == call(b, ok)
    assert reads(a) == reads(b)
