"""The `fft` analyzer node (wasm/FFT.h) on the GPU against recordings of the reference's wasm engine (tests/golden/fft_wasm.*).

Tolerances, all set by the recording (tests/golden/make_fft_golden.js):
  audio     bit-equal to the same graph without the fft node, and within 1e-6 of the recorded output
  events    count, block, order and `source` exactly the recording's
  spectra   max |engine - recording| <= 2 * E_ref[size], E_ref = the reference's own largest error against a float64 DFT
The achieved figures are printed before they are asserted.
"""
import sys
import threading
import time

import numpy as np
import pytest

import fft_cases as fc
from elementary_amd import el
from elementary_amd.offline import OfflineRenderer
from helpers import lcg_noise_fast

pytestmark = pytest.mark.gpu
TOL = 1e-6
MAN = fc.manifest()
SCENARIOS = sorted(MAN["scenarios"])


def _hip(sr, bs, spec=None):
    from elementary_amd.runtime import Runtime
    rt = Runtime(sr, bs, device=0)
    if spec is not None:
        rt.set_option("specialize", spec)
    return rt


def _keyed(sc):
    """Every fft node gets a `key`, so that a re-render with another `size` reaches the SAME node (the recording sets the property)."""
    return {k: {"key": f"fft{k}"} for k in range(len(sc["ffts"]))}


def _overrides(sc, after_block):
    ov = _keyed(sc)
    for ch in sc["changes"]:
        if ch["after_block"] <= after_block:
            k = next(i for i, f in enumerate(sc["ffts"]) if f["id"] == ch["id"])
            ov[k][ch["key"]] = ch["value"]
    return ov


def _per_block(sc, with_fft=True, spec=None):
    """The recording's own drive: one process call per block, a plain relay after every `relay_every`-th, property changes between."""
    bs, n_out = sc["block"], sc["out_channels"]
    rt = _hip(float(MAN["sample_rate"]), bs, spec)
    assert rt.render(*fc.roots(sc, with_fft, _keyed(sc)))["result"] == 0
    x = fc.scenario_input(MAN, sc)
    events, outs = [], []
    for b in range(sc["blocks"]):
        outs.append(rt.process(x[None, b * bs:(b + 1) * bs], n_out, bs))
        if (b + 1) % sc["relay_every"] == 0:
            events += [(b, kind, p) for kind, p in rt.process_queued_events()]
        if any(ch["after_block"] == b for ch in sc["changes"]):
            assert rt.render(*fc.roots(sc, with_fft, _overrides(sc, b)))["result"] == 0
    return events, np.concatenate(outs, axis=1), rt


def _check_events(name, sc, got, with_blocks=True):
    """`got`: [(block or None, kind, payload)] against the scenario's recorded events; returns the worst spectrum errors per size."""
    want = sc["events"]
    assert len(got) == len(want), (name, len(got), len(want), [(b, k) for b, k, _ in got][:8], [(e["block"], e["type"]) for e in want][:8])
    rec, x = fc.recording(), fc.scenario_input(MAN, sc)
    worst = {}
    for i, ((b, kind, p), ev) in enumerate(zip(got, want)):
        assert kind == ev["type"] and p.get("source") == ev["source"], (name, i, kind, ev["type"], p.get("source"), ev["source"])
        if with_blocks:
            assert b == ev["block"], (name, i, b, ev["block"])
        if kind != "fft":
            continue
        size, bins = ev["size"], ev["size"] // 2 + 1
        re, im = np.asarray(p["data"]["real"], np.float64), np.asarray(p["data"]["imag"], np.float64)
        assert re.shape == (bins,) and im.shape == (bins,), (name, i, re.shape)
        dft = np.fft.rfft(fc.windowed_frame(x, ev).astype(np.float64))
        w = worst.setdefault(size, [0.0, 0.0])
        w[1] = max(w[1], float(np.abs(re - dft.real).max()), float(np.abs(im - dft.imag).max()))
        stored = fc.recorded_spectrum(rec, ev)
        if stored is not None:
            w[0] = max(w[0], float(np.abs(re - stored[0]).max()), float(np.abs(im - stored[1]).max()))
    for size, (e_rec, e_dft) in sorted(worst.items()):
        print(f"{name} size {size}: max |engine - recording| {e_rec:.3e} (bound {2 * fc.e_ref(MAN, size):.3e}), "
              f"max |engine - float64 DFT| {e_dft:.3e} (E_ref {fc.e_ref(MAN, size):.3e})")
    for size, (e_rec, _) in worst.items():
        assert e_rec <= 2.0 * fc.e_ref(MAN, size), (name, size, e_rec)
    return worst


def _check_audio(name, sc, y, y_plain):
    x, rec, stored = fc.scenario_input(MAN, sc), fc.recording(), int(MAN["out_stored"])
    assert y.tobytes() == y_plain.tobytes(), (name, "the fft node changed the audio")
    for c in range(sc["out_channels"]):
        head = rec[sc["out_offsets"][c]:sc["out_offsets"][c] + stored]
        assert float(np.abs(y[c, :stored] - head).max()) <= TOL, (name, c)
        assert float(np.abs(y[c, stored:] - x[stored:]).max()) <= TOL, (name, c)      # (recorded: the input itself, bit for bit)


def _expected_window(sc):
    per_host = (sc["block"] + 511) // 512
    w = max(1, 1024 // per_host)
    for k, f in enumerate(sc["ffts"]):
        size = _final_size(sc, k)
        if size < sc["block"]:
            return 1
        w = min(w, max(1, (8192 - size) // sc["block"]))
    return w


def _final_size(sc, k):
    size = sc["ffts"][k]["props"].get("size", 1024)
    for ch in sc["changes"]:
        if ch["id"] == sc["ffts"][k]["id"] and ch["key"] == "size":
            size = ch["value"]
    return size


@pytest.mark.parametrize("name", SCENARIOS)
def test_recorded_scenario_relayed_as_recorded(gpu_required, name):
    """Every recorded scenario driven as the recording was (a relay after every block, or every third): the same events at the
    same blocks, spectra within twice the reference's own error, audio bit-equal to the graph without the node."""
    sc = MAN["scenarios"][name]
    events, y, rt = _per_block(sc)
    _, y_plain, _ = _per_block(sc, with_fft=False)
    _check_events(name, sc, events)
    _check_audio(name, sc, y, y_plain)
    d = rt.describe_plan()
    n_fft = len(fc.fft_events(sc))
    assert d["fft_frames"] == n_fft and d["fft_launches"] <= max(n_fft, 0)      # the relay kernel made them: at most one launch per relay
    if name.startswith("i_"):
        assert d["fft_launches"] == sc["blocks"] and d["fft_frames"] > d["fft_launches"]   # two nodes' frames share one launch


@pytest.mark.parametrize("spec", [0, 2])
@pytest.mark.parametrize("name", [n for n in SCENARIOS if MAN["scenarios"][n]["relay_every"] == 1])
def test_recorded_scenario_through_the_offline_renderer(gpu_required, name, spec):
    """The same scenarios through OfflineRenderer.process over the whole stretch (launch sets + the blockwise relay, which replays
    the per-block `>= size` comparison): the same events in the same order; the window is the documented rule."""
    sc = MAN["scenarios"][name]
    bs, n_out = sc["block"], sc["out_channels"]
    x = fc.scenario_input(MAN, sc)

    def run(with_fft):
        core = OfflineRenderer(lambda sr, b: _hip(sr, b, spec))
        core.initialize(num_input_channels=1, num_output_channels=n_out, sample_rate=float(MAN["sample_rate"]), block_size=bs)
        log = []
        for kind in ("fft", "meter"):
            core.on(kind, lambda p, kind=kind: log.append((None, kind, p)))
        core.render(*fc.roots(sc, with_fft, _keyed(sc)))
        cuts = sorted({(ch["after_block"] + 1) * bs for ch in sc["changes"]}) + [len(x)]
        outs, at = [], 0
        for cut in cuts:
            out = [np.zeros(cut - at, np.float32) for _ in range(n_out)]
            core.process([x[at:cut]], out)
            outs.append(np.stack(out))
            if cut < len(x):
                core.render(*fc.roots(sc, with_fft, _overrides(sc, cut // bs - 1)))
            at = cut
        return log, np.concatenate(outs, axis=1), core
    log, y, core = run(True)
    _, y_plain, _ = run(False)
    _check_events(name, sc, log, with_blocks=False)
    _check_audio(name, sc, y, y_plain)
    window = core.runtime.event_window_blocks()
    assert window == _expected_window(sc), (name, window, _expected_window(sc))
    st = core.runtime.stats()
    assert st["blocks_rendered"] == sc["blocks"] * ((bs + 511) // 512)
    if window > 1:
        assert st["batch_launches"] >= 1, st
        if spec == 2:
            assert st["spec_launches"] > 0, st
    if name.startswith("b_"):
        assert window == 1                      # size 256 below the block: the ring overruns under any relay, only a relay per block reproduces where
    d = core.runtime.describe_plan()
    assert d["fft_frames"] == len(fc.fft_events(sc))
    assert d["fft_launches"] <= d["fft_frames"]
    if name.startswith("a_"):
        assert window == 14 and d["fft_launches"] == 3      # 40 blocks in windows of 14: three relays, three launches for 20 frames


def test_rejected_size_leaves_the_previous_size_in_force(gpu_required):
    """The recording: size 512, then a rejected 300 — still one 257-bin event per 512-frame block."""
    keep = MAN["rejected_keeps"]
    rt = _hip(48000.0, 512)
    assert rt.render(el.fft({"key": "f", "size": keep["size_before"]}, el.in_({"channel": 0})))["result"] == 0
    assert rt.render(el.fft({"key": "f", "size": keep["rejected"]}, el.in_({"channel": 0})))["result"] == 6
    x = lcg_noise_fast(512, 3, 0.5)[None, :]
    got = []
    for _ in range(keep["blocks"]):
        rt.process(x, 1, 512)
        got += rt.process_queued_events()
    assert len(got) == keep["events"] and all(len(p["data"]["real"]) == keep["bins"] for _, p in got)


def test_a_rerender_that_keeps_the_node_carries_its_ring_across(gpu_required):
    """Size 1024 at block 512: one block, a re-render that keeps the fft node (a meter root is added), one more block — the event
    after the second block is the transform of BOTH blocks' frames: the first recorded event of scenario (a)."""
    sc = MAN["scenarios"]["a_default"]
    x = fc.scenario_input(MAN, sc)
    rt = _hip(48000.0, 512)
    node = el.fft({"key": "fft0"}, el.in_({"channel": 0}))
    assert rt.render(node)["result"] == 0
    rt.process(x[None, :512], 1, 512)
    assert rt.process_queued_events() == []
    assert rt.render(node, el.meter({"name": "m"}, el.in_({"channel": 0})))["result"] == 0
    rt.process(x[None, 512:1024], 2, 512)
    got = [(1, k, p) for k, p in rt.process_queued_events() if k == "fft"]
    assert len(got) == 1
    first = dict(sc, events=[fc.fft_events(sc)[0]])
    _check_events("rerender", first, got)


def test_gc_of_a_dropped_fft_node_matches_other_analyzers(gpu_required):
    """gc.test.js:5-43 with an analyzer: the nodes of a replaced graph stay held while their root (faded out, still a current root)
    waits for the next rebuild, and go at the gc after it (Runtime.h:220-272, 368-433). The fft node and its ring are pruned exactly
    when a meter in the same place is; no event arrives from a root that was switched off."""
    pruned = {}
    for kind in ("fft", "meter"):
        rt = _hip(48000.0, 512)
        x = el.in_({"channel": 0})
        stats = rt.render(el.fft({"size": 512}, x) if kind == "fft" else el.meter({}, x))
        assert stats["result"] == 0
        node_id = next(i[1] for i in stats["batch"] if i[0] == 0 and i[2] == kind)
        xin = lcg_noise_fast(512, 3, 0.5)[None, :]
        rt.process(xin, 1, 512)
        assert [k for k, _ in rt.process_queued_events()] == [kind]
        assert rt.render(el.mul(0.5, x))["result"] == 0
        for _ in range(10):
            rt.process(xin, 1, 512)
        assert rt.process_queued_events() == []          # (its root is no longer active: GraphRenderSequence.h:192)
        second = rt.gc()
        assert node_id not in second, (kind, node_id, second)
        assert rt.render(el.mul(0.25, x))["result"] == 0
        for _ in range(10):
            rt.process(xin, 1, 512)
        third = rt.gc()
        assert node_id in third, (kind, node_id, third)
        pruned[kind] = (len(second), len(third))
        rt.process(xin, 1, 512)
        assert rt.process_queued_events() == []
    assert pruned["fft"] == pruned["meter"], pruned


def test_fft_relay_does_not_hold_up_the_render_thread(gpu_required):
    """test_gpu_events.py's standard for the relay, with fft nodes: a render thread calling elemhip_process block after block while a
    second thread relays as fast as it can — every relay launches the transform kernel (two nodes, size 512: a frame each per block)
    on the relay's stream. The render call's latency stays what it is without the poller (same bounds as the scope's test)."""
    rt = _hip(48000.0, 512)
    x = el.in_({"channel": 0})
    assert rt.render(el.fft({"name": "a", "size": 512}, x), el.fft({"name": "b", "size": 512}, el.mul(0.5, x)),
                     el.meter({"name": "m"}, el.lowpass(500.0, 0.7, x)))["result"] == 0
    xin = lcg_noise_fast(512, 3, 0.5)[None, :]
    for _ in range(50):
        rt.process(xin, 3, 512)

    def render_for(seconds):
        lat = []
        t_end = time.perf_counter() + seconds
        while time.perf_counter() < t_end:
            t0 = time.perf_counter()
            rt.process(xin, 3, 512)
            lat.append(1e6 * (time.perf_counter() - t0))
        lat.sort()
        return lat
    quiet = render_for(1.0)
    stop, polls, events = threading.Event(), [0], [0]

    def poll():
        while not stop.is_set():
            events[0] += len([1 for k, _ in rt.process_queued_events() if k == "fft"])
            polls[0] += 1
    th = threading.Thread(target=poll)
    old = sys.getswitchinterval()
    sys.setswitchinterval(1e-4)
    th.start()
    busy = render_for(1.5)
    stop.set(); th.join()
    sys.setswitchinterval(old)
    p = lambda a, q: a[min(len(a) - 1, int(q * len(a)))]
    print(f"render call us quiet p50 {p(quiet, 0.5):.1f} p99 {p(quiet, 0.99):.1f} | polled p50 {p(busy, 0.5):.1f} p99 {p(busy, 0.99):.1f} "
          f"| {polls[0]} relays, {events[0]} fft events in 1.5 s")
    assert polls[0] > 200 and events[0] > 100
    assert rt.describe_plan()["fft_launches"] > 50
    assert p(busy, 0.5) <= 2.0 * p(quiet, 0.5) + 30.0
    assert p(busy, 0.99) <= 3.0 * p(quiet, 0.99) + 150.0
