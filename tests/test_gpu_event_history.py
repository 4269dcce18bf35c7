"""Option "event_history_blocks" on the GPU: `scope` and `fft` nodes with a device ring that keeps a whole relay window, and a
blockwise relay that replays the reference's per-block reads (elementary_amd/csrc/event_replay.h) — launch sets of full size with
such a listener attached, ring overruns included.

The reference is what test_gpu_events.py uses: the reference engine behind OfflineRenderer, relayed after every block, scope data
and meters within that file's TOL. fft spectra are held to the recording's bound, 2 * E_ref[size] (tests/fft_cases.py).
"""
import numpy as np
import pytest

import event_history_cases as eh
import fft_cases as fc
import test_gpu_events as ge
import test_gpu_fft as gf
from elementary_amd import el
from elementary_amd.offline import OfflineRenderer
from helpers import lcg_noise_fast

pytestmark = pytest.mark.gpu
TOL = ge.TOL
MAN = fc.manifest()


def _collect(factory, roots_fn, frames, n_in, n_out, bs, history=None, second=None, kinds=("meter", "scope", "fft")):
    """test_gpu_events._collect with the renderer's `event_history_blocks` keyword (None: initialize() is called without it)."""
    core = OfflineRenderer(factory)
    kw = {} if history is None else {"event_history_blocks": history}
    core.initialize(num_input_channels=n_in, num_output_channels=n_out, sample_rate=48000.0, block_size=bs, **kw)
    log = []
    for kind in kinds:
        core.on(kind, lambda p, kind=kind: log.append((kind, p)))
    core.render(*roots_fn())
    x = [lcg_noise_fast(frames, 11 + c, 0.5) for c in range(n_in)]
    out = [np.zeros(frames, np.float32) for _ in range(n_out)]
    core.process(x, out)
    if second is not None:
        core.render(*second())
        out2 = [np.zeros(frames, np.float32) for _ in range(n_out)]
        core.process(x, out2)
        out = [np.concatenate([a, b]) for a, b in zip(out, out2)]
    return log, np.stack(out), core


def _scope_roots(size, gain=0.5):
    def roots():
        x = el.in_({"channel": 0})
        return [el.scope({"name": "sc", "size": size, "channels": 2}, x, el.mul(gain, x)), el.meter({"name": "m"}, el.mul(gain, x))]
    return roots


def test_scope_at_or_above_the_block_through_full_launch_sets(gpu_required):
    """Scope of 256 frames, two channels, beside a meter, block 128, 200 blocks, history 256: the reference's events one for one,
    the same samples, a window of 256 (the 8192-frame rule gives 61) and ONE engine call rendered as launch sets."""
    a, ya, core = _collect(ge._hip, _scope_roots(256), 200 * 128, 1, 2, 128, history=256)
    b, yb, _ = _collect(ge._ref, _scope_roots(256), 200 * 128, 1, 2, 128)
    assert len([1 for k, _ in b if k == "scope"]) >= 90 and len([1 for k, _ in b if k == "meter"]) == 200
    ge._same_events(a, b)
    assert float(np.abs(ya - yb).max()) <= TOL
    assert core.runtime.event_window_blocks() == 256
    st = core.runtime.stats()
    # 200 single-block calls would leave no launch set behind; the first blocks, while the roots fade in, go block by block
    assert st["blocks_rendered"] == 200 and st["batch_launches"] >= 1, st


def test_scope_below_the_block_overruns_as_the_reference_does(gpu_required):
    """Scope of 256 frames at block 512: every block brings twice what a relay takes, the reference's ring overruns from about
    block 30 on and skips frames. 96 blocks in one window of 96 (the 8192-frame rule allows one): the reference's events."""
    a, ya, core = _collect(ge._hip, _scope_roots(256), 96 * 512, 1, 2, 512, history=96)
    b, yb, _ = _collect(ge._ref, _scope_roots(256), 96 * 512, 1, 2, 512)
    assert core.runtime.event_window_blocks() == 96
    assert len([1 for k, _ in b if k == "scope"]) == 96
    ge._same_events(a, b)
    assert float(np.abs(ya - yb).max()) <= TOL
    st = core.runtime.stats()
    assert st["blocks_rendered"] == 96 and st["batch_launches"] >= 1, st


def test_scope_positions_carry_over_a_rerender(gpu_required):
    """test_blockwise_relay_with_a_scope_and_a_rerender's shape with history 64: 64 blocks, a re-render that keeps the scope node
    (the meter gets a new input), 64 more — two windows of 64, the second replayed from where the first ended."""
    a, ya, core = _collect(ge._hip, _scope_roots(1024), 64 * 512, 1, 2, 512, history=64, second=_scope_roots(1024, 0.25))
    b, yb, _ = _collect(ge._ref, _scope_roots(1024), 64 * 512, 1, 2, 512, second=_scope_roots(1024, 0.25))
    assert core.runtime.event_window_blocks() == 64
    assert len([1 for k, _ in b if k == "scope"]) >= 60
    ge._same_events(a, b)
    assert float(np.abs(ya - yb).max()) <= TOL


def _offline_fft(sc, history):
    """test_gpu_fft's offline drive of a recorded scenario; returns (log, output, renderer, process calls that brought fft events)."""
    bs, n_out = sc["block"], sc["out_channels"]
    x = fc.scenario_input(MAN, sc)
    core = OfflineRenderer(lambda sr, b: gf._hip(sr, b))
    kw = {} if history is None else {"event_history_blocks": history}
    core.initialize(num_input_channels=1, num_output_channels=n_out, sample_rate=float(MAN["sample_rate"]), block_size=bs, **kw)
    log = []
    for kind in ("fft", "meter"):
        core.on(kind, lambda p, kind=kind: log.append((None, kind, p)))
    core.render(*fc.roots(sc, True, gf._keyed(sc)))
    cuts = sorted({(ch["after_block"] + 1) * bs for ch in sc["changes"]}) + [len(x)]
    outs, at, calls_with_fft = [], 0, 0
    for cut in cuts:
        out = [np.zeros(cut - at, np.float32) for _ in range(n_out)]
        before = len([1 for _, k, _ in log if k == "fft"])
        core.process([x[at:cut]], out)
        calls_with_fft += len([1 for _, k, _ in log if k == "fft"]) > before
        outs.append(np.stack(out))
        if cut < len(x):
            core.render(*fc.roots(sc, True, gf._overrides(sc, cut // bs - 1)))
        at = cut
    return log, np.concatenate(outs, axis=1), core, calls_with_fft


@pytest.mark.parametrize("name", [n for n in gf.SCENARIOS if MAN["scenarios"][n]["relay_every"] == 1])
def test_recorded_fft_scenario_in_one_window(gpu_required, name):
    """Every recorded scenario (relayed after every block, as the offline renderer relays) with a history of its whole length:
    the recorded events in the recorded order, spectra within 2 * E_ref of the recording — and every process call is ONE relay
    with ONE launch of the transform kernel for all its frames (b_size256: 40 frames of a ring that a one-block window served)."""
    sc = MAN["scenarios"][name]
    log, y, core, calls_with_fft = _offline_fft(sc, sc["blocks"])
    gf._check_events(name, sc, log, with_blocks=False)
    x = fc.scenario_input(MAN, sc)
    stored = int(MAN["out_stored"])
    rec = fc.recording()
    for c in range(sc["out_channels"]):
        head = rec[sc["out_offsets"][c]:sc["out_offsets"][c] + stored]
        assert float(np.abs(y[c, :stored] - head).max()) <= TOL and float(np.abs(y[c, stored:] - x[stored:]).max()) <= TOL, (name, c)
    per_host = (sc["block"] + 511) // 512
    assert core.runtime.event_window_blocks() == min(sc["blocks"], 1024 // per_host)
    st = core.runtime.stats()
    assert st["blocks_rendered"] == sc["blocks"] * per_host and st["batch_launches"] >= 1, st
    assert st["fft_frames"] == len(fc.fft_events(sc))
    assert st["fft_launches"] == calls_with_fft, (st["fft_launches"], calls_with_fft)
    assert calls_with_fft == (0 if name.startswith("d_") else 1 + len(sc["changes"]))


def test_fft_below_the_block_against_the_model(gpu_required):
    """fft of 256 frames at block 512, 96 blocks, history 96 — the overrun regime. The events sit at the blocks the ring model
    (tests/event_history_cases.py) gives: a meter beside the fft node reports once per block, so the meter events before an fft
    event count its block. Every spectrum is within 2 * E_ref[256] of a float64 DFT of the windowed frame at the
    model's position."""
    def roots():
        x = el.in_({"channel": 0})
        return [el.fft({"name": "f", "size": 256}, x), el.meter({"name": "m"}, x)]
    blocks, bs, size = 96, 512, 256
    log, _, core = _collect(ge._hip, roots, blocks * bs, 1, 2, bs, history=blocks, kinds=("fft", "meter"))
    want, _ = eh.model_events(bs, size, eh.AT_LEAST, blocks)
    assert len(want) == blocks and any(want[i + 1][1] != want[i][1] + size for i in range(len(want) - 1))     # frames are skipped
    got_blocks, meters, spectra = [], 0, []
    meter_first = log[0][0] == "meter"            # the two nodes' order inside a block is their render order, the same in every block
    for kind, p in log:
        if kind == "meter":
            meters += 1
        else:
            got_blocks.append(meters - 1 if meter_first else meters)
            spectra.append(p)
    assert meters == blocks and got_blocks == [b for b, _ in want], (meters, got_blocks[:8])
    x = lcg_noise_fast(blocks * bs, 11, 0.5)
    bound, worst = 2.0 * fc.e_ref(MAN, size), 0.0
    for (b, first), p in zip(want, spectra):
        assert p["source"] == "f"
        dft = np.fft.rfft(fc.windowed_frame(x, {"frame": first, "size": size}).astype(np.float64))
        re, im = np.asarray(p["data"]["real"], np.float64), np.asarray(p["data"]["imag"], np.float64)
        assert re.shape == (size // 2 + 1,) and im.shape == re.shape
        worst = max(worst, float(np.abs(re - dft.real).max()), float(np.abs(im - dft.imag).max()))
    print(f"size {size}, {len(want)} frames: max |engine - float64 DFT| {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound
    st = core.runtime.stats()
    assert core.runtime.event_window_blocks() == blocks and st["fft_launches"] == 1 and st["fft_frames"] == blocks, st


def test_option_off_is_the_engine_without_the_option(gpu_required):
    """`event_history_blocks = 0` handed to the renderer: the events, the samples and the window of a renderer that was never told."""
    a, ya, ca = _collect(ge._hip, _scope_roots(1024), 48 * 512, 1, 2, 512, history=0)
    b, yb, cb = _collect(ge._hip, _scope_roots(1024), 48 * 512, 1, 2, 512)
    assert a == b and len([1 for k, _ in a if k == "scope"]) >= 20
    assert ya.tobytes() == yb.tobytes()
    assert ca.runtime.event_window_blocks() == cb.runtime.event_window_blocks() == (8191 - 1024) // 512
    sc = MAN["scenarios"]["a_default"]
    la, ya, ca, _ = _offline_fft(sc, 0)
    lb, yb, cb, _ = _offline_fft(sc, None)
    assert la == lb and len(la) == len(sc["events"])
    assert ya.tobytes() == yb.tobytes()
    assert ca.runtime.event_window_blocks() == cb.runtime.event_window_blocks() == 14
    assert ca.runtime.stats()["fft_launches"] == cb.runtime.stats()["fft_launches"] == 3
