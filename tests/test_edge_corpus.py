"""The edge corpus and its comparison (tests/edge_cases.py) checked on the CPU: the corpus reaches the edges it names — rendered
by the restatement, which test_oracle_vs_ref.py holds bit for bit against the reference engine on the same cases — and the
comparison helper rejects every kind of disagreement the GPU suite (test_gpu_edges.py) relies on it to reject."""
import numpy as np
import pytest

import edge_cases as E
import oracle

needs_port = pytest.mark.skipif(not oracle.have_port(), reason="needs the port (oracle/libelemoracle.so)")
_cache = {}


def _render(name, sr=44100.0, bs=512, blocks=8):
    if (name, sr, bs) not in _cache:
        rt = oracle.PortRuntime(sr, bs)
        for rname, data in E.edge_resources().items():
            assert rt.add_shared_resource(rname, data)
        roots = E.edge_roots(name, bs)
        assert rt.render(*roots)["result"] == 0
        _cache[(name, sr, bs)] = np.stack([rt.process(E.edge_inputs(k, bs), len(roots), bs, sample_time=k * bs) for k in range(blocks)])
    return _cache[(name, sr, bs)]


def test_inputs_hold_zeros_of_both_signs_and_ties():
    x = E.edge_inputs(3, 512)
    assert x.shape == (4, 512) and x.dtype == np.float32
    assert np.abs(x[:2]).max() <= 0.5
    z = x[2] == 0.0
    frames = np.arange(512)
    minus = frames % 11 == 3                                             # (a frame that is both gets -0.0)
    assert np.array_equal(z & np.signbit(x[2]), minus) and np.array_equal(z & ~np.signbit(x[2]), (frames % 7 == 0) & ~minus)
    assert np.array_equal(x[2][~z], x[0][~z])
    assert np.array_equal(x[3] * 4, np.round(x[3] * 4)) and (np.abs(x[3] % 1.0) == 0.5).any() and (x[3] % 1.0 == 0.0).any()
    assert (np.abs((2 * x[3]) % 1.0) == 0.5).any()


@needs_port
@pytest.mark.parametrize("name", ["math_domain", "nan_ordering", "nonfinite_into_state"])
def test_nonfinite_groups_are_nonfinite(name):
    y = _render(name)
    assert np.isnan(y).any() and (y == np.inf).any() and (y == -np.inf).any()
    assert np.isfinite(y).any(axis=(0, 2)).all()                    # ... and no root is non-finite throughout


@needs_port
def test_nonfinite_signal_is_the_input_elsewhere():
    """Root 0 of nonfinite_into_state is x0 bit for bit (behind the root's fade-in) except +inf, -inf and the NaN island where
    the docstring puts them."""
    y = _render("nonfinite_into_state")[:, 0]
    x0 = np.stack([E.edge_inputs(k, 512)[0] for k in range(8)])
    odd = ~np.isfinite(y)
    where = [(int(b), int(f)) for b, f in np.argwhere(odd)]
    assert where == [(2, 7), (4, 3)] + [(5, f) for f in (509, 510, 511)] + [(6, f) for f in range(5)]
    assert y[2, 7] == np.inf and y[4, 3] == -np.inf and np.isnan(y[5, 509:]).all()
    assert np.array_equal(y[2:][~odd[2:]].view(np.uint32), x0[2:][~odd[2:]].view(np.uint32))


@needs_port
def test_tiny_negative_phasor_outputs_exactly_one():
    y = _render("phasor_edges")
    assert (y[:, 1] == 1.0).any() and (y[:, 5] == 1.0).any()          # phasor(-0.001 Hz): as a constant, as a signal
    assert np.array_equal(y[:, 1], y[:, 5])
    assert (y[2:, 2] == 0.0).all()                                     # 0 Hz stays at phase 0


@pytest.mark.parametrize("bs", [512, 37, 64])
def test_ramped_delay_length_changes_sides_of_the_threshold(bs):
    """delay_ramp: of every four blocks two have their smallest length below n + 2 (run_delay's serial walk) and two at or above
    it (the sample-parallel branch); n + 2 + 60 x1 stays on the serial side, within 30 frames of the threshold."""
    t = np.arange(8 * bs, dtype=np.float64).reshape(8, bs)
    ramp = (np.float32(bs - 28.0) + np.float32(15.0 / bs) * np.mod(t, 4.0 * bs).astype(np.float32)).astype(np.float32)
    side = [bool(r.min() >= bs + 2) for r in ramp]
    assert side == [False, False, True, True] * 2
    noisy = [float((np.float32(bs + 2.0) + np.float32(60.0) * E.edge_inputs(k, bs)[1]).min()) for k in range(8)]
    assert all(bs + 2 - 30.001 <= m < bs + 2 for m in noisy)


def _pair(name="svf_clamps", shape=(2, 3, 16)):
    rng = np.random.default_rng(5)
    ref = rng.uniform(-1, 1, shape).astype(np.float32)
    return ref, ref.copy()


def test_compare_accepts_equal_and_within_tolerance():
    ref, got = _pair()
    ref[1, 2, 5], got[1, 2, 5] = np.nan, np.nan
    ref[0, 1, 3], got[0, 1, 3] = np.inf, np.inf
    ref[0, 1, 4], got[0, 1, 4] = -np.inf, -np.inf
    got[1, 0, 0] += np.float32(5e-7)
    E.compare_edges("svf_clamps", got, ref)


@pytest.mark.parametrize("kind", ["nan_missing", "nan_extra", "inf_sign", "inf_missing", "inf_extra", "off"])
def test_compare_rejects(kind):
    ref, got = _pair()
    if kind == "nan_missing":
        ref[1, 2, 5] = np.nan
    elif kind == "nan_extra":
        got[1, 2, 5] = np.nan
    elif kind == "inf_sign":
        ref[1, 2, 5], got[1, 2, 5] = np.inf, -np.inf
    elif kind == "inf_missing":
        ref[1, 2, 5], got[1, 2, 5] = np.inf, 3.0e38
    elif kind == "inf_extra":
        got[1, 2, 5] = np.inf
    else:
        got[1, 2, 5] += np.float32(3e-6)
    with pytest.raises(AssertionError, match=r"root 2, block 1, frame 5"):
        E.compare_edges("svf_clamps", got, ref)


def test_compare_is_per_sample_for_the_stateless_groups_and_per_root_for_the_others():
    ref, got = _pair()
    ref[0, 1, 0] = got[0, 1, 0] = 1000.0                                # a loud sample in root 1
    got[1, 1, 7] += np.float32(5e-4)                                    # 5e-4 off elsewhere in that root: inside 1e-6 * 1000
    E.compare_edges("svf_clamps", got, ref)
    with pytest.raises(AssertionError, match=r"root 1, block 1, frame 7"):
        E.compare_edges("math_domain", got, ref)
    got[0, 1, 0] = np.float32(1000.0005)                                # per sample: 1e-6 * |ref|
    got[1, 1, 7] = ref[1, 1, 7]
    E.compare_edges("math_domain", got, ref)


def test_compare_holds_the_float_recurrences_to_their_bits():
    ref, got = _pair(shape=(2, 12, 16))
    got[1, 3, 2] = np.nextafter(got[1, 3, 2], np.float32(2.0))
    E.compare_edges("svf_clamps", got, ref)
    with pytest.raises(AssertionError, match=r"root 3, block 1, frame 2"):
        E.compare_edges("phasor_edges", got, ref)
    with pytest.raises(AssertionError, match=r"root 3, block 1, frame 2"):
        E.compare_edges("nonfinite_into_state", got, ref)
    got[1, 3, 2] = ref[1, 3, 2]
    got[1, 9, 2] = np.nextafter(got[1, 9, 2], np.float32(2.0))          # root 9 (an SVF) is held to 1e-6, not to its bits
    E.compare_edges("nonfinite_into_state", got, ref)
