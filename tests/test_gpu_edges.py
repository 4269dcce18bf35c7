"""The HIP engine against the reference engine on the edge corpus (tests/edge_cases.py): clamps, domain edges, non-finite
samples and the clock far from zero, on each of the three render paths — process() block by block through the interpreter
kernels (8 blocks from the first), interpreter launch sets at a block that is no multiple of 64, specialised launch sets. The
engine renders launch sets only once every root's 20 ms fade-in has settled — 52 blocks of 37 frames at 96 kHz, 15 of 64 at
48 kHz — so the two launch-set paths render those blocks first (block by block inside the same call, compared like the rest)
and then the 8 blocks in sets of 3; the timed events of the corpus count from the first of the 8. The comparison leaves out no
sample (edge_cases.compare_edges): NaN where the reference has NaN, the same infinity, 1e-6 elsewhere, equal bits for the
float recurrences."""
import numpy as np
import pytest

import edge_cases as E
from test_gpu_spec import _assert_ran_specialised, _checker

pytestmark = pytest.mark.gpu
NB = 8
PATHS = {
    # name: (sample rate, block, options)
    "process": (44100.0, 512, {}),
    "sets": (96000.0, 37, {"specialize": 0, "batch_blocks": 3}),
    "spec": (48000.0, 64, {"specialize": 2, "batch_blocks": 3}),
}
_ref_cache = {}


def _first(path):
    sr, bs, _ = PATHS[path]
    return 0 if path == "process" else E.settle_blocks(sr, bs)


def _reference(name, path, start):
    """The reference engine's render of (case, path, first sample_time): computed once, shared, never written to."""
    key = (name, path, start)
    if key not in _ref_cache:
        sr, bs, _ = PATHS[path]
        c = _checker(sr, bs)
        for rname, data in E.edge_resources().items():
            assert c.add_shared_resource(rname, data)
        first = _first(path)
        roots = E.edge_roots(name, bs, first)
        assert c.render(*roots)["result"] == 0
        ref = np.stack([c.process(E.edge_inputs(k, bs), len(roots), bs, sample_time=start + k * bs) for k in range(first + NB)])
        ref.setflags(write=False)
        _ref_cache[key] = ref
    return _ref_cache[key]


def _render_hip(name, path, start):
    import torch
    from elementary_amd.runtime import Runtime
    sr, bs, opts = PATHS[path]
    rt = Runtime(sr, bs, device=0)
    for k, v in opts.items():
        rt.set_option(k, v)
    for rname, data in E.edge_resources().items():
        assert rt.add_shared_resource(rname, data)
    first = _first(path)
    nb = first + NB
    roots = E.edge_roots(name, bs, first)
    n_out = len(roots)
    assert rt.render(*roots)["result"] == 0
    x = np.stack([E.edge_inputs(k, bs) for k in range(nb)])                      # [nb, 4, bs]
    if path == "process":
        return np.stack([rt.process(x[k], n_out, bs, sample_time=start + k * bs) for k in range(nb)])
    xin = torch.from_numpy(x).cuda()
    out = torch.zeros((nb, n_out, bs), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    # two calls: block-at-a-time rendering takes up to 8 blocks at a time, so the fade blocks get a call of their own
    rt.process_blocks(first, n_out, out_ptr=out.data_ptr(), in_ptr=xin.data_ptr(), num_inputs=4, sample_time=start)
    rt.process_blocks(NB, n_out, out_ptr=out[first:].data_ptr(), in_ptr=xin[first:].data_ptr(), num_inputs=4, sample_time=start + first * bs)
    got = out.cpu().numpy()
    assert rt.stats()["batch_launches"] >= 2, rt.stats()                          # the last 8 blocks went out in sets of 3
    if path == "spec":
        _assert_ran_specialised(rt)
        assert rt.stats()["spec_launches"] > 0
    else:
        assert rt.stats()["spec_launches"] == 0
    return got


def _needs_ref(name):
    if name in E.EDGE_REF_ONLY:
        import oracle
        if not oracle.have_ref():
            pytest.skip("needs oracle/_ref")


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", sorted(set(E.NODE_EDGE_CASES) - {"clock_far_out"}))
def test_edge_case(gpu_required, name, path):
    _needs_ref(name)
    ref = _reference(name, path, 0)
    got = _render_hip(name, path, 0)
    E.compare_edges(name, got, ref, what=path)


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("which", range(4))
def test_clock_far_out(gpu_required, which, path):
    """time, metro, sparseq2 over time and a train, 8 blocks from sample_time 2^24 - 2 blocks, 2^31 - 2 blocks, 2^32 - 2 blocks and
    2^40 + 3 (the host passes the clock with every call: Runtime.h:274-291)."""
    start = E.clock_starts(PATHS[path][1], _first(path))[which]
    ref = _reference("clock_far_out", path, start)
    got = _render_hip("clock_far_out", path, start)
    E.compare_edges("clock_far_out", got, ref, what=f"{path} from sample_time {start}")
