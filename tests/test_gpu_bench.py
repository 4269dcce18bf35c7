"""bench.py's plain run (`--gpus 1 --steps K --warmup W`): the result line's contract fields, `--steps` as the number of timed
steps, nothing beyond the headline, and `--dump-outputs` — what the timed path handed its caller in the LAST timed step —
against the CPU checker advanced through the whole run (warm-up and timed steps)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from elementary_amd import graphs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 512


def _bench(args, tmp_path):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dump-outputs", str(tmp_path)] + args,
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 2 and json.loads(lines[0]).get("record") == "headline_full", res.stdout[-2000:]
    rec = json.loads(lines[-1])
    assert rec["unit"] == "samples/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32" and rec["ms_per_step"] > 0
    for k in ("configs", "cpu_baseline", "parity", "device_resident"):        # the legs behind --full
        assert k not in rec, k
    return rec


def _checker(sr):
    return oracle.RefRuntime(sr, BLOCK) if oracle.have_ref() else oracle.PortRuntime(sr, BLOCK)


@pytest.mark.parametrize("mode", ["host", "device_resident"])
def test_plain_c2_run_dumps_its_last_timed_step(gpu_required, tmp_path, mode):
    """host: the planar host arrays [2, frames] the timed call filled; device_resident: the last step's bus chunk [blocks, 2, frames]
    as copied to pinned host memory."""
    steps, warmup, B, voices = 3, 1, 16, 8
    extra = ["--device-resident"] if mode == "device_resident" else []
    rec = _bench(["--steps", str(steps), "--warmup", str(warmup), "--batch-blocks", str(B), "--voices", str(voices)] + extra, tmp_path)
    assert rec["steps"] == steps and rec["warmup"] == warmup
    assert abs(rec["value"] * rec["ms_per_step"] * 1e-3 / (B * BLOCK) - 1) < 1e-4      # value = frames of one step / ms_per_step
    got = np.load(tmp_path / "c2_bus_last_step.npy")
    chk = _checker(graphs.C2_SAMPLE_RATE)
    assert chk.render(*graphs.c2_graph(voices=voices, channels=2))["result"] == 0
    for _ in range((warmup + steps - 1) * B):
        chk.process(None, 2, BLOCK)
    ref = np.stack([chk.process(None, 2, BLOCK) for _ in range(B)])                 # [blocks, 2, frames]
    if mode == "host":
        ref = np.concatenate(list(ref), axis=1)                                     # [2, frames]
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert float(np.abs(got - ref).max()) <= 1e-6 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("mode", ["device_resident", "host_delivered"])
def test_plain_c4_run_dumps_its_last_timed_step(gpu_required, tmp_path, mode):
    """device_resident: [blocks, job, frames] from the device buffer; host_delivered: the caller's planar arrays [job, frames]."""
    steps, warmup, B, inst = 2, 1, 16, 6
    extra = ["--host-delivered"] if mode == "host_delivered" else []
    rec = _bench(["--workload", "c4", "--instances", str(inst), "--steps", str(steps), "--warmup", str(warmup), "--batch-blocks", str(B)]
                 + extra, tmp_path)
    assert rec["steps"] == steps and rec["warmup"] == warmup
    got = np.load(tmp_path / "c4_jobs_last_step.npy")
    chk = _checker(graphs.C4_SAMPLE_RATE)
    assert chk.render(*[graphs.c4_instance(k) for k in range(inst)])["result"] == 0
    for _ in range((warmup + steps - 1) * B):
        chk.process(None, inst, BLOCK)
    ref = np.stack([chk.process(None, inst, BLOCK) for _ in range(B)])             # [blocks, job, frames]
    if mode == "host_delivered":
        ref = ref.transpose(1, 0, 2).reshape(inst, B * BLOCK)                       # [job, frames]
    assert got.dtype == np.float32 and got.shape == ref.shape                      # fewer jobs than the sample: every job, in order
    assert float(np.abs(got - ref).max()) <= 1e-6 * max(1.0, float(np.abs(ref).max()))
