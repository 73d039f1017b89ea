"""bench.py's plain run on the GPU: `--steps` timed steps, the headline line
and nothing else, and `--dump-outputs` -- the last timed step's z, log-det and
NLL sums, checked against the numpy oracle (flows/flows.py:17-25) and an fp64
restatement of the calibrator NLL (calibrators.py:289) on the inputs the
arguments determine (not the time-based settle).  One bench process, a small
odd batch (4,099 rows: several blocks, a partial last tile), three rotating
input sets."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from _golden import rel_err
from oracle import cnf_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, STEPS, WARMUP, NSETS = 4099, 4, 1, 3


def test_plain_run_is_lean_and_dumps_the_last_timed_step(tmp_path):
    out_dir = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", str(STEPS), "--warmup", str(WARMUP), "--batch", str(B),
                        "--rotate-gb", "0.001", "--dump-outputs", str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    for key in ("variants", "cpu_baseline", "roofline", "rank_kernel_us", "per_batch_allreduce"):
        assert key not in line, key  # those run only with --full
    assert line["steps"] == STEPS and line["ms_per_step"] > 0
    # value and ms_per_step state the same timed region (both are rounded)
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / B - 1) < 1e-2
    info = line["dump_outputs"]
    assert info["rows"] == info["of"] == B
    # the rotation restarts after the settle: the last timed step's input set
    # follows from --warmup and --steps alone
    assert info["step"] == WARMUP + STEPS - 1 and info["input_set"] == info["step"] % NSETS

    z, ld, sums = (np.load(out_dir / (n + ".npy")) for n in ("z", "log_det", "nll_sums"))
    assert z.dtype == ld.dtype == sums.dtype == np.float32
    assert z.shape == (B, 10) and ld.shape == (B,) and sums.shape == (3,)

    dev = torch.device("cuda:0")
    w = dict(bench.WORKLOADS["cfg2"], B=B)
    x, y = bench.synthetic_logits(B, 10, dev, 1234 + info["input_set"])
    flow = bench.make_flow(w, "cpu")
    st = {k: v.numpy() for k, v in flow.state_dict().items()}
    ol = O.layers_from_state(st, w["L"], 10, len(w["hidden"]) + 1)
    ozs, old = O.flow_forward(ol, x.cpu().numpy())
    assert rel_err(z, ozs[-1]) <= 1e-5
    assert rel_err(ld, old) <= 1e-5
    zd, yd = torch.from_numpy(ozs[-1]).double(), y.cpu()
    lpy = torch.log_softmax(zd, dim=1).gather(1, yd.view(-1, 1)).squeeze(1)
    ce = -torch.log(torch.exp(lpy) + 1e-7)
    ldd = torch.from_numpy(np.asarray(old)).double().reshape(-1)
    ref = np.array([(ce - ldd).sum().item(), ce.sum().item(), ldd.sum().item()])
    # fp32 per-row terms summed over B rows (as tests/_cfg3_worker.py)
    assert (np.abs(sums - ref) <= 1e-5 * (np.abs(ref) + B)).all(), (sums, ref)
