"""Time the radial-flow path on the device, on the fused kernels (cnf_radial_*)
and, in the same process, on the torch-op path that CNF_RADIAL_NATIVE=0
selects (the code before the kernels existed).  Rows per shape:
  transform   final z (Flow.transform)
  zs          every layer's output (Flow.forward)
  train_step  loss + every gradient: cnf_radial_loss_vjp against torch
              autograd through the torch ops (zero_grad, forward, backward)
  predict     the calibrator's predict as ONE launch (cnf_radial_predict)
              against device torch ops: centring, the layers, both softmaxes
  score       predict ending in the calibration record (cnf_radial_score)
              against those torch ops followed by one cnf_metrics launch
and, at N = 1500 rows (the notebooks' size), full batch:
  fit_epoch   one epoch of TorchFlowCalibrator.fit: a captured HIP graph of
              `reps` epochs replayed, and the same epochs issued eagerly,
              against the torch loop (_fit_torch) on the torch ops
Shapes: (D=3, L=10) and (D=10, L=10) at 2^20 rows, (D=100, L=4) at 2^18.

Method.  The very first native call is followed by a device synchronise before
any loop starts; each side is then warmed by a fixed handful of synchronised
calls (WARM, not a timed loop); each timed window is `reps` calls ended by one
device synchronise, and the two paths alternate window by window.  Every row
records whether the slowest native window beat the fastest torch-op window,
and the run fails at its end if one did not.
One JSON line per (shape, row) is printed and appended to
profiles/radial_bench.jsonl (or --out; `--out -` prints only).  `vs_planar` on
the transform and predict rows is this time over the planar row of the same
shape in profiles/planar_bench.jsonl (reported, no bar).

Counted per row, from the shapes (what the algorithm needs; sqrt and the
division count as one operation each):
  bytes   transform 8 D;  zs 4 D + 4 L D;  train step 4 D + 8;  predict 8 D;
          score 4 D + 8
  flops   forward L (5 D + 5);  train step L (15 D + 17) + 5 D
Roofs: 157.3 TFLOP/s fp32 vector, 8 TB/s HBM (spec).

Usage:  python tools/radial_bench.py [--reps 20] [--windows 5] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "calibration-normalizing-flows_amd"))

from cnf_hip import engine  # noqa: E402
from cnf_hip.metrics import calibration_record  # noqa: E402
from flows import flows as FL  # noqa: E402

VALU_PEAK, HBM_PEAK = 157.3e12, 8.0e12
WARM = 3

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radial_bench.jsonl"))
a = ap.parse_args()
assert torch.cuda.is_available(), "radial_bench needs the GPU"
dev = torch.device("cuda:0")


def window(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def native_counters():
    return sum(v for k, v in engine.stats.items() if k.startswith("radial_"))


def alternate(native, torch_ops, per_call=1):
    """{side: [window times]}: WARM synchronised calls per side, then `windows`
    rounds of one window per side.  `native` maps names to callables that run
    with RADIAL_NATIVE on, `torch_ops` is the one callable that runs with it
    off (fewer reps per window: it is the slow side)."""
    sides = [(k, fn, True) for k, fn in native.items()] + [("torch_ops", torch_ops, False)]
    for _, fn, on in sides:
        FL.RADIAL_NATIVE = on
        for _ in range(WARM):
            fn()
            torch.cuda.synchronize()
    times = {k: [] for k, _, _ in sides}
    for _ in range(a.windows):
        for k, fn, on in sides:
            FL.RADIAL_NATIVE = on
            n0 = native_counters()
            reps = 1 if per_call != 1 else (a.reps if on else max(2, a.reps // 4))
            times[k].append(window(fn, reps) / per_call)
            # (a graph replay counts its launches once, at capture)
            assert on or native_counters() == n0, "%s ran native launches" % k
            assert not on or k == "graph" or native_counters() > n0, "%s ran no native launch" % k
    FL.RADIAL_NATIVE = True
    return times


def finish(row, times, primary):
    for k, v in times.items():
        row[k + "_ms"] = float(np.median(v)) * 1e3
        row[k + "_ms_min"] = float(np.min(v)) * 1e3
        row[k + "_ms_max"] = float(np.max(v)) * 1e3
    row["speedup"] = row["torch_ops_ms"] / row[primary + "_ms"]
    row["native_slowest_beats_torch_fastest"] = all(
        row[k + "_ms_max"] < row["torch_ops_ms_min"] for k in times if k != "torch_ops")
    row["reps"], row["windows"] = a.reps, a.windows
    print(json.dumps(row), flush=True)
    return row


def planar_ms(op, D, L, B):
    """The planar row of the same shape (its last record), or None."""
    path = os.path.join(ROOT, "profiles", "planar_bench.jsonl")
    found = None
    if os.path.exists(path):
        for line in open(path):
            r = json.loads(line)
            if r.get("op") == op and (r.get("D"), r.get("L"), r.get("B")) == (D, L, B):
                found = r.get("native_ms", r.get("fused_ms"))
    return found


def roofs(row, B, bytes_row, flops_row):
    t = row["native_ms"] * 1e-3
    row["rows_per_s"] = B / t
    row["bytes_per_row"], row["flops_per_row"] = bytes_row, flops_row
    row["hbm_roof_fraction"] = B * bytes_row / t / HBM_PEAK
    row["valu_roof_fraction"] = B * flops_row / t / VALU_PEAK


def bench_fit_epoch(D, L, N):
    """One epoch, full batch; a window is `reps` epochs."""
    import calibrators as C
    from cnf_hip.adam import StackAdam
    from flows.normalizing_flows_torch import RadialFlow
    rs = np.random.RandomState(D)
    logits = 2.0 * rs.standard_normal((N, D))
    torch.manual_seed(D)
    cal = C.TorchFlowCalibrator(RadialFlow, logits, np.eye(D)[rs.randint(0, D, size=N)], layers=L,
                                epochs=0, dev=dev)
    cal.flow.to(dev)
    xs, ys = cal.logits.to(dev), cal.target.to(dev)
    stack = C._tensor_stack(cal.flow, dev)
    run = C._EpochRunner(stack, StackAdam.like(stack, cal.optimizer), xs, ys, N)
    terms = torch.empty(a.reps, 3, dtype=torch.float32, device=dev)
    run.eager_epoch(terms[0])
    torch.cuda.synchronize()
    graph = C._EpochGraph(run, a.reps)

    def eager():
        for _ in range(a.reps):
            run.eager_epoch(terms[0])

    times = alternate({"graph": lambda: graph.replay(terms), "eager": eager},
                      lambda: cal._fit_torch(xs, ys, a.reps, N), per_call=a.reps)
    stack.release_workspace()
    assert bool(torch.isfinite(terms).all())
    return finish({"op": "fit_epoch", "D": D, "L": L, "N": N}, times, "graph")


rows = []
first = True
for D, L, B in ((3, 10, 1 << 20), (10, 10, 1 << 20), (100, 4, 1 << 18)):
    torch.manual_seed(D)
    flow = FL.Flow([FL.RadialLayer(D) for _ in range(L)])
    with torch.no_grad():
        for p in flow.parameters():
            p.copy_(torch.randn(p.shape) * 0.5)
        for ly in flow.layers:
            ly.a.copy_(ly.a.abs() + 0.1)
    flow = flow.to(dev)
    x = torch.randn(B, D, device=dev)
    y = torch.randint(0, D, (B,), device=dev)
    lp = torch.log(torch.arange(1, D + 1, device=dev, dtype=torch.float32) / (D * (D + 1) / 2))
    stack = flow._radial_stack()
    if first:  # the very first native call, alone, before any loop
        stack.run(x)
        torch.cuda.synchronize()
        first = False

    def transform():
        with torch.no_grad():
            return flow.transform(x)

    def forward_all():
        with torch.no_grad():
            return flow(x)

    def train_native():
        return stack.loss_and_grads(x, y, grad_scale=1.0 / B)

    def train_torch():
        flow.zero_grad()
        zs, ld = flow(x)
        ce = torch.log(torch.softmax(zs[-1], dim=1).gather(1, y.view(-1, 1)) + 1e-7)
        (-torch.mean(ce.squeeze() + ld)).backward()

    def predict_torch():
        with torch.no_grad():
            z, _ = flow.transform(x - x.mean(dim=1, keepdim=True))
            return torch.softmax(torch.log(torch.softmax(z, dim=1) + 1e-7) - lp, dim=1)

    fwd = L * (5 * D + 5)
    ops = (("transform", transform, transform, 8 * D, fwd),
           ("zs", forward_all, forward_all, 4 * D + 4 * L * D, fwd),
           ("train_step", train_native, train_torch, 4 * D + 8, L * (15 * D + 17) + 5 * D),
           ("predict", lambda: stack.predict(x, lp), predict_torch, 8 * D, fwd + 12 * D),
           ("score", lambda: stack.score(x, lp, y, 15),
            lambda: calibration_record(predict_torch(), y, 15), 4 * D + 8, fwd + 14 * D))
    for name, fn_native, fn_torch, bytes_row, flops_row in ops:
        times = alternate({"native": fn_native}, fn_torch)
        row = {"op": name, "D": D, "L": L, "B": B}
        for k, v in times.items():
            row[k + "_ms"] = float(np.median(v)) * 1e3
        roofs(row, B, bytes_row, flops_row)
        if name in ("transform", "predict"):
            pm = planar_ms(name, D, L, B)
            row["vs_planar"] = None if pm is None else row["native_ms"] / pm
        rows.append(finish(row, times, "native"))
    flow.zero_grad()
    del x, y
for D, L, N in ((3, 10, 1500), (10, 10, 1500)):
    rows.append(bench_fit_epoch(D, L, N))
if a.out != "-":
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
slow = [(r["op"], r["D"]) for r in rows if not r["native_slowest_beats_torch_fastest"]]
assert not slow, "a native window was not faster than every torch-op window: %s" % slow
