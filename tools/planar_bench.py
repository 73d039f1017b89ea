"""Time the planar-flow path on the device: `transform` (final z + log-det), the
full `zs` forward (every layer's output) and the training step (loss + every
gradient), on the fused kernels (cnf_planar_*) and, in the same process, on the
torch-op path that CNF_PLANAR_NATIVE=0 selects (the code before the kernels
existed).  Shapes: (D=3, L=10) and (D=10, L=10) at 2^20 rows, (D=100, L=4) at
2^18.  Untimed calls settle the clock first; each timed window is `reps` calls
ended by one device synchronise, and the two paths alternate window by window.
One JSON line per (shape, operation) is printed and appended to
profiles/planar_bench.jsonl (or --out; `--out -` prints only).

Two more rows per shape:
  predict    the calibrator's predict as ONE launch (cnf_planar_predict) against
             the composition it fuses: device torch ops for the centring,
             cnf_planar_forward, and torch's two softmaxes, log and subtraction
  fit_epoch  one epoch of TorchFlowCalibrator.fit (full batch, N = 1500 rows,
             the notebook's size; D = 3 and D = 10, L = 10) three ways: a
             captured HIP graph of `reps` epochs replayed, the same epochs
             issued eagerly (cnf_planar_loss_vjp + one native Adam launch +
             cnf_planar_forward_loss), and the loop before the native Adam
             (cnf_planar_loss_vjp, torch.optim.Adam.step, cnf_planar_forward_loss)

Counted per row, from the shapes (what the algorithm needs, not what the
compiler emits; tanh and log count as one operation each):
  bytes   transform 8 D + 4;  zs forward 4 D + 4 L D + 4;  train step 4 D + 8
          predict 8 D (fused);  24 D + 4 for the composition's six passes
          (centre 8 D, forward 8 D + 4, softmax 8 D; log, subtract and the
          second softmax fuse at best into the same 8 D each: counted 0)
  flops   forward L (4 D + 10);  train step L (15 D + 30) + 5 D
Roofs: 157.3 TFLOP/s fp32 vector, 8 TB/s HBM (spec).

Usage:  python tools/planar_bench.py [--reps 20] [--windows 5] [--settle-s 0.3] [--out PATH]
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
from flows import flows as FL  # noqa: E402

VALU_PEAK, HBM_PEAK = 157.3e12, 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--settle-s", type=float, default=0.3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planar_bench.jsonl"))
a = ap.parse_args()
assert torch.cuda.is_available(), "planar_bench needs the GPU"
dev = torch.device("cuda:0")


def window(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def median_row(times):
    return {k + "_ms": float(np.median(v)) * 1e3 for k, v in times.items()} | \
        {k + "_ms_min": float(np.min(v)) * 1e3 for k, v in times.items()} | \
        {k + "_ms_max": float(np.max(v)) * 1e3 for k, v in times.items()}


def alternate(sides, per_call=1):
    """Settle every side, then `windows` rounds of one window per side."""
    for fn in sides.values():
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < a.settle_s:
            fn()
            torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(a.windows):
        for k, fn in sides.items():
            times[k].append(window(fn, a.reps if per_call == 1 else 1) / per_call)
    return times


def bench_predict(stack, x, D, L, B):
    lp = torch.log(torch.arange(1, D + 1, device=dev, dtype=torch.float32) / (D * (D + 1) / 2))

    def fused():
        return stack.predict(x, lp)

    def composed():
        xc = x - x.mean(dim=1, keepdim=True)
        z, _, _ = stack.run(xc)
        return torch.softmax(torch.log(torch.softmax(z, dim=1) + 1e-7) - lp, dim=1)

    n0 = engine.stats["planar_predict"]
    times = alternate({"fused": fused, "composed": composed})
    assert engine.stats["planar_predict"] >= n0 + a.windows * a.reps, "no fused predict ran"
    row = {"op": "predict", "D": D, "L": L, "B": B, **median_row(times)}
    row["speedup"] = row["composed_ms"] / row["fused_ms"]
    row["rows_per_s"] = B / (row["fused_ms"] * 1e-3)
    row["bytes_per_row"] = 8 * D
    row["hbm_roof_fraction"] = B * 8 * D / (row["fused_ms"] * 1e-3) / HBM_PEAK
    row["reps"], row["windows"] = a.reps, a.windows
    return row


def bench_fit_epoch(D, L, N):
    """One epoch, full batch, three ways; a window is `reps` epochs."""
    import calibrators as C
    from cnf_hip.adam import StackAdam
    from flows._factory import PlanarFlow
    rs = np.random.RandomState(D)
    logits = 2.0 * rs.standard_normal((N, D))
    torch.manual_seed(D)
    cal = C.TorchFlowCalibrator(PlanarFlow, logits, np.eye(D)[rs.randint(0, D, size=N)], layers=L,
                                epochs=0, dev=dev)
    cal.flow.to(dev)
    xs, ys = cal.logits.to(dev), cal.target.to(dev)
    stack = C._tensor_stack(cal.flow, dev)
    run = C._EpochRunner(stack, StackAdam.like(stack, cal.optimizer), xs, ys, N)
    terms = torch.empty(a.reps, 3, dtype=torch.float32, device=dev)
    run.eager_epoch(terms[0])
    graph = C._EpochGraph(run, a.reps)

    def eager():
        for _ in range(a.reps):
            run.eager_epoch(terms[0])

    times = alternate({"graph": lambda: graph.replay(terms), "eager": eager,
                       "parent_loop": lambda: cal._fit_torch_step(stack, xs, ys, a.reps, N)},
                      per_call=a.reps)
    stack.release_workspace()
    assert bool(torch.isfinite(terms).all())
    row = {"op": "fit_epoch", "D": D, "L": L, "N": N, **median_row(times)}
    row["graph_vs_parent"] = row["parent_loop_ms"] / row["graph_ms"]
    row["eager_vs_parent"] = row["parent_loop_ms"] / row["eager_ms"]
    row["reps"], row["windows"] = a.reps, a.windows
    return row


rows = []
for D, L, B in ((3, 10, 1 << 20), (10, 10, 1 << 20), (100, 4, 1 << 18)):
    torch.manual_seed(D)
    flow = FL.Flow([FL.PlanarLayer(D) for _ in range(L)])
    with torch.no_grad():
        for p in flow.parameters():
            p.copy_(torch.randn(p.shape) * 0.5)
    flow = flow.to(dev)
    x = torch.randn(B, D, device=dev)
    y = torch.randint(0, D, (B,), device=dev)
    stack = flow._planar_stack()

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

    ops = {"transform": (transform, transform, 8 * D + 4, L * (4 * D + 10)),
           "forward_zs": (forward_all, forward_all, 4 * D + 4 * L * D + 4, L * (4 * D + 10)),
           "train_step": (train_native, train_torch, 4 * D + 8, L * (15 * D + 30) + 5 * D)}
    for name, (fn_native, fn_torch, bytes_row, flops_row) in ops.items():
        times = {True: [], False: []}
        for native in (True, False):  # warm both paths up, settle the clock
            FL.PLANAR_NATIVE = native
            fn = fn_native if native else fn_torch
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < a.settle_s:
                fn()
                torch.cuda.synchronize()
        n0 = engine.stats["planar_forward"] + engine.stats["planar_loss_vjp"]
        for _ in range(a.windows):
            for native in (True, False):
                FL.PLANAR_NATIVE = native
                times[native].append(window(fn_native if native else fn_torch,
                                            a.reps if native else max(2, a.reps // 4)))
        FL.PLANAR_NATIVE = True
        assert engine.stats["planar_forward"] + engine.stats["planar_loss_vjp"] \
            == n0 + a.windows * a.reps, "the native path did not run"
        tn, tt = float(np.median(times[True])), float(np.median(times[False]))
        row = {"op": name, "D": D, "L": L, "B": B, "native_ms": tn * 1e3,
               "native_ms_min": float(np.min(times[True])) * 1e3,
               "native_ms_max": float(np.max(times[True])) * 1e3,
               "torch_ops_ms": tt * 1e3, "speedup": tt / tn, "rows_per_s": B / tn,
               "torch_ops_rows_per_s": B / tt, "bytes_per_row": bytes_row,
               "flops_per_row": flops_row, "hbm_roof_fraction": B * bytes_row / tn / HBM_PEAK,
               "valu_roof_fraction": B * flops_row / tn / VALU_PEAK,
               "reps": a.reps, "windows": a.windows}
        rows.append(row)
        print(json.dumps(row), flush=True)
    rows.append(bench_predict(stack, x, D, L, B))
    print(json.dumps(rows[-1]), flush=True)
    del x, y
for D, L, N in ((3, 10, 1500), (10, 10, 1500)):
    rows.append(bench_fit_epoch(D, L, N))
    print(json.dumps(rows[-1]), flush=True)
if a.out != "-":
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
