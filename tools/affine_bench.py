"""Time the affine-constant path on the device, on the fused kernels
(cnf_affine_*) and, in the same process, on the torch-op path that
CNF_AFFINE_NATIVE=0 selects (the code before the kernels existed).  Rows per
shape:
  transform   final z (Flow.transform)
  zs          every layer's output (Flow.forward)
  inverse     final x (Flow.inverse_transform)
  train_step  loss + every gradient: cnf_affine_loss_vjp against torch
              autograd through the torch ops (zero_grad, forward, backward)
  predict     the calibrator's predict as ONE launch (cnf_affine_predict)
              against device torch ops: centring, the layers, both softmaxes
  score       predict ending in the calibration record (cnf_affine_score)
              against those torch ops followed by one cnf_metrics launch
and, at N = 1500 rows (the notebooks' size), full batch:
  fit_epoch   one epoch of TorchFlowCalibrator.fit: a captured HIP graph of
              `reps` epochs replayed, and the same epochs issued eagerly,
              against the torch loop (_fit_torch) on the torch ops
Shapes: (D=3, L=5) and (D=10, L=5) at 2^20 rows, (D=100, L=4) at 2^18.

Method (tools/radial_bench.py's).  The very first native call is followed by a
device synchronise before any loop starts; each side is then warmed by a fixed
handful of synchronised calls (WARM, not a timed loop); each timed window is
`reps` calls ended by one device synchronise, and the sides alternate window
by window.  Every row records whether the slowest native window beat the
fastest torch-op window, and the run fails at its end if one did not.

Against the radial family.  The transform, train_step, predict and score rows
also time a RadialStack of the same (D, L, B) in windows that alternate with
the other two sides -- same process, same build -- and report
`vs_radial` = affine / radial (medians) and `radial_spread`, the radial side's
(max - min) / median over its windows.  An affine layer does less arithmetic
than a radial one over the same bytes, so vs_radial above 1 + spread wants a
look.

One JSON line per (shape, row) is printed and appended to
profiles/affine_bench.jsonl (or --out; `--out -` prints only).  `--only
OP:D` (repeatable) runs just those rows, so a driver can give each row its own
time limit.

Counted per row, from the shapes (what the algorithm needs):
  bytes   transform, inverse 8 D;  zs 4 D + 4 L D;  train step 4 D + 8;
          predict 8 D;  score 4 D + 8
  flops   forward / inverse 2 L D;  train step 6 L D + 5 D;  predict + 12 D;
          score + 14 D
Roofs: 157.3 TFLOP/s fp32 vector, 8 TB/s HBM (spec).

Usage:  python tools/affine_bench.py [--reps 20] [--windows 5] [--out PATH] [--only OP:D ...]
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
ap.add_argument("--only", action="append", default=[], help="OP:D, e.g. transform:3")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affine_bench.jsonl"))
a = ap.parse_args()
assert torch.cuda.is_available(), "affine_bench needs the GPU"
dev = torch.device("cuda:0")


def wanted(op, D):
    return not a.only or ("%s:%d" % (op, D)) in a.only


def window(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def native_counters():
    return sum(v for k, v in engine.stats.items() if k.startswith("affine_"))


def alternate(native, torch_ops, per_call=1):
    """{side: [window times]}: WARM synchronised calls per side, then `windows`
    rounds of one window per side.  `native` maps names to callables that run
    with AFFINE_NATIVE on ("radial": the sibling family, no affine launch),
    `torch_ops` is the one callable that runs with it off (fewer reps per
    window: it is the slow side)."""
    sides = [(k, fn, True) for k, fn in native.items()] + [("torch_ops", torch_ops, False)]
    for _, fn, on in sides:
        FL.AFFINE_NATIVE = on
        for _ in range(WARM):
            fn()
            torch.cuda.synchronize()
    times = {k: [] for k, _, _ in sides}
    for _ in range(a.windows):
        for k, fn, on in sides:
            FL.AFFINE_NATIVE = on
            n0 = native_counters()
            reps = 1 if per_call != 1 else (a.reps if on else max(2, a.reps // 4))
            times[k].append(window(fn, reps) / per_call)
            # (a graph replay counts its launches once, at capture)
            ran = native_counters() > n0
            assert not (ran and (not on or k == "radial")), "%s ran affine launches" % k
            assert ran or not on or k in ("graph", "radial"), "%s ran no native launch" % k
    FL.AFFINE_NATIVE = True
    return times


def finish(row, times, primary):
    for k, v in times.items():
        row[k + "_ms"] = float(np.median(v)) * 1e3
        row[k + "_ms_min"] = float(np.min(v)) * 1e3
        row[k + "_ms_max"] = float(np.max(v)) * 1e3
    row["speedup"] = row["torch_ops_ms"] / row[primary + "_ms"]
    row["native_slowest_beats_torch_fastest"] = all(
        row[k + "_ms_max"] < row["torch_ops_ms_min"] for k in times
        if k not in ("torch_ops", "radial"))
    if "radial" in times:
        row["vs_radial"] = row["native_ms"] / row["radial_ms"]
        row["radial_spread"] = (row["radial_ms_max"] - row["radial_ms_min"]) / row["radial_ms"]
        row["native_spread"] = (row["native_ms_max"] - row["native_ms_min"]) / row["native_ms"]
    row["reps"], row["windows"] = a.reps, a.windows
    print(json.dumps(row), flush=True)
    return row


def roofs(row, B, bytes_row, flops_row):
    t = row["native_ms"] * 1e-3
    row["rows_per_s"] = B / t
    row["bytes_per_row"], row["flops_per_row"] = bytes_row, flops_row
    row["hbm_roof_fraction"] = B * bytes_row / t / HBM_PEAK
    row["valu_roof_fraction"] = B * flops_row / t / VALU_PEAK


def draw_affine(D, L):
    flow = FL.Flow([FL.AffineConstantLayer(D) for _ in range(L)])
    with torch.no_grad():
        for ly in flow.layers:
            ly.s.copy_(torch.randn(1, D) * min(0.3, 1.0 / L))
            ly.t.copy_(torch.randn(1, D) * min(0.5, 2.0 / L))
    return flow


def bench_fit_epoch(D, L, N):
    """One epoch, full batch; a window is `reps` epochs."""
    import calibrators as C
    from cnf_hip.adam import StackAdam
    from flows.normalizing_flows_torch import AffineConstantFlow
    rs = np.random.RandomState(D)
    logits = 2.0 * rs.standard_normal((N, D))
    torch.manual_seed(D)
    cal = C.TorchFlowCalibrator(AffineConstantFlow, logits, np.eye(D)[rs.randint(0, D, size=N)],
                                layers=L, epochs=0, dev=dev)
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


OPS = ("transform", "zs", "inverse", "train_step", "predict", "score")
rows = []
first = True
for D, L, B in ((3, 5, 1 << 20), (10, 5, 1 << 20), (100, 4, 1 << 18)):
    if not any(wanted(op, D) for op in OPS):
        continue
    torch.manual_seed(D)
    flow = draw_affine(D, L).to(dev)
    rflow = FL.Flow([FL.RadialLayer(D) for _ in range(L)])
    with torch.no_grad():
        for p in rflow.parameters():
            p.copy_(torch.randn(p.shape) * 0.5)
        for ly in rflow.layers:
            ly.a.copy_(ly.a.abs() + 0.1)
    rflow = rflow.to(dev)
    x = torch.randn(B, D, device=dev)
    y = torch.randint(0, D, (B,), device=dev)
    lp = torch.log(torch.arange(1, D + 1, device=dev, dtype=torch.float32) / (D * (D + 1) / 2))
    stack = flow._row_stack(FL._row_class(list(flow.layers), x), list(flow.layers))
    rstack = rflow._radial_stack()
    if first:  # the very first native call, alone, before any loop
        stack.run(x)
        torch.cuda.synchronize()
        first = False
    with torch.no_grad():
        zfin = flow.transform(x)[0]

    def transform():
        with torch.no_grad():
            return flow.transform(x)

    def forward_all():
        with torch.no_grad():
            return flow(x)

    def inverse():
        with torch.no_grad():
            return flow.inverse_transform(zfin)

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

    def radial_transform():
        with torch.no_grad():
            return rflow.transform(x)

    fwd = 2 * L * D
    ops = (("transform", transform, transform, radial_transform, 8 * D, fwd),
           ("zs", forward_all, forward_all, None, 4 * D + 4 * L * D, fwd),
           ("inverse", inverse, inverse, None, 8 * D, fwd),
           ("train_step", train_native, train_torch,
            lambda: rstack.loss_and_grads(x, y, grad_scale=1.0 / B), 4 * D + 8, 6 * L * D + 5 * D),
           ("predict", lambda: stack.predict(x, lp), predict_torch,
            lambda: rstack.predict(x, lp), 8 * D, fwd + 12 * D),
           ("score", lambda: stack.score(x, lp, y, 15),
            lambda: calibration_record(predict_torch(), y, 15),
            lambda: rstack.score(x, lp, y, 15), 4 * D + 8, fwd + 14 * D))
    for name, fn_native, fn_torch, fn_radial, bytes_row, flops_row in ops:
        if not wanted(name, D):
            continue
        native = {"native": fn_native}
        if fn_radial is not None:
            native["radial"] = fn_radial
        times = alternate(native, fn_torch)
        row = {"op": name, "D": D, "L": L, "B": B}
        for k, v in times.items():
            row[k + "_ms"] = float(np.median(v)) * 1e3
        roofs(row, B, bytes_row, flops_row)
        rows.append(finish(row, times, "native"))
    flow.zero_grad()
    del x, y, zfin
for D, L, N in ((3, 5, 1500), (10, 5, 1500)):
    if wanted("fit_epoch", D):
        rows.append(bench_fit_epoch(D, L, N))
if a.out != "-":
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
slow = [(r["op"], r["D"]) for r in rows if not r["native_slowest_beats_torch_fastest"]]
assert not slow, "a native window was not faster than every torch-op window: %s" % slow
