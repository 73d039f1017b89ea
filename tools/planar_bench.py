"""Time the planar-flow path on the device: `transform` (final z + log-det), the
full `zs` forward (every layer's output) and the training step (loss + every
gradient), on the fused kernels (cnf_planar_*) and, in the same process, on the
torch-op path that CNF_PLANAR_NATIVE=0 selects (the code before the kernels
existed).  Shapes: (D=3, L=10) and (D=10, L=10) at 2^20 rows, (D=100, L=4) at
2^18.  Untimed calls settle the clock first; each timed window is `reps` calls
ended by one device synchronise, and the two paths alternate window by window.
One JSON line per (shape, operation) is printed and goes to
profiles/planar_bench.jsonl (or --out; `--out -` prints only).

Counted per row, from the shapes (what the algorithm needs, not what the
compiler emits; tanh and log count as one operation each):
  bytes   transform 8 D + 4;  zs forward 4 D + 4 L D + 4;  train step 4 D + 8
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
if a.out != "-":
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
