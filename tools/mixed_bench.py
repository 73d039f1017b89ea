"""Time a mixed planar / radial / affine flow on the device, on the fused stack
(cnf_mixed_*) and, in the same process, on the path CNF_MIXED_NATIVE=0
selects: the layer loop, each layer one launch of its own family (the code
before the fused stack existed).  Rows per shape:
  transform   final z (Flow.transform)
  zs          every layer's output (Flow.forward)
  train_step  loss + every gradient: cnf_mixed_loss_vjp against torch autograd
              through the layer loop (zero_grad, forward, backward: one forward
              and one reverse launch per layer)
  predict     the calibrator's predict as ONE launch (cnf_mixed_predict)
              against device torch ops around the layer loop
  score       predict ending in the calibration record (cnf_mixed_score)
              against those ops followed by one cnf_metrics launch
and, at N = 1500 rows (the notebooks' size), full batch:
  fit_epoch   one epoch of TorchFlowCalibrator.fit: a captured HIP graph of
              `reps` epochs replayed, and the same epochs issued eagerly,
              against the torch loop (_fit_torch) over the layer loop
Shapes: PRPRPRPRPA at D = 10, 2^20 rows; PRAP at D = 100, 2^18 rows; fit_epoch
PRPRA at D = 3.

Method (tools/affine_bench.py's).  The very first native call is followed by a
device synchronise before any loop starts; each side is then warmed by a fixed
handful of synchronised calls (WARM, not a timed loop); each timed window is
`reps` calls ended by one device synchronise, and the sides alternate window
by window.  Every row records whether the slowest fused window beat the
fastest layer-loop window; nothing is asserted on it.

Context.  The transform, train_step, predict and score rows also time a
PlanarStack and a RadialStack of the same (D, L, B) in windows that alternate
with the other sides -- same process, same build -- and report vs_planar and
vs_radial = mixed / that family (medians): the cost of the mixed reverse mode,
which recomputes what the single families tape, relative to them.

One JSON line per (shape, row) is printed and appended to
profiles/mixed_bench.jsonl (or --out; `--out -` prints only).  `--only OP:D`
(repeatable) runs just those rows, so a driver can give each row its own time
limit and stop at the first that fails.

Counted per row, from the shapes (what the algorithm needs):
  bytes   transform 8 D;  zs 4 D + 4 L D;  train step 4 D + 8;  predict 8 D;
          score 4 D + 8
Roof: 8 TB/s HBM (spec).

Usage:  python tools/mixed_bench.py [--reps 10] [--windows 30] [--out PATH] [--only OP:D ...]
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

HBM_PEAK = 8.0e12
WARM = 3
LAYER = {"P": FL.PlanarLayer, "R": FL.RadialLayer, "A": FL.AffineConstantLayer}

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--windows", type=int, default=30)
ap.add_argument("--only", action="append", default=[], help="OP:D, e.g. transform:10")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_bench.jsonl"))
a = ap.parse_args()
assert torch.cuda.is_available(), "mixed_bench needs the GPU"
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


def mixed_counters():
    return sum(v for k, v in engine.stats.items() if k.startswith("mixed_"))


def alternate(native, today, per_call=1):
    """{side: [window times]}: WARM synchronised calls per side, then `windows`
    rounds of one window per side.  `native` maps names to callables that run
    with MIXED_NATIVE on ("planar", "radial": the single families, no mixed
    launch), `today` is the one callable that runs with it off (fewer reps per
    window: it is the slow side)."""
    sides = [(k, fn, True) for k, fn in native.items()] + [("today", today, False)]
    for _, fn, on in sides:
        FL.MIXED_NATIVE = on
        for _ in range(WARM):
            fn()
            torch.cuda.synchronize()
    times = {k: [] for k, _, _ in sides}
    for _ in range(a.windows):
        for k, fn, on in sides:
            FL.MIXED_NATIVE = on
            n0 = mixed_counters()
            reps = 1 if per_call != 1 else (a.reps if on else max(2, a.reps // 4))
            times[k].append(window(fn, reps) / per_call)
            # (a graph replay counts its launches once, at capture)
            ran = mixed_counters() > n0
            assert not (ran and (not on or k in ("planar", "radial"))), "%s ran mixed launches" % k
            assert ran or not on or k in ("graph", "planar", "radial"), "%s ran no mixed launch" % k
    FL.MIXED_NATIVE = True
    return times


def finish(row, times, primary):
    for k, v in times.items():
        row[k + "_ms"] = float(np.median(v)) * 1e3
        row[k + "_ms_min"] = float(np.min(v)) * 1e3
        row[k + "_ms_max"] = float(np.max(v)) * 1e3
    row["speedup"] = row["today_ms"] / row[primary + "_ms"]
    row["fused_slowest_beats_today_fastest"] = all(
        row[k + "_ms_max"] < row["today_ms_min"] for k in times
        if k not in ("today", "planar", "radial"))
    for fam in ("planar", "radial"):
        if fam in times:
            row["vs_" + fam] = row["native_ms"] / row[fam + "_ms"]
    row["reps"], row["windows"] = a.reps, a.windows
    print(json.dumps(row), flush=True)
    return row


def draw(order, D):
    """Damped as the tests' sweeps draw them (tests/_mixed_ref.draw_params)."""
    L = len(order)
    flow = FL.Flow([LAYER[c](D) for c in order])
    sc = min(0.5, 1.0 / np.sqrt(D))
    with torch.no_grad():
        for c, ly in zip(order, flow.layers):
            if c == "P":
                ly.w.copy_(torch.randn(D) * sc)
                ly.u.copy_(torch.randn(D) * sc)
                ly.b.copy_(torch.randn(1) * 0.5)
            elif c == "R":
                ly.z0.copy_(torch.randn(D) * 0.5)
                ly.a.copy_((1.0 + 0.5 * torch.randn(1)).abs())
                ly.b.copy_(torch.randn(1) * 0.5)
            else:
                ly.s.copy_(torch.randn(1, D) * min(0.3, 1.0 / L))
                ly.t.copy_(torch.randn(1, D) * min(0.5, 2.0 / L))
    return flow


def bench_fit_epoch(order, D, N):
    """One epoch, full batch; a window is `reps` epochs."""
    import calibrators as C
    from cnf_hip.adam import StackAdam
    from flows.normalizing_flows_torch import MixedFlow
    rs = np.random.RandomState(D)
    logits = 2.0 * rs.standard_normal((N, D))
    torch.manual_seed(D)
    cal = C.TorchFlowCalibrator(MixedFlow, logits, np.eye(D)[rs.randint(0, D, size=N)],
                                layers=order, epochs=0, dev=dev)
    cal.flow.to(dev)
    xs, ys = cal.logits.to(dev), cal.target.to(dev)
    stack = C._tensor_stack(cal.flow, dev)
    assert stack is not None and stack.family == "mixed"
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
    return finish({"op": "fit_epoch", "order": order, "D": D, "L": len(order), "N": N}, times,
                  "graph")


OPS = ("transform", "zs", "train_step", "predict", "score")
rows = []
first = True
for order, D, B in (("PRPRPRPRPA", 10, 1 << 20), ("PRAP", 100, 1 << 18)):
    if not any(wanted(op, D) for op in OPS):
        continue
    L = len(order)
    torch.manual_seed(D)
    flow = draw(order, D).to(dev)
    pflow = draw("P" * L, D).to(dev)
    rflow = draw("R" * L, D).to(dev)
    x = torch.randn(B, D, device=dev)
    y = torch.randint(0, D, (B,), device=dev)
    lp = torch.log(torch.arange(1, D + 1, device=dev, dtype=torch.float32) / (D * (D + 1) / 2))
    cls = FL._row_class(list(flow.layers), x)
    assert cls is not None and cls.family == "mixed"
    stack = flow._row_stack(cls, list(flow.layers))
    pstack, rstack = pflow._planar_stack(), rflow._radial_stack()
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

    def train_today():
        flow.zero_grad()
        zs, ld = flow(x)
        ce = torch.log(torch.softmax(zs[-1], dim=1).gather(1, y.view(-1, 1)) + 1e-7)
        (-torch.mean(ce.squeeze() + ld)).backward()

    def predict_today():
        with torch.no_grad():
            z, _ = flow.transform(x - x.mean(dim=1, keepdim=True))
            return torch.softmax(torch.log(torch.softmax(z, dim=1) + 1e-7) - lp, dim=1)

    def single(st, what):
        if what == "transform":
            return lambda: st.run(x)
        if what == "train_step":
            return lambda: st.loss_and_grads(x, y, grad_scale=1.0 / B)
        if what == "predict":
            return lambda: st.predict(x, lp)
        return lambda: st.score(x, lp, y, 15)

    ops = (("transform", transform, transform, True, 8 * D),
           ("zs", forward_all, forward_all, False, 4 * D + 4 * L * D),
           ("train_step", train_native, train_today, True, 4 * D + 8),
           ("predict", lambda: stack.predict(x, lp), predict_today, True, 8 * D),
           ("score", lambda: stack.score(x, lp, y, 15),
            lambda: calibration_record(predict_today(), y, 15), True, 4 * D + 8))
    for name, fn_native, fn_today, context, bytes_row in ops:
        if not wanted(name, D):
            continue
        native = {"native": fn_native}
        if context:
            native["planar"], native["radial"] = single(pstack, name), single(rstack, name)
        times = alternate(native, fn_today)
        row = {"op": name, "order": order, "D": D, "L": L, "B": B}
        t = float(np.median(times["native"]))
        row["rows_per_s"] = B / t
        row["bytes_per_row"] = bytes_row
        row["hbm_roof_fraction"] = B * bytes_row / t / HBM_PEAK
        rows.append(finish(row, times, "native"))
    flow.zero_grad()
    del x, y
if wanted("fit_epoch", 3):
    rows.append(bench_fit_epoch("PRPRA", 3, 1500))
if a.out != "-":
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
