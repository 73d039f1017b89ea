"""Time the fused score launch (cnf_planar_score) next to the two-launch
sequence it replaces (cnf_planar_predict, then cnf_metrics), plus cnf_metrics
alone and cnf_guard_nonfinite on the same probability tensor.

Method: device events around each call on the current stream; per shape a
fixed handful of warm-up launches of every timed call followed by a
synchronise; then `--reps` rounds in which the fused call and the two-launch
sequence ALTERNATE in one process (so clock and cache drift hit both alike),
each round also timing cnf_metrics and the guard.  min / median / max over the
rounds per row.  Parameters live on the device and the record is a reused
buffer, so a timed call is launches only.  One JSON line per shape is APPENDED
to profiles/score_bench.jsonl (or --out).

Without --case this is the driver: each shape runs as a child process under
its own `timeout`, and the driver stops at the first non-zero status.

Usage:  python tools/score_bench.py [--reps 30] [--out PATH] [--case NAME]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "calibration-normalizing-flows_amd"))

# name -> (D, rows, planar layers)
CASES = {
    "planar_d10": (10, 1 << 20, 10),
    "planar_d100": (100, 1 << 18, 4),
}
WARMUP = 5
CHILD_TIMEOUT_S = 120


def build(D, L, dev):
    """(score(x, y, record), predict(x), the flow that owns the parameters)
    of a seeded planar stack on the device."""
    import numpy as np
    import torch
    from flows.flows import Flow, PlanarLayer
    rs = np.random.RandomState(100 + D)
    lp64 = np.log(np.arange(1, D + 1) / (D * (D + 1) / 2.0))
    flow = Flow([PlanarLayer(D) for _ in range(L)])
    with torch.no_grad():
        for ly in flow.layers:
            ly.w.copy_(torch.from_numpy((rs.standard_normal(D) * 0.5).astype(np.float32)))
            ly.u.copy_(torch.from_numpy((rs.standard_normal(D) * 0.5).astype(np.float32)))
            ly.b.copy_(torch.from_numpy((rs.standard_normal(1) * 0.5).astype(np.float32)))
    flow = flow.to(dev)
    stack = flow._planar_stack()
    lp = torch.as_tensor(lp64, dtype=torch.float32, device=dev)
    return (lambda x, y, rec: stack.score(x, lp, y, 15, rec)), \
        (lambda x: stack.predict(x, lp)), flow


def run_case(name, reps, out):
    import numpy as np
    import torch
    from cnf_hip.guard import NonFiniteGuard
    from cnf_hip.metrics import calibration_record
    D, B, L = CASES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(D)
    x = (1.5 * torch.randn(B, D, generator=g)).to(dev)
    y = torch.randint(0, D, (B,), generator=g).to(dev)
    def stage(what):   # unbuffered: a stalled child shows where it stopped
        print("score_bench %s: %s" % (name, what), file=sys.stderr, flush=True)
    stage("inputs on the device")
    score, predict, keep = build(D, L, dev)
    rec = torch.zeros(4 + 3 * 15, dtype=torch.int64, device=dev)
    guard = NonFiniteGuard(dev)
    probs = predict(x)

    calls = {
        "fused": lambda: score(x, y, rec),
        "two_launch": lambda: calibration_record(predict(x), y, 15, rec),
        "predict": lambda: predict(x),
        "metrics": lambda: calibration_record(probs, y, 15, rec),
        "guard": lambda: guard.check(probs),
    }
    # the fused record is the two-launch record, or the timing means nothing
    a = score(x, y, torch.zeros_like(rec))
    b = calibration_record(predict(x), y, 15, torch.zeros_like(rec))
    assert torch.equal(a, b), (a.tolist(), b.tolist())
    stage("fused record equals the two-launch record")
    for _ in range(WARMUP):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize(dev)
    stage("warmed up")
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():      # fused and two_launch alternate
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    row = {"case": name, "D": D, "B": B, "layers": L, "bins": 15, "reps": reps, "warmup": WARMUP}
    for k, ts in times.items():
        row[k + "_ms"] = {"min": float(np.min(ts)), "median": float(np.median(ts)),
                          "max": float(np.max(ts))}
    row["fused_over_two_launch_median"] = row["fused_ms"]["median"] / row["two_launch_ms"]["median"]
    row["metrics_GBps_median"] = B * (4 * D + 8) / (row["metrics_ms"]["median"] * 1e-3) / 1e9
    row["guard_GBps_median"] = B * 4 * D / (row["guard_ms"]["median"] * 1e-3) / 1e9
    print(json.dumps(row))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.jsonl"))
    ap.add_argument("--case", choices=sorted(CASES))
    a = ap.parse_args()
    if a.case:
        run_case(a.case, a.reps, a.out)
        return 0
    for name in CASES:
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable,
               os.path.abspath(__file__), "--case", name, "--reps", str(a.reps), "--out", a.out]
        rc = subprocess.call(cmd)
        if rc != 0:
            print("score_bench: %s ended with status %d; stopping" % (name, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
