"""Generate the affine-constant fixtures (tests/golden/affine/*.npz) FROM THE
REFERENCE ITSELF: its Flow([AffineConstantLayer(dim) ...]) (flows/flows.py:8-37,
40-65), forward and backward, and its Calibrator.predict around that flow
(calibrators.py:40-44, 330-353) on seeded inputs, in fp32 and with the same
module converted to float64.

Test infrastructure only; runs on the CPU against a checkout of the reference,
whose directory is the script's one argument.  Nothing here is imported by the
product or by the tests: those read only the committed .npz files.  The
reference's calibrators.py still says `np.float`, which NumPy 2 dropped: this
generator sets `np.float = float` before it imports it.

Per case two files (each below the 1 MiB limit): <name>.npz holds
  S [L, D], T [L, D]    the parameters (layer l: s, t)
  x [B, D] fp32, y [B] int64 labels, seed
  zs [L, B, D], ld [1]  Flow.forward(x) in fp32; ld64
  xs [L, B, D], ild [1] Flow.backward(zs[-1]) in fp32; ild64
  loss_cal, loss_ce     -mean(log(softmax(z)[y] + 1e-7) + ld)   (calibrators.py:287-291)
                        CE(z, y) - 0.7 * mean(ld * ones)  (the CE loss with a log-det weight)
                        in fp32, and *_64 in float64
  g_cal, g_ce           their autograd gradients, flat in state_dict order
                        (s, t per layer), fp32; *_64 in float64
  floor_zs, floor_xs, floor_ld, floor_rt
                        the reference's own fp32-vs-float64 error under
                        tests/_golden.rel_err (rt: xs[-1] against x)
  floor_g_cal, floor_g_ce   the same for the gradients under
                        tests/test_gpu_vjp._grad_err
  log_priors [D], probs [B, D] (the fp32 flow), probs64, floor_probs
                        Calibrator.predict(x) of an untrained calibrator
and <name>_f64.npz holds zs64, xs64 [L, B, D].

Draw: x ~ 2 N(0, 1), s ~ min(0.3, 1 / L) N(0, 1), t ~ min(0.5, 2 / L) N(0, 1).
Cases (the smallest that reach each code path of csrc/cnf_affine.hip):
  one       D=2   L=1   B=1    a single row: the log-det is still [1]
  d3        D=3   L=5   B=777  notebook shape
  d10       D=10  L=5   B=777
  init      D=10  L=5   B=300  the module's own zero init: identity forward,
                               non-zero gradients
  d17       D=17  L=3   B=130  odd D, 16 lanes per row
  d100      D=100 L=4   B=70   64 lanes per row
  tape      D=3   L=11  B=300  one layer past the register depth (10)
  contract  D=10  L=10  B=300  layer 0: s = -6, t = 3 (inverting it loses its input)
  centre    D=10  L=10  B=300  x ~ 5 + 0.1 N, layer 0: s = 0, t = -5 (the shift
                               cancels the data's mean)

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_affine.py REFERENCE_DIR
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else None
OUT = os.path.join(HERE, "affine")
DET = 0.7


def _reference():
    if REF is None or not os.path.isdir(REF):
        sys.exit("usage: gen_golden_affine.py REFERENCE_DIR")
    sys.dont_write_bytecode = True
    np.float = float  # the alias NumPy 2 removed
    sys.path.insert(0, REF)
    import calibrators as C  # the reference's
    from flows import flows as RF
    return C, RF


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / (np.abs(b) + 1.0)))


def grad_err(got, ref):
    sc = float(np.max(np.abs(ref))) + 1e-3
    return float(np.max(np.abs(got - ref))) / sc


def build(RF, D, L, rs, special):
    flow = RF.Flow([RF.AffineConstantLayer(D) for _ in range(L)])
    if special == "init":
        return flow
    S = (min(0.3, 1.0 / L) * rs.standard_normal((L, D))).astype(np.float32)
    T = (min(0.5, 2.0 / L) * rs.standard_normal((L, D))).astype(np.float32)
    if special == "contract":
        S[0], T[0] = -6.0, 3.0
    if special == "centre":
        S[0], T[0] = 0.0, -5.0
    with torch.no_grad():
        for l, ly in enumerate(flow.layers):
            ly.s.copy_(torch.from_numpy(S[l:l + 1]))
            ly.t.copy_(torch.from_numpy(T[l:l + 1]))
    return flow


def run(flow, x, y):
    ps = list(flow.parameters())
    zs, ld = flow(x)
    assert tuple(ld.shape) == (1,)
    z = zs[-1]
    probs = torch.softmax(z, dim=1)
    ce = torch.log(probs.gather(1, y.view(-1, 1)) + 1e-7)
    cal = -torch.mean(ce.squeeze() + ld)
    cel = torch.nn.functional.cross_entropy(z, y) - DET * torch.mean(ld * torch.ones_like(z[:, 0]))
    g_cal = torch.autograd.grad(cal, ps, retain_graph=True)
    g_ce = torch.autograd.grad(cel, ps)
    flat = lambda gs: torch.cat([g.reshape(-1) for g in gs]).detach().numpy()
    with torch.no_grad():
        xs, ild = flow.backward(z)
    assert tuple(ild.shape) == (1,)
    return {"zs": torch.stack(zs).detach().numpy(), "ld": ld.detach().numpy(),
            "xs": torch.stack(xs).numpy(), "ild": ild.numpy(), "loss_cal": cal.item(),
            "loss_ce": cel.item(), "g_cal": flat(g_cal), "g_ce": flat(g_ce)}


class FinalOutput(torch.nn.Module):
    """flow(x) -> (zs[-1], log_det): what the calibrator expects of its factory."""

    def __init__(self, flow):
        super().__init__()
        self.flow = flow

    def forward(self, x):
        zs, ld = self.flow(x)
        return zs[-1], ld


def calibrator(C, flow, log_priors, double):
    """The reference's TorchFlowCalibrator around `flow`, untrained.  double:
    predict_logits feeds the (float64) flow float64 rows instead of fp32."""
    cls = C.TorchFlowCalibrator
    if double:
        class Double(cls):
            def predict_logits(self, logits):
                preds, _ = self.flow(torch.as_tensor(logits, dtype=torch.double))
                return preds.detach().numpy()
        cls = Double
    cal = object.__new__(cls)
    cal.flow = FinalOutput(flow)
    cal.dev = torch.device("cpu")
    cal.log_priors = log_priors
    return cal


def record(C, RF, D, L, B, seed, special):
    rs = np.random.RandomState(seed)
    flow = build(RF, D, L, rs, special)
    x = (2.0 * rs.standard_normal((B, D))).astype(np.float32)
    if special == "centre":
        x = (5.0 + 0.1 * rs.standard_normal((B, D))).astype(np.float32)
    y = rs.randint(0, D, size=B).astype(np.int64)
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    f64 = copy.deepcopy(flow).double()
    r32 = run(flow, xt, yt)
    r64 = run(f64, xt.double(), yt)
    # Calibrator.predict: the priors of a skewed label draw, float64 rows in
    x64 = x.astype(np.float64)
    wts = 1.0 + np.arange(D, dtype=np.float64) / D
    yp = rs.choice(D, size=max(B, 50 * D), p=wts / wts.sum())
    assert (np.bincount(yp, minlength=D) > 0).all()
    lp = C.Calibrator._get_log_priors(None, np.eye(D)[yp])
    probs = calibrator(C, flow, lp, False).predict(x64)
    probs64 = calibrator(C, f64, lp, True).predict(x64)
    data = {
        "S": np.concatenate([ly.s.detach().numpy() for ly in flow.layers]),
        "T": np.concatenate([ly.t.detach().numpy() for ly in flow.layers]),
        "x": x, "y": y, "seed": np.int64(seed), "det": np.float64(DET),
        "zs": r32["zs"], "ld": r32["ld"], "xs": r32["xs"], "ild": r32["ild"],
        "ld64": r64["ld"], "ild64": r64["ild"],
        "loss_cal": np.float32(r32["loss_cal"]), "loss_ce": np.float32(r32["loss_ce"]),
        "loss_cal_64": np.float64(r64["loss_cal"]), "loss_ce_64": np.float64(r64["loss_ce"]),
        "g_cal": r32["g_cal"], "g_ce": r32["g_ce"], "g_cal_64": r64["g_cal"],
        "g_ce_64": r64["g_ce"],
        "floor_zs": np.float64(rel_err(r32["zs"], r64["zs"])),
        "floor_xs": np.float64(rel_err(r32["xs"], r64["xs"])),
        "floor_ld": np.float64(max(rel_err(r32["ld"], r64["ld"]), rel_err(r32["ild"], r64["ild"]))),
        "floor_rt": np.float64(rel_err(r32["xs"][-1], x)),
        "floor_g_cal": np.float64(grad_err(r32["g_cal"], r64["g_cal"])),
        "floor_g_ce": np.float64(grad_err(r32["g_ce"], r64["g_ce"])),
        "log_priors": lp, "probs": probs, "probs64": probs64,
        "floor_probs": np.float64(rel_err(probs, probs64)),
    }
    return data, {"zs64": r64["zs"], "xs64": r64["xs"]}


def _save(name, data):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **data)
    assert os.path.getsize(path) < (1 << 20), (name, os.path.getsize(path))
    return os.path.getsize(path)


def main():
    C, RF = _reference()
    cases = (("one", 2, 1, 1, 601, None), ("d3", 3, 5, 777, 602, None),
             ("d10", 10, 5, 777, 603, None), ("init", 10, 5, 300, 604, "init"),
             ("d17", 17, 3, 130, 605, None), ("d100", 100, 4, 70, 606, None),
             ("tape", 3, 11, 300, 607, None), ("contract", 10, 10, 300, 608, "contract"),
             ("centre", 10, 10, 300, 609, "centre"))
    for name, D, L, B, seed, special in cases:
        data, big = record(C, RF, D, L, B, seed, special)
        if special == "init":
            assert np.array_equal(data["zs"][-1], data["x"]) and np.abs(data["g_cal"]).max() > 0
        n1, n2 = _save(name, data), _save(name + "_f64", big)
        print("%s: floor zs=%.2e xs=%.2e ld=%.2e rt=%.2e probs=%.2e g_cal=%.2e g_ce=%.2e"
              "  %d + %d bytes"
              % (name, data["floor_zs"], data["floor_xs"], data["floor_ld"], data["floor_rt"],
                 data["floor_probs"], data["floor_g_cal"], data["floor_g_ce"], n1, n2))


if __name__ == "__main__":
    main()
