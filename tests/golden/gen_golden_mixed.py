"""Generate the mixed-flow fixtures (tests/golden/mixed/*.npz) FROM THE
REFERENCE ITSELF: its Flow of PlanarLayers, RadialLayers and
AffineConstantLayers in a given order (flows/flows.py:8-37, 40-65, 129-193),
forward, and its Calibrator.predict around that flow (calibrators.py:40-44,
330-353) on seeded inputs, in fp32 and with the same module converted to
float64.

Test infrastructure only; runs on the CPU against a checkout of the reference,
whose directory is the script's one argument.  Nothing here is imported by the
product or by the tests: those read only the committed .npz files.  The
reference's calibrators.py still says `np.float`, which NumPy 2 dropped: this
generator sets `np.float = float` before it imports it.  The parameter draw is
tests/_mixed_ref.draw_params.

Only orders the reference's loop accepts are used (it accumulates the log-det
in place into the first layer's): planar first when B > 1.

Per case two files (each below the 1 MiB limit): <name>.npz holds
  order                 the spec string over P, R, A
  p<l>_<name>           layer l's parameters under their state_dict names
                        (w, u, b / z0, a, b / s, t)
  x [B, D] fp32, y [B] int64 labels, seed, det
  zs [L, B, D], ld      Flow.forward(x) in fp32, ld in the loop's shape; ld64
  loss_cal, loss_ce     -mean(log(softmax(z)[y] + 1e-7) + ld)   (calibrators.py:287-291)
                        CE(z, y) - 0.7 * mean(ld over the rows)
                        in fp32, and *_64 in float64
  g_cal, g_ce           their autograd gradients, flat in state_dict order,
                        fp32; *_64 in float64
  floor_zs, floor_ld, floor_zs_step [L]
                        the reference's own fp32-vs-float64 error under
                        tests/_golden.rel_err (per layer output: _step)
  floor_g_cal, floor_g_ce   the same for the gradients under
                        tests/test_gpu_vjp._grad_err
  log_priors [D], probs [B, D] (the fp32 flow), probs64, floor_probs
                        Calibrator.predict(x) of an untrained calibrator
and <name>_f64.npz holds zs64 [L, B, D].

Cases:
  pra       PRA          D=3   B=777  notebook shape
  d10       PRPRPRPRPA   D=10  B=777  register-resident depth
  deep      (PRA) x 6    D=3   B=300  L = 18 crosses a checkpoint segment
  contract  PAPR         D=10  B=300  affine s = -6, t = 3: inverting it loses its input
  d17       PAR          D=17  B=130  16 lanes per row, odd D
  d100      PRAP         D=100 B=70   64 lanes per row
  ar        ARA          D=4   B=50   the log-det is [1]
  one       AP           D=2   B=1    a single row: [1]

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_mixed.py REFERENCE_DIR
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else None
OUT = os.path.join(HERE, "mixed")
DET = 0.7
NAMES = {"P": ("w", "u", "b"), "R": ("z0", "a", "b"), "A": ("s", "t")}


def _reference():
    if REF is None or not os.path.isdir(REF):
        sys.exit("usage: gen_golden_mixed.py REFERENCE_DIR")
    sys.dont_write_bytecode = True
    np.float = float  # the alias NumPy 2 removed
    sys.path.insert(0, REF)
    import calibrators as C  # the reference's
    from flows import flows as RF
    return C, RF


def _draw_params():
    sys.path.append(os.path.dirname(HERE))
    import _mixed_ref
    return _mixed_ref.draw_params


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / (np.abs(b) + 1.0)))


def grad_err(got, ref):
    sc = float(np.max(np.abs(ref))) + 1e-3
    return float(np.max(np.abs(got - ref))) / sc


def build(RF, D, params):
    cls = {"P": lambda: RF.PlanarLayer(D), "R": lambda: RF.RadialLayer(D),
           "A": lambda: RF.AffineConstantLayer(D)}
    flow = RF.Flow([cls[k]() for k, _ in params])
    with torch.no_grad():
        for ly, (k, p) in zip(flow.layers, params):
            for n, v in zip(NAMES[k], p):
                t = getattr(ly, n)
                t.copy_(torch.from_numpy(np.asarray(v, dtype=np.float32)).reshape(t.shape))
    return flow


def run(flow, x, y):
    ps = list(flow.parameters())
    B = x.shape[0]
    zs, ld = flow(x)
    z = zs[-1]
    probs = torch.softmax(z, dim=1)
    ce = torch.log(probs.gather(1, y.view(-1, 1)) + 1e-7)
    cal = -torch.mean(ce.reshape(-1) + ld)
    rows = ld * torch.ones(B, dtype=z.dtype)
    cel = torch.nn.functional.cross_entropy(z, y) - DET * torch.mean(rows)
    g_cal = torch.autograd.grad(cal, ps, retain_graph=True)
    g_ce = torch.autograd.grad(cel, ps)
    flat = lambda gs: torch.cat([g.reshape(-1) for g in gs]).detach().numpy()
    return {"zs": torch.stack(zs).detach().numpy(), "ld": ld.detach().numpy(),
            "loss_cal": cal.item(), "loss_ce": cel.item(), "g_cal": flat(g_cal),
            "g_ce": flat(g_ce)}


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


def record(C, RF, draw, order, D, B, seed, contract):
    rs = np.random.RandomState(seed)
    params = draw(rs, D, order, contract=contract)
    flow = build(RF, D, params)
    x = (2.0 * rs.standard_normal((B, D))).astype(np.float32)
    y = rs.randint(0, D, size=B).astype(np.int64)
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    f64 = copy.deepcopy(flow).double()
    r32 = run(flow, xt, yt)
    r64 = run(f64, xt.double(), yt)
    x64 = x.astype(np.float64)
    wts = 1.0 + np.arange(D, dtype=np.float64) / D
    yp = rs.choice(D, size=max(B, 50 * D), p=wts / wts.sum())
    assert (np.bincount(yp, minlength=D) > 0).all()
    lp = C.Calibrator._get_log_priors(None, np.eye(D)[yp])
    probs = calibrator(C, flow, lp, False).predict(x64)
    probs64 = calibrator(C, f64, lp, True).predict(x64)
    data = {
        "order": np.array(order), "x": x, "y": y, "seed": np.int64(seed), "det": np.float64(DET),
        "zs": r32["zs"], "ld": r32["ld"], "ld64": r64["ld"],
        "loss_cal": np.float32(r32["loss_cal"]), "loss_ce": np.float32(r32["loss_ce"]),
        "loss_cal_64": np.float64(r64["loss_cal"]), "loss_ce_64": np.float64(r64["loss_ce"]),
        "g_cal": r32["g_cal"], "g_ce": r32["g_ce"], "g_cal_64": r64["g_cal"],
        "g_ce_64": r64["g_ce"],
        "floor_zs": np.float64(rel_err(r32["zs"], r64["zs"])),
        "floor_zs_step": np.array([rel_err(a, b) for a, b in zip(r32["zs"], r64["zs"])]),
        "floor_ld": np.float64(rel_err(r32["ld"], r64["ld"])),
        "floor_g_cal": np.float64(grad_err(r32["g_cal"], r64["g_cal"])),
        "floor_g_ce": np.float64(grad_err(r32["g_ce"], r64["g_ce"])),
        "log_priors": lp, "probs": probs, "probs64": probs64,
        "floor_probs": np.float64(rel_err(probs, probs64)),
    }
    for l, (k, p) in enumerate(params):
        for n, v in zip(NAMES[k], p):
            data["p%d_%s" % (l, n)] = np.asarray(v, dtype=np.float32)
    return data, {"zs64": r64["zs"]}


def _save(name, data):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **data)
    assert os.path.getsize(path) < (1 << 20), (name, os.path.getsize(path))
    return os.path.getsize(path)


def main():
    C, RF = _reference()
    draw = _draw_params()
    cases = (("pra", "PRA", 3, 777, 701), ("d10", "PRPRPRPRPA", 10, 777, 702),
             ("deep", "PRA" * 6, 3, 300, 703), ("contract", "PAPR", 10, 300, 704),
             ("d17", "PAR", 17, 130, 705), ("d100", "PRAP", 100, 70, 706),
             ("ar", "ARA", 4, 50, 707), ("one", "AP", 2, 1, 708))
    for name, order, D, B, seed in cases:
        data, big = record(C, RF, draw, order, D, B, seed, name == "contract")
        n1, n2 = _save(name, data), _save(name + "_f64", big)
        print("%s: ld%s floor zs=%.2e ld=%.2e probs=%.2e g_cal=%.2e g_ce=%.2e  %d + %d bytes"
              % (name, tuple(data["ld"].shape), data["floor_zs"], data["floor_ld"],
                 data["floor_probs"], data["floor_g_cal"], data["floor_g_ce"], n1, n2))


if __name__ == "__main__":
    main()
