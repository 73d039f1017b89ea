"""Generate the radial-flow fixtures (tests/golden/radial/*.npz) FROM THE
REFERENCE ITSELF: its Flow([RadialLayer(dim) ...]) (flows/flows.py:8-25,
168-193) and its Calibrator.predict around that flow (calibrators.py:40-44,
330-353) on seeded inputs, in fp32 and with the same module converted to
float64.

Test infrastructure only; runs on the CPU against a checkout of the reference,
whose directory is the script's one argument.  Nothing here is imported
by the product or by the tests: those read only the committed .npz files.  The
reference's calibrators.py still says `np.float`, which NumPy 2 dropped: this
generator sets `np.float = float` before it imports it.

Per case two files (each below the 1 MiB limit): <name>.npz holds
  Z0 [L, D], A [L], Bv [L]   the parameters (layer l: z0, a, b)
  x [B, D] fp32, y [B] int64 labels, seed
  zs [L, B, D]          the reference's fp32 outputs (its log-det is the
                        constant log(1.0) = 0 and is not recorded)
  loss_cal, loss_ce     -mean(log(softmax(z)[y] + 1e-7) + 0)    (calibrators.py:287-291)
                        CE(z, y)
                        in fp32, and *_64 in float64
  g_cal, g_ce           their autograd gradients, flat in state_dict order
                        (z0, a, b per layer), fp32; *_64 in float64
  floor_zs              the reference's own fp32-vs-float64 error under
                        tests/_golden.rel_err
  floor_g_cal, floor_g_ce   the same for the gradients under
                        tests/test_gpu_vjp._grad_err
  amin, rmin            min (a + r) and min r over rows and layers (float64),
                        over the rows as given and over the centred rows
                        predict feeds the flow
  log_priors [D], probs [B, D] (the fp32 flow), probs64, floor_probs
                        Calibrator.predict(x) of an untrained calibrator
and <name>_f64.npz holds zs64 [L, B, D].

h = 1 / (a + r) is ill-conditioned near a + r = 0 and the norm's gradient near
r = 0, so a fixture must not sit there: the generator asserts amin >= 0.05 and
rmin >= 1e-3 on the reference's float64 values and takes the first seed of
seed0, seed0 + 10, ... that passes.  `zero` is exempt from rmin and `sing`
from both; `sing` records no gradients.

Cases (the smallest that reach each code path of csrc/cnf_radial.hip):
  one    D=2   L=1   B=1    rand    0-d log-det, single row
  d3     D=3   L=10  B=777  rand    notebook shape
  d10    D=10  L=10  B=777  rand    notebook shape
  d10n   D=10  L=10  B=777  normal  N(0,1) * 0.5 parameters, a <- |a| + 0.1
  d17    D=17  L=3   B=130  normal  odd D, 16 lanes per row
  d100   D=100 L=4   B=70   rand    64 lanes per row
  tape   D=3   L=11  B=300  normal  one layer past the register tape (10)
  neg    D=10  L=3   B=64   rand    layer 1: a = -0.3, z0 += 3 (a < 0, a + r well above 0)
  zero   D=10  L=2   B=64   rand    row 5 of x = layer 0's z0 bit for bit: r == 0
  sing   D=10  L=2   B=64   rand    as zero with layer 0's a = 0: h = inf, that row NaN

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_radial.py REFERENCE_DIR
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else None
OUT = os.path.join(HERE, "radial")
AMIN, RMIN = 0.05, 1e-3
REG_TAPE = 10  # kRegL of csrc/cnf_radial.hip


def _reference():
    if REF is None or not os.path.isdir(REF):
        sys.exit("usage: gen_golden_radial.py REFERENCE_DIR")
    sys.dont_write_bytecode = True
    np.float = float  # the alias NumPy 2 removed
    sys.path.insert(0, REF)
    import calibrators as C  # the reference's
    from flows import flows as RF
    return C, RF


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ok = ~np.isnan(b)
    assert (np.isnan(a) == np.isnan(b)).all()
    return float(np.max(np.abs(a[ok] - b[ok]) / (np.abs(b[ok]) + 1.0))) if ok.any() else 0.0


def grad_err(got, ref):
    sc = float(np.max(np.abs(ref))) + 1e-3
    return float(np.max(np.abs(got - ref))) / sc


def build(RF, D, L, init, seed, special):
    torch.manual_seed(seed)
    flow = RF.Flow([RF.RadialLayer(D) for _ in range(L)])
    with torch.no_grad():
        if init == "normal":
            for p in flow.parameters():
                p.copy_(torch.randn(p.shape) * 0.5)
            for ly in flow.layers:
                ly.a.copy_(ly.a.abs() + 0.1)
        if special == "neg":
            flow.layers[1].a.fill_(-0.3)
            flow.layers[1].z0.add_(3.0)
        if special == "sing":
            flow.layers[0].a.zero_()
    return flow


def losses(flow, x, y):
    zs, ld = flow(x)
    z = zs[-1]
    probs = torch.softmax(z, dim=1)
    ce = torch.log(probs.gather(1, y.view(-1, 1)) + 1e-7)
    cal = -torch.mean(ce.squeeze() + ld)
    cel = torch.nn.functional.cross_entropy(z, y)
    return zs, cal, cel


def run(flow, x, y, grads):
    ps = list(flow.parameters())
    zs, cal, cel = losses(flow, x, y)
    out = [torch.stack(zs).detach().numpy(), cal.item(), cel.item()]
    if grads:
        g_cal = torch.autograd.grad(cal, ps, retain_graph=True)
        g_ce = torch.autograd.grad(cel, ps)
        flat = lambda gs: torch.cat([g.reshape(-1) for g in gs]).detach().numpy()
        out += [flat(g_cal), flat(g_ce)]
    return out


def mins_of(flow64, x64):
    """(min (a + r), min r) over rows and layers, float64."""
    amin = rmin = np.inf
    x = x64
    with torch.no_grad():
        for ly in flow64.layers:
            r = torch.norm(x - ly.z0, dim=1)
            amin, rmin = min(amin, float(torch.min(ly.a + r))), min(rmin, float(torch.min(r)))
            x, _ = ly(x)
    return amin, rmin


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


def record(C, RF, D, L, B, init, seed, special):
    flow = build(RF, D, L, init, seed, special)
    rs = np.random.RandomState(seed + 1)
    x = (2.0 * rs.standard_normal((B, D))).astype(np.float32)
    y = rs.randint(0, D, size=B).astype(np.int64)
    if special in ("zero", "sing"):
        x[5] = flow.layers[0].z0.detach().numpy()
    grads = special != "sing"
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    f64 = copy.deepcopy(flow).double()
    with np.errstate(invalid="ignore", divide="ignore"):
        r32 = run(flow, xt, yt, grads)
        r64 = run(f64, xt.double(), yt, grads)
    amin, rmin = mins_of(f64, xt.double())
    # Calibrator.predict: the priors of a skewed label draw, float64 rows in
    x64 = x.astype(np.float64)
    wts = 1.0 + np.arange(D, dtype=np.float64) / D
    yp = rs.choice(D, size=max(B, 50 * D), p=wts / wts.sum())
    assert (np.bincount(yp, minlength=D) > 0).all()
    lp = C.Calibrator._get_log_priors(None, np.eye(D)[yp])
    probs = calibrator(C, flow, lp, False).predict(x64)
    probs64 = calibrator(C, f64, lp, True).predict(x64)
    xc = torch.from_numpy(x64 - np.mean(x64, axis=1, keepdims=True))
    amin_c, rmin_c = mins_of(f64, xc)
    data = {
        "Z0": np.stack([ly.z0.detach().numpy() for ly in flow.layers]),
        "A": np.concatenate([ly.a.detach().numpy() for ly in flow.layers]),
        "Bv": np.concatenate([ly.b.detach().numpy() for ly in flow.layers]),
        "x": x, "y": y, "seed": np.int64(seed), "zs": r32[0],
        "loss_cal": np.float32(r32[1]), "loss_ce": np.float32(r32[2]),
        "loss_cal_64": np.float64(r64[1]), "loss_ce_64": np.float64(r64[2]),
        "floor_zs": np.float64(rel_err(r32[0], r64[0])),
        "amin": np.float64(min(amin, amin_c)), "rmin": np.float64(min(rmin, rmin_c)),
        "log_priors": lp, "probs": probs, "probs64": probs64,
        "floor_probs": np.float64(rel_err(probs, probs64)),
    }
    if grads:
        data.update({"g_cal": r32[3], "g_ce": r32[4], "g_cal_64": r64[3], "g_ce_64": r64[4],
                     "floor_g_cal": np.float64(grad_err(r32[3], r64[3])),
                     "floor_g_ce": np.float64(grad_err(r32[4], r64[4]))})
    return data, {"zs64": r64[0]}


def _save(name, data):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **data)
    assert os.path.getsize(path) < (1 << 20), (name, os.path.getsize(path))
    return os.path.getsize(path)


def _accept(data, special):
    if special == "sing":
        return True
    return data["amin"] >= AMIN and (special == "zero" or data["rmin"] >= RMIN)


def main():
    C, RF = _reference()
    cases = (("one", 2, 1, 1, "rand", 501, None), ("d3", 3, 10, 777, "rand", 502, None),
             ("d10", 10, 10, 777, "rand", 503, None), ("d10n", 10, 10, 777, "normal", 504, None),
             ("d17", 17, 3, 130, "normal", 505, None), ("d100", 100, 4, 70, "rand", 506, None),
             ("tape", 3, REG_TAPE + 1, 300, "normal", 507, None),
             ("neg", 10, 3, 64, "rand", 508, "neg"), ("zero", 10, 2, 64, "rand", 509, "zero"),
             ("sing", 10, 2, 64, "rand", 510, "sing"))
    for name, D, L, B, init, seed0, special in cases:
        for seed in range(seed0, seed0 + 500, 10):
            data, big = record(C, RF, D, L, B, init, seed, special)
            if _accept(data, special):
                break
        assert _accept(data, special), name
        if special == "zero":
            assert data["rmin"] == 0.0 and np.isfinite(data["zs"]).all()
            assert np.isfinite(data["g_cal_64"]).all() and np.isfinite(data["g_ce_64"]).all()
        if special == "sing":
            nan_rows = np.isnan(data["zs"]).any(axis=(0, 2))
            assert nan_rows[5] and nan_rows.sum() == 1
        n1, n2 = _save(name, data), _save(name + "_f64", big)
        print("%s: seed=%d amin=%.3f rmin=%.2e floor zs=%.2e probs=%.2e g_cal=%.2e g_ce=%.2e"
              "  %d + %d bytes"
              % (name, seed, data["amin"], data["rmin"], data["floor_zs"], data["floor_probs"],
                 data.get("floor_g_cal", np.nan), data.get("floor_g_ce", np.nan), n1, n2))


if __name__ == "__main__":
    main()
