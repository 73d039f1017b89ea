"""Generate the planar-flow fixtures (tests/golden/planar/*.npz) FROM THE
REFERENCE ITSELF: its Flow([PlanarLayer(dim) ...]) (flows/flows.py:8-25,
129-165; get_Planarmodel of the calibration notebooks) on seeded inputs, in
fp32 and with the same module converted to float64.

Test infrastructure only; runs on the CPU against a checkout of the reference,
whose directory is the script's one argument.  Nothing here is imported
by the product or by the tests: those read only the committed .npz files.

Per case two files (each below the 1 MiB limit): <name>.npz holds
  W, U [L, D], Bv [L]   the parameters (layer l: w, u, b)
  x [B, D] fp32, y [B] int64 labels, det (the CE loss's log-det weight), seed
  zs [L, B, D], ld [B]  the reference's fp32 outputs
  loss_cal, loss_ce     -mean(log(softmax(z)[y] + 1e-7) + ld)   (calibrators.py:287-291)
                        CE(z, y) - det * mean(ld)               (run_experiment3D.py:107)
                        in fp32, and *_64 in float64
  g_cal, g_ce           their autograd gradients, flat in state_dict order
                        (w, u, b per layer), fp32; *_64 in float64
  floor_zs, floor_ld    the reference's own fp32-vs-float64 error under
                        tests/_golden.rel_err
  floor_g_cal, floor_g_ce   the same for the gradients under
                        tests/test_gpu_vjp._grad_err
  qmin                  min |1 + h'c| over rows and layers (float64)
and <name>_f64.npz holds zs64 [L, B, D] and ld64 [B].

The log-det log|1 + h'c| is ill-conditioned near 0, so a fixture must not sit
there: the generator asserts qmin >= 0.05 on the reference's float64 values and
takes the first seed of seed0, seed0 + 10, ... that passes.  The `nan` case
(w = 0 in layer 1: ||w|| = 0, so u_hat and everything after it is NaN) is
exempt; its NaN positions are what the tests compare.

Cases (the smallest that reach each code path of csrc/cnf_planar.hip):
  one    D=2   L=1   B=1    rand    0-d log-det
  d3     D=3   L=10  B=777  rand    notebook shape
  d10    D=10  L=10  B=777  rand    notebook shape
  d10n   D=10  L=10  B=777  normal  N(0,1) * 0.5 parameters
  d17    D=17  L=3   B=130  normal  odd D, 16 lanes per row
  d100   D=100 L=4   B=70   rand    64 lanes per row
  tape   D=3   L=11  B=300  normal  one layer past the register tape (10)
  nan    D=10  L=2   B=64   rand    w = 0 in layer 1

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_planar.py REFERENCE_DIR
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else None
OUT = os.path.join(HERE, "planar")
QMIN = 0.05
DET = 0.5


def _reference():
    if REF is None or not os.path.isdir(REF):
        sys.exit("usage: gen_golden_planar.py REFERENCE_DIR")
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    from flows import flows as RF  # the reference's
    return RF


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ok = ~np.isnan(b)
    assert (np.isnan(a) == np.isnan(b)).all()
    return float(np.max(np.abs(a[ok] - b[ok]) / (np.abs(b[ok]) + 1.0))) if ok.any() else 0.0


def grad_err(got, ref):
    sc = float(np.max(np.abs(ref))) + 1e-3
    return float(np.max(np.abs(got - ref))) / sc


def build(RF, D, L, init, seed, zero_w=None):
    torch.manual_seed(seed)
    flow = RF.Flow([RF.PlanarLayer(D) for _ in range(L)])
    if init == "normal":
        with torch.no_grad():
            for p in flow.parameters():
                p.copy_(torch.randn(p.shape) * 0.5)
    if zero_w is not None:
        with torch.no_grad():
            flow.layers[zero_w].w.zero_()
    return flow


def losses(flow, x, y, det):
    zs, ld = flow(x)
    z = zs[-1]
    probs = torch.softmax(z, dim=1)
    ce = torch.log(probs.gather(1, y.view(-1, 1)) + 1e-7)
    cal = -torch.mean(ce.squeeze() + ld)
    cel = torch.nn.functional.cross_entropy(z, y) - det * torch.mean(ld)
    return zs, ld, cal, cel


def run(flow, x, y, det):
    ps = list(flow.parameters())
    zs, ld, cal, cel = losses(flow, x, y, det)
    g_cal = torch.autograd.grad(cal, ps, retain_graph=True)
    g_ce = torch.autograd.grad(cel, ps)
    flat = lambda gs: torch.cat([g.reshape(-1) for g in gs]).detach().numpy()
    return (torch.stack(zs).detach().numpy(), ld.detach().reshape(-1).numpy(), cal.item(),
            cel.item(), flat(g_cal), flat(g_ce))


def qmin_of(flow64, x64):
    q = np.inf
    x = x64
    with torch.no_grad():
        for ly in flow64.layers:
            wtu = torch.dot(ly.w, ly.u)
            m = -1 + torch.log1p(torch.exp(wtu))
            u_hat = ly.u + (m - wtu) * ly.w / torch.norm(ly.w)
            h = torch.tanh(x @ ly.w + ly.b)
            q = min(q, float(torch.min(torch.abs(1 + (1 - h ** 2) * torch.dot(ly.w, u_hat)))))
            x = x + h.view(-1, 1) * u_hat.view(1, -1)
    return q


def record(RF, D, L, B, init, seed, zero_w=None):
    import copy
    flow = build(RF, D, L, init, seed, zero_w)
    rs = np.random.RandomState(seed + 1)
    x = (2.0 * rs.standard_normal((B, D))).astype(np.float32)
    y = rs.randint(0, D, size=B).astype(np.int64)
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    zs, ld, cal, cel, g_cal, g_ce = run(flow, xt, yt, DET)
    f64 = copy.deepcopy(flow).double()
    zs64, ld64, cal64, cel64, g_cal64, g_ce64 = run(f64, xt.double(), yt, DET)
    data = {
        "W": np.stack([ly.w.detach().numpy() for ly in flow.layers]),
        "U": np.stack([ly.u.detach().numpy() for ly in flow.layers]),
        "Bv": np.concatenate([ly.b.detach().numpy() for ly in flow.layers]),
        "x": x, "y": y, "det": np.float64(DET), "seed": np.int64(seed),
        "zs": zs, "ld": ld, "loss_cal": np.float32(cal), "loss_ce": np.float32(cel),
        "loss_cal_64": np.float64(cal64), "loss_ce_64": np.float64(cel64),
        "g_cal": g_cal, "g_ce": g_ce, "g_cal_64": g_cal64, "g_ce_64": g_ce64,
        "floor_zs": np.float64(rel_err(zs, zs64)), "floor_ld": np.float64(rel_err(ld, ld64)),
        "qmin": np.float64(qmin_of(f64, xt.double())),
    }
    if zero_w is None:
        data["floor_g_cal"] = np.float64(grad_err(g_cal, g_cal64))
        data["floor_g_ce"] = np.float64(grad_err(g_ce, g_ce64))
    return data, {"zs64": zs64, "ld64": ld64}


def _save(name, data):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **data)
    assert os.path.getsize(path) < (1 << 20), (name, os.path.getsize(path))
    return os.path.getsize(path)


def main():
    RF = _reference()
    cases = (("one", 2, 1, 1, "rand", 301, None), ("d3", 3, 10, 777, "rand", 302, None),
             ("d10", 10, 10, 777, "rand", 303, None), ("d10n", 10, 10, 777, "normal", 304, None),
             ("d17", 17, 3, 130, "normal", 305, None), ("d100", 100, 4, 70, "rand", 306, None),
             ("tape", 3, 11, 300, "normal", 307, None), ("nan", 10, 2, 64, "rand", 308, 1))
    for name, D, L, B, init, seed0, zero_w in cases:
        for seed in range(seed0, seed0 + 500, 10):
            data, big = record(RF, D, L, B, init, seed, zero_w)
            if zero_w is not None or data["qmin"] >= QMIN:
                break
        assert zero_w is not None or data["qmin"] >= QMIN, name
        n1, n2 = _save(name, data), _save(name + "_f64", big)
        print("%s: seed=%d qmin=%.3f floor zs=%.2e ld=%.2e g_cal=%.2e g_ce=%.2e  %d + %d bytes"
              % (name, seed, data["qmin"], data["floor_zs"], data["floor_ld"],
                 data.get("floor_g_cal", np.nan), data.get("floor_g_ce", np.nan), n1, n2))


if __name__ == "__main__":
    main()
