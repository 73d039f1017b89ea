"""Generate the planar predict fixtures (tests/golden/planar_predict/*.npz) FROM
THE REFERENCE ITSELF: its Calibrator.predict around
TorchFlowCalibrator.predict_post (calibrators.py:40-44, 330-353) over its
Flow([PlanarLayer ...]) (flows/flows.py:8-25, 129-165) holding the parameters
of the committed planar fixtures (tests/golden/planar/*.npz).

Test infrastructure only; runs on the CPU against a checkout of the reference,
whose directory is the script's one argument.  Nothing here is imported by the
product or by the tests: those read only the committed .npz files.  The
reference's calibrators.py still says `np.float`, which NumPy 2 dropped: this
generator sets `np.float = float` before it imports it.

The calibrator object is made without running its constructor (which trains):
the generator sets the three attributes predict reads -- flow, dev, log_priors
-- and calls the reference's own predict.  The flow is the reference's Flow
behind a wrapper whose call returns (zs[-1], log_det), as the calibrator's
factories do.  log_priors are the reference's Calibrator._get_log_priors of the
one-hot rows of a seeded draw of max(B, 50 D) labels with class weights
proportional to 1 + c / D (non-uniform, yet every class occurs; `inf`: the last
class has weight 0, so it never occurs and its log-prior is -inf).

Per case one file:
  x [B, D] fp32 (handed to predict as float64 rows, so the centring runs in
            float64, as it does for the calibrator's usual float64 logits),
  log_priors [D] float64, seed
  probs     predict(x) as the reference runs it (fp32 flow, float64 afterwards)
  probs64   the same with the flow converted to float64 and fed float64 rows
  ld64 [B]  log-det of the centred rows, from the float64 flow
  floor_ld     rel_err of the fp32 flow's log-det against ld64
  floor_probs  tests/_golden.rel_err(probs, probs64)
  qmin      min |1 + h'c| over rows and layers on the centred rows (float64)

Cases (parameters from tests/golden/planar/<from>.npz):
  one   from one   D=2   L=1   B=1
  d3    from d3    D=3   L=10  B=777
  d10   from d10   D=10  L=10  B=777
  d17   from d17   D=17  L=3   B=130   padding columns, 16 lanes per row
  d100  from d100  D=100 L=4   B=70    64 lanes per row
  nan   from nan   D=10  L=2   B=64    w = 0 in layer 1: NaN positions compared
  inf   from d3    D=3   L=10  B=64    one log-prior is -inf: every row NaN

As for the planar fixtures, the log-det is ill-conditioned near 0: the generator
takes the first seed of seed0, seed0 + 10, ... with qmin >= 0.05 (`nan` exempt).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_planar_predict.py REFERENCE_DIR
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else None
SRC = os.path.join(HERE, "planar")
OUT = os.path.join(HERE, "planar_predict")
QMIN = 0.05

sys.path.insert(0, os.path.dirname(HERE))
from _golden import rel_err  # noqa: E402  (tests/_golden.py)


def _reference():
    if REF is None or not os.path.isdir(REF):
        sys.exit("usage: gen_golden_planar_predict.py REFERENCE_DIR")
    sys.dont_write_bytecode = True
    np.float = float  # the alias NumPy 2 removed
    sys.path.insert(0, REF)
    import calibrators as C  # the reference's
    from flows import flows as RF
    return C, RF


class FinalOutput(torch.nn.Module):
    """flow(x) -> (zs[-1], log_det): what the calibrator expects of its factory."""

    def __init__(self, flow):
        super().__init__()
        self.flow = flow

    def forward(self, x):
        zs, ld = self.flow(x)
        return zs[-1], ld


def build_flow(RF, d):
    L, D = d["W"].shape
    flow = RF.Flow([RF.PlanarLayer(D) for _ in range(L)])
    with torch.no_grad():
        for l, ly in enumerate(flow.layers):
            ly.w.copy_(torch.from_numpy(d["W"][l]))
            ly.u.copy_(torch.from_numpy(d["U"][l]))
            ly.b.copy_(torch.from_numpy(d["Bv"][l:l + 1]))
    return flow


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


def record(C, RF, src, B, seed, drop_last):
    d = np.load(os.path.join(SRC, src + ".npz"))
    L, D = d["W"].shape
    flow = build_flow(RF, d)
    f64 = copy.deepcopy(flow).double()
    rs = np.random.RandomState(seed)
    x = (2.0 * rs.standard_normal((B, D))).astype(np.float32)
    x64 = x.astype(np.float64)  # predict centres in its input's precision: float64 rows
    wts = 1.0 + np.arange(D, dtype=np.float64) / D
    if drop_last:
        wts[-1] = 0.0
    y = rs.choice(D, size=max(B, 50 * D), p=wts / wts.sum())
    assert (np.bincount(y, minlength=D) > 0).sum() == D - int(drop_last)
    with np.errstate(divide="ignore"):
        lp = C.Calibrator._get_log_priors(None, np.eye(D)[y])
    with np.errstate(invalid="ignore", divide="ignore"):
        probs = calibrator(C, flow, lp, False).predict(x64)
        probs64 = calibrator(C, f64, lp, True).predict(x64)
    xc = x64 - np.mean(x64, axis=1, keepdims=True)      # calibrators.py:42
    with torch.no_grad():
        _, ld32 = flow(torch.as_tensor(xc, dtype=torch.float))
        _, ld64 = f64(torch.as_tensor(xc, dtype=torch.double))
    ld32, ld64 = ld32.reshape(-1).numpy(), ld64.reshape(-1).numpy()
    return {"x": x, "log_priors": lp, "seed": np.int64(seed), "probs": probs, "probs64": probs64,
            "ld64": ld64, "floor_ld": np.float64(rel_err(ld32, ld64)),
            "floor_probs": np.float64(rel_err(probs, probs64)),
            "qmin": np.float64(qmin_of(f64, torch.as_tensor(xc, dtype=torch.double)))}


def main():
    C, RF = _reference()
    os.makedirs(OUT, exist_ok=True)
    cases = (("one", "one", 1, 401, False), ("d3", "d3", 777, 402, False),
             ("d10", "d10", 777, 403, False), ("d17", "d17", 130, 404, False),
             ("d100", "d100", 70, 405, False), ("nan", "nan", 64, 406, False),
             ("inf", "d3", 64, 407, True))
    for name, src, B, seed0, drop_last in cases:
        for seed in range(seed0, seed0 + 500, 10):
            data = record(C, RF, src, B, seed, drop_last)
            if name == "nan" or data["qmin"] >= QMIN:
                break
        assert name == "nan" or data["qmin"] >= QMIN, name
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **data)
        assert os.path.getsize(path) < (1 << 20), (name, os.path.getsize(path))
        print("%s: seed=%d qmin=%.3f floor probs=%.2e ld=%.2e nan rows=%d  %d bytes"
              % (name, seed, data["qmin"], data["floor_probs"], data["floor_ld"],
                 int(np.isnan(data["probs64"]).any(axis=1).sum()), os.path.getsize(path)))


if __name__ == "__main__":
    main()
