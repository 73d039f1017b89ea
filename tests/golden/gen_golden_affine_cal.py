"""Generate the affine calibrator fixtures (tests/golden/affine_cal/{full,mb128}.npz)
FROM THE REFERENCE ITSELF: its TorchFlowCalibrator (calibrators.py:239-353)
trained on the CPU around its Flow of five AffineConstantLayers
(flows/flows.py:8-25, 40-65; the stack of train-flows-det.ipynb), and its
predict of held-out rows.

Test infrastructure only; runs on the CPU against a checkout of the reference,
whose directory is the script's one argument.  Nothing here is imported by the
product or by the tests: those read only the committed .npz files.  The
reference's calibrators.py still says `np.float`, which NumPy 2 dropped: this
generator sets `np.float = float` before it imports it.

The recipe is that of gen_golden_radial_cal.py: D = 3, N = 300, 5 epochs,
torch.manual_seed(seed) before the constructor (every DataLoader shuffle draws
from it; the layers' own init is zeros), rows and labels from RandomState(31).
`full` trains with batch 300, `mb128` with batch 128 (three batches per pass,
the last of 44 rows).

Adam's first steps move a parameter by lr * sign(gradient), so a gradient
entry near zero makes the fit sensitive to rounding.  The generator therefore
also runs the reference's fit with the flow in float64 and the same seed, and
takes the first seed of 7, 8, ... at which the fp32 and float64 final
parameters agree within a quarter of the tests' parameter bar
(steps * lr * 2e-2): no such entry decides the test.

Recorded: logits [N, D] float64 and labels [N], seed, epochs, batch_size,
S0, T0 [L, D] (the parameters before the first step: zeros) and S, T (after
the last), S64, T64 (the float64 fit's), the history lists loss / ce / log_det
[epochs] (fp32), held [50, D] float64 and pred = predict(held) (float64).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_affine_cal.py REFERENCE_DIR
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else None
OUT = os.path.join(HERE, "affine_cal")
D, N, LAYERS, EPOCHS, SEED0, HELD, LR = 3, 300, 5, 5, 7, 50, 1e-3


def _reference():
    if REF is None or not os.path.isdir(REF):
        sys.exit("usage: gen_golden_affine_cal.py REFERENCE_DIR")
    sys.dont_write_bytecode = True
    np.float = float  # the alias NumPy 2 removed
    sys.path.insert(0, REF)
    import calibrators as C  # the reference's
    from flows import flows as RF
    return C, RF


def _params(flow):
    return (np.concatenate([ly.s.detach().numpy().copy() for ly in flow.layers]),
            np.concatenate([ly.t.detach().numpy().copy() for ly in flow.layers]))


def main():
    C, RF = _reference()
    initial = []

    def factory(double):
        class AffineFactory(torch.nn.Module):
            def __init__(self, dim, layers=LAYERS, **kwargs):
                super().__init__()
                self.flow = RF.Flow([RF.AffineConstantLayer(dim) for _ in range(layers)])
                if double:
                    self.flow.double()
                initial.append(_params(self.flow))

            def forward(self, x):
                zs, ld = self.flow(x)
                return zs[-1], ld
        return AffineFactory

    rs = np.random.RandomState(31)
    logits = 2.0 * rs.standard_normal((N, D))
    labels = rs.randint(0, D, size=N)
    held = 2.0 * rs.standard_normal((HELD, D))
    os.makedirs(OUT, exist_ok=True)

    def fit(double, seed, bs):
        del initial[:]
        torch.manual_seed(seed)
        return C.TorchFlowCalibrator(factory(double), logits, np.eye(D)[labels], layers=LAYERS,
                                     epochs=EPOCHS, batch_size=bs, dev=torch.device("cpu"))

    for name, bs in (("full", N), ("mb128", 128)):
        steps = EPOCHS * -(-N // bs)
        quarter = steps * LR * 2e-2 / 4
        for seed in range(SEED0, SEED0 + 50):
            c64 = fit(True, seed, bs)
            S64, T64 = _params(c64.flow.flow)
            cal = fit(False, seed, bs)
            S0, T0 = initial[0]
            S, T = _params(cal.flow.flow)
            gap = max(np.abs(S - S64).max(), np.abs(T - T64).max())
            if gap <= quarter:
                break
        assert gap <= quarter, (name, gap, quarter)
        hist = {k: np.array([float(v) for v in cal.history[k]], dtype=np.float32)
                for k in ("loss", "ce", "log_det")}
        pred = cal.predict(held)
        data = {"logits": logits, "labels": labels.astype(np.int64), "seed": np.int64(seed),
                "epochs": np.int64(EPOCHS), "batch_size": np.int64(bs), "S0": S0, "T0": T0,
                "S": S, "T": T, "S64": S64, "T64": T64, "loss": hist["loss"], "ce": hist["ce"],
                "log_det": hist["log_det"], "held": held, "pred": pred}
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **data)
        assert os.path.getsize(path) < (1 << 20)
        print("%s: seed %d  fp32-f64 gap %.2e (quarter bar %.2e)  loss %s  log_det %s  %d bytes"
              % (name, seed, gap, quarter, hist["loss"], hist["log_det"], os.path.getsize(path)))


if __name__ == "__main__":
    main()
