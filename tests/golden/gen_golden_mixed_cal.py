"""Generate the mixed calibrator fixtures (tests/golden/mixed_cal/{full,mb128}.npz)
FROM THE REFERENCE ITSELF: its TorchFlowCalibrator (calibrators.py:239-353)
trained on the CPU around its Flow of PlanarLayer, RadialLayer, PlanarLayer,
RadialLayer, AffineConstantLayer (flows/flows.py:8-25, 40-65, 129-193), and its
predict of held-out rows.

Test infrastructure only; runs on the CPU against a checkout of the reference,
whose directory is the script's one argument.  Nothing here is imported by the
product or by the tests: those read only the committed .npz files.  The
reference's calibrators.py still says `np.float`, which NumPy 2 dropped: this
generator sets `np.float = float` before it imports it.

The recipe is that of gen_golden_affine_cal.py: D = 3, N = 300, 5 epochs,
torch.manual_seed(seed) before the constructor (the planar and radial layers'
torch.rand init and every DataLoader shuffle draw from it), rows and labels
from RandomState(31).  `full` trains with batch 300, `mb128` with batch 128
(three batches per pass, the last of 44 rows).

Adam's first steps move a parameter by lr * sign(gradient), so a gradient
entry near zero makes the fit sensitive to rounding.  The generator therefore
also runs the reference's fit with the flow in float64 and the same seed (the
float64 flow starts from the fp32 init, converted, and is fed its rows as
float64), and takes the first seed of
7, 8, ... at which the fp32 and float64 final parameters agree within a quarter
of the tests' parameter bar (steps * lr * 2e-2): no such entry decides the test.

Recorded: order ("PRPRA"), logits [N, D] float64 and labels [N], seed, epochs,
batch_size, P0 (the flat parameters in state_dict order before the first
step), P (after the last), P64 (the float64 fit's), the history lists loss /
ce / log_det [epochs] (fp32), held [50, D] float64 and pred = predict(held)
(float64).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_mixed_cal.py REFERENCE_DIR
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else None
OUT = os.path.join(HERE, "mixed_cal")
ORDER = "PRPRA"
D, N, EPOCHS, SEED0, HELD, LR = 3, 300, 5, 7, 50, 1e-3


def _reference():
    if REF is None or not os.path.isdir(REF):
        sys.exit("usage: gen_golden_mixed_cal.py REFERENCE_DIR")
    sys.dont_write_bytecode = True
    np.float = float  # the alias NumPy 2 removed
    sys.path.insert(0, REF)
    import calibrators as C  # the reference's
    from flows import flows as RF
    return C, RF


def _params(flow):
    return np.concatenate([p.detach().numpy().reshape(-1).copy() for p in flow.parameters()])


def main():
    C, RF = _reference()
    initial = []

    def factory(double):
        class MixedFactory(torch.nn.Module):
            def __init__(self, dim, **kwargs):
                super().__init__()
                cls = {"P": RF.PlanarLayer, "R": RF.RadialLayer, "A": RF.AffineConstantLayer}
                self.flow = RF.Flow([cls[c](dim) for c in ORDER])   # fp32 init, as drawn
                initial.append(_params(self.flow))
                if double:
                    self.flow.double()

            def forward(self, x):
                zs, ld = self.flow(x.double() if double else x)
                return zs[-1], ld
        return MixedFactory

    rs = np.random.RandomState(31)
    logits = 2.0 * rs.standard_normal((N, D))
    labels = rs.randint(0, D, size=N)
    held = 2.0 * rs.standard_normal((HELD, D))
    os.makedirs(OUT, exist_ok=True)

    def fit(double, seed, bs):
        del initial[:]
        torch.manual_seed(seed)
        return C.TorchFlowCalibrator(factory(double), logits, np.eye(D)[labels], epochs=EPOCHS,
                                     batch_size=bs, dev=torch.device("cpu"))

    for name, bs in (("full", N), ("mb128", 128)):
        steps = EPOCHS * -(-N // bs)
        quarter = steps * LR * 2e-2 / 4
        for seed in range(SEED0, SEED0 + 50):
            c64 = fit(True, seed, bs)
            P64 = _params(c64.flow.flow)
            cal = fit(False, seed, bs)
            P0 = initial[0]
            P = _params(cal.flow.flow)
            gap = np.abs(P - P64).max()
            if gap <= quarter:
                break
        assert gap <= quarter, (name, gap, quarter)
        hist = {k: np.array([float(v) for v in cal.history[k]], dtype=np.float32)
                for k in ("loss", "ce", "log_det")}
        pred = cal.predict(held)
        data = {"order": np.array(ORDER), "logits": logits, "labels": labels.astype(np.int64),
                "seed": np.int64(seed), "epochs": np.int64(EPOCHS), "batch_size": np.int64(bs),
                "P0": P0, "P": P, "P64": P64, "loss": hist["loss"], "ce": hist["ce"],
                "log_det": hist["log_det"], "held": held, "pred": pred}
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **data)
        assert os.path.getsize(path) < (1 << 20)
        print("%s: seed %d  fp32-f64 gap %.2e (quarter bar %.2e)  loss %s  log_det %s  %d bytes"
              % (name, seed, gap, quarter, hist["loss"], hist["log_det"], os.path.getsize(path)))


if __name__ == "__main__":
    main()
