"""Generate the radial calibrator fixtures (tests/golden/radial_cal/{full,mb128}.npz)
FROM THE REFERENCE ITSELF: its TorchFlowCalibrator (calibrators.py:239-353)
trained on the CPU around its Flow of four RadialLayers (flows/flows.py:8-25,
168-193), and its predict of held-out rows.

Test infrastructure only; runs on the CPU against a checkout of the reference,
whose directory is the script's one argument.  Nothing here is imported by the
product or by the tests: those read only the committed .npz files.  The
reference's calibrators.py still says `np.float`, which NumPy 2 dropped: this
generator sets `np.float = float` before it imports it.

The flow factory is local to this generator: the reference's Flow of four
RadialLayer(3) behind a module whose forward returns (zs[-1], log_det), as the
calibrator expects of its factory.  The recipe is that of
gen_golden_planar_cal.py: D = 3, N = 300, 5 epochs, torch.manual_seed(7) before
the constructor (layer initialisation and every DataLoader shuffle draw from
it); rows and labels from RandomState(31).  `full` trains with batch 300,
`mb128` with batch 128 (three batches per pass, the last of 44 rows).

Recorded: logits [N, D] float64 and labels [N], seed, epochs, batch_size,
Z00 [L, D], A0, Bv0 [L] (the parameters before the first step) and Z0, A, Bv
(after the last), the history lists loss / ce / log_det [epochs] (fp32; the
log-det history is zeros, the layer's log-det being the constant 0), held
[50, D] float64 and pred = predict(held) (float64).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_radial_cal.py REFERENCE_DIR
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else None
OUT = os.path.join(HERE, "radial_cal")
D, N, LAYERS, EPOCHS, SEED, HELD = 3, 300, 4, 5, 7, 50


def _reference():
    if REF is None or not os.path.isdir(REF):
        sys.exit("usage: gen_golden_radial_cal.py REFERENCE_DIR")
    sys.dont_write_bytecode = True
    np.float = float  # the alias NumPy 2 removed
    sys.path.insert(0, REF)
    import calibrators as C  # the reference's
    from flows import flows as RF
    return C, RF


def _params(flow):
    return (np.stack([ly.z0.detach().numpy().copy() for ly in flow.layers]),
            np.concatenate([ly.a.detach().numpy().copy() for ly in flow.layers]),
            np.concatenate([ly.b.detach().numpy().copy() for ly in flow.layers]))


def main():
    C, RF = _reference()
    initial = []

    class RadialFactory(torch.nn.Module):
        def __init__(self, dim, layers=LAYERS, **kwargs):
            super().__init__()
            self.flow = RF.Flow([RF.RadialLayer(dim) for _ in range(layers)])
            initial.append(_params(self.flow))

        def forward(self, x):
            zs, ld = self.flow(x)
            return zs[-1], ld

    rs = np.random.RandomState(31)
    logits = 2.0 * rs.standard_normal((N, D))
    labels = rs.randint(0, D, size=N)
    held = 2.0 * rs.standard_normal((HELD, D))
    os.makedirs(OUT, exist_ok=True)
    for name, bs in (("full", N), ("mb128", 128)):
        del initial[:]
        torch.manual_seed(SEED)
        cal = C.TorchFlowCalibrator(RadialFactory, logits, np.eye(D)[labels], layers=LAYERS,
                                    epochs=EPOCHS, batch_size=bs, dev=torch.device("cpu"))
        Z00, A0, Bv0 = initial[0]
        Z0, A, Bv = _params(cal.flow.flow)
        hist = {k: np.array([float(v) for v in cal.history[k]], dtype=np.float32)
                for k in ("loss", "ce", "log_det")}
        assert not hist["log_det"].any()
        pred = cal.predict(held)
        data = {"logits": logits, "labels": labels.astype(np.int64), "seed": np.int64(SEED),
                "epochs": np.int64(EPOCHS), "batch_size": np.int64(bs), "Z00": Z00, "A0": A0,
                "Bv0": Bv0, "Z0": Z0, "A": A, "Bv": Bv, "loss": hist["loss"], "ce": hist["ce"],
                "log_det": hist["log_det"], "held": held, "pred": pred}
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **data)
        assert os.path.getsize(path) < (1 << 20)
        print("%s: loss %s  moved %.3e  %d bytes" % (name, hist["loss"],
                                                      np.abs(Z0 - Z00).max(), os.path.getsize(path)))


if __name__ == "__main__":
    main()
