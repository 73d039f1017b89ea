"""Float64 NumPy restatement of a planar calibrator's predict -- the reference's
Calibrator.predict around TorchFlowCalibrator.predict_post (calibrators.py:
40-44, 330-353) over a planar flow -- on top of tests/_planar_ref.forward:
  xc = x - mean(x);  z = planar stack(xc);  p = softmax(z)
  probs = softmax(log(p + 1e-7) - log_priors)
with SciPy's softmax restated (exp(q - max) / sum), so a -inf log-prior (q =
+inf, q - max = NaN) makes the whole row NaN, as SciPy's does.
tests/test_planar_predict_cpu.py holds it to the reference's float64 record
(tests/golden/planar_predict/*.npz); it is the oracle for shapes too large for
fixtures.
"""
import os

import numpy as np

import _planar_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {"one": "one", "d3": "d3", "d10": "d10", "d17": "d17", "d100": "d100", "nan": "nan",
            "inf": "d3"}   # predict fixture -> the planar fixture holding its parameters


def _softmax(q):
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(q - np.max(q, axis=1, keepdims=True))
        return e / np.sum(e, axis=1, keepdims=True)


def predict(params, x, log_priors):
    """(probs [B, D], ld [B] of the centred rows) in float64."""
    x = np.asarray(x, dtype=np.float64)
    xc = x - np.mean(x, axis=1, keepdims=True)
    zs, ld, _ = R.forward(params, xc)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = _softmax(zs[-1])
        q = np.log(p + 1e-7) - np.asarray(log_priors, dtype=np.float64)
    return _softmax(q), ld


def load(name):
    """The predict fixture's arrays plus W, U, Bv of its planar fixture."""
    d = dict(np.load(os.path.join(GOLDEN, "planar_predict", name + ".npz")))
    src = np.load(os.path.join(GOLDEN, "planar", FIXTURES[name] + ".npz"))
    for k in ("W", "U", "Bv"):
        d[k] = src[k]
    return d


def load_cal(name):
    return dict(np.load(os.path.join(GOLDEN, "planar_cal", name + ".npz")))
