"""Generate the detection fixtures (tests/golden/detection/d*.npz) FROM THE
REFERENCE ITSELF: its utils/ops.py detection_log_likelihood_ratios and
utils/metrics.py empirical_cross_entropy, imported the way
gen_golden_metrics.py imports the reference.  ECE_plot's axis loop
(visualization.py:459-471: np.linspace, odds = 10**t, prior = odds / (1 + odds))
is restated here; visualization.py is not imported.

Test infrastructure only; runs in the build container, where the reference is
mounted read-only at /root/reference.  Nothing here is imported by the
product or by the tests: those read only the committed .npz files.  The
fixtures live in their own directory because tests/_golden.py lists every
.npz directly under tests/golden/ as a flow fixture.

Logits are gen_golden.synthetic_logits as fp32 (times `scale`, rounded to
fp32), widened to float64 for the reference.  Each fixture holds `x` fp32
[B, D], `y` int64 [B], `priors` float64 [D], the reference's `llr` [B, D], the
`axis` [P] of prior log10-odds, the per-class curves `curves` [D, P]
(ECE of np.exp(llr[:, c]) against y == c) and the flattened curve `flat` [P]
(all classes against the one-hot target):

  d1  D=3,   B=600,  uniform priors
  d2  D=10,  B=1031, Dirichlet priors
  d3  D=10,  B=1031, logits x 8 (row spread ~ 58: saturated ratios), Dirichlet
  d4  D=100, B=200,  labels arange % D shuffled (every class occurs), uniform
  d5  D=2,   B=65,   logits x 4, Dirichlet
  d6  D=3,   B=40,   class 2 never occurs: its curve is NaN (0 / 0)
  d7  the binary form: column 0 of d1's ratios against y == 0 at ONE prior
      (axis [0.5]); `llr` [B, 1], `t` the 0/1 target, `curves` [1, 1]

Every reference output other than d6's missing class is asserted finite.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_detection.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "detection")


def _reference():
    sys.dont_write_bytecode = True
    pkg_dir = os.path.join(REF, "utils")
    pkg = importlib.util.module_from_spec(importlib.util.spec_from_file_location(
        "ref_utils", os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir]))
    sys.modules["ref_utils"] = pkg
    pkg.__spec__.loader.exec_module(pkg)
    import ref_utils.metrics as M  # reference utils/metrics.py
    import ref_utils.ops as O      # reference utils/ops.py
    return M, O


def _curve(M, ratios, target, axis):
    """ECE_plot's loop (visualization.py:468-471)."""
    out = np.zeros(axis.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, logprior in enumerate(axis):
            odds = 10 ** logprior
            prior = odds / (1. + odds)
            out[i] = M.empirical_cross_entropy(ratios, target, prior)
    return out


def _write(M, O, name, x, y, priors, axis, missing=()):
    B, D = x.shape
    llr = O.detection_log_likelihood_ratios(x.astype(np.float64), priors)
    assert np.isfinite(llr).all()
    onehot = np.zeros((B, D))
    onehot[np.arange(B), y] = 1
    ratios = np.exp(llr)
    curves = np.stack([_curve(M, ratios[:, c], (y == c).astype(np.float64), axis)
                       for c in range(D)])
    flat = _curve(M, ratios.ravel(), onehot.ravel(), axis)
    for c in range(D):
        assert np.isnan(curves[c]).all() if c in missing else np.isfinite(curves[c]).all()
    assert np.isfinite(flat).all()
    _save(name, x=x, y=y.astype(np.int64), priors=priors, llr=llr, axis=axis, curves=curves,
          flat=flat)


def _save(name, **arrays):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("%s: %s (%d bytes)" % (name, " ".join("%s%s" % (k, list(np.shape(v)))
                                                for k, v in arrays.items()),
                                 os.path.getsize(path)))


def _logits(B, D, seed, scale=1.0):
    sys.path.insert(0, HERE)
    from gen_golden import synthetic_logits
    x, y = synthetic_logits(B, D, seed)
    return (x * np.float32(scale)).astype(np.float32), y


def main():
    M, O = _reference()
    rs = np.random.RandomState(20261019)
    axis = np.linspace(-2.5, 2.5, num=100)
    x1, y1 = _logits(600, 3, 21)
    _write(M, O, "d1", x1, y1, np.full(3, 1. / 3), axis)
    x, y = _logits(1031, 10, 22)
    _write(M, O, "d2", x, y, rs.dirichlet(np.full(10, 5.0)), axis)
    x, y = _logits(1031, 10, 23, scale=8.0)
    _write(M, O, "d3", x, y, rs.dirichlet(np.full(10, 5.0)), axis)
    x, _ = _logits(200, 100, 24)
    y = rs.permutation(np.arange(200) % 100)
    _write(M, O, "d4", x, y, np.full(100, 1. / 100), axis)
    x, y = _logits(65, 2, 25, scale=4.0)
    _write(M, O, "d5", x, y, rs.dirichlet(np.full(2, 5.0)), axis)
    x, y = _logits(40, 3, 26)
    y = y % 2  # class 2 never occurs
    _write(M, O, "d6", x, y, np.full(3, 1. / 3), axis, missing=(2,))
    # d7: the binary form at one prior
    llr1 = O.detection_log_likelihood_ratios(x1.astype(np.float64), np.full(3, 1. / 3))
    t = (y1 == 0).astype(np.float64)
    one = np.array([0.5])
    c = _curve(M, np.exp(llr1[:, 0]), t, one)
    assert np.isfinite(c).all()
    _save("d7", x=x1, y=y1.astype(np.int64), priors=np.full(3, 1. / 3), llr=llr1[:, :1],
          t=t.astype(np.int64), axis=one, curves=c.reshape(1, 1), flat=c)


if __name__ == "__main__":
    main()
