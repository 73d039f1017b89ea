"""Generate the scoring fixtures (tests/golden/metrics/m*.npz) FROM THE
REFERENCE ITSELF: its utils/metrics.py (neg_log_likelihood,
expected_calibration_error, accuracy) applied to `probs.astype(float64)`,
which is what Calibrator.predict hands users.

Test infrastructure only; runs in the build container, where the reference is
mounted read-only at /root/reference.  Nothing here is imported by the
product or by the tests: those read only the committed .npz files.

NumPy 2 rejects one call of the reference, metrics.py:54
`np.equal(preds, target, dtype=np.float32)` (TypeError: no loop for that
signature).  For that call alone the reference module is given a NumPy proxy
whose `equal(a, b, dtype)` is `np.equal(a, b).astype(dtype)` -- the 0/1 hits
as fp32, which is what the call produced on NumPy 1; every other attribute is
NumPy's own.

The fixtures live in their own directory because tests/_golden.py lists every
.npz directly under tests/golden/ as a flow fixture.

Each fixture holds fp32 `probs` [B, D], int64 `y` [B], `bins`, and the
reference's `ece`, `nll`, `acc` (targets handed over as one-hot rows of width
D, so a label the batch never draws cannot change the width):

  m1  D=10, bins=15: 4,099 softmax rows of synthetic_logits (gen_golden.py),
      then for every edge i/15 (i = 1..15) rows whose confidence is fp32(edge)
      and its fp32 neighbours (<= 1), the other columns small so the maximum
      is unambiguous, then two all-equal rows (argmax ties)
  m2  D=100, B=257, bins=15
  m3  D=3, B=600, bins=10
  m4  D=2, B=65, bins=1

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_metrics.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "metrics")


class _NumpyProxy:
    """NumPy, except equal(a, b, dtype) = np.equal(a, b).astype(dtype)."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def equal(a, b, dtype=None):
        r = np.equal(a, b)
        return r if dtype is None else r.astype(dtype)


def _reference_metrics():
    sys.dont_write_bytecode = True
    pkg_dir = os.path.join(REF, "utils")
    pkg = importlib.util.module_from_spec(importlib.util.spec_from_file_location(
        "ref_utils", os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir]))
    sys.modules["ref_utils"] = pkg
    pkg.__spec__.loader.exec_module(pkg)
    import ref_utils.metrics as M  # reference utils/metrics.py
    M.np = _NumpyProxy()
    return M


def _softmax_rows(B, D, seed):
    sys.path.insert(0, HERE)
    from gen_golden import synthetic_logits
    x, y = synthetic_logits(B, D, seed)
    x = x.astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32), y


def _edge_rows(D, bins, rs):
    """Rows whose maximum is fp32(edge) or an fp32 neighbour of it."""
    rows, labels = [], []
    for i in range(1, bins + 1):
        e = np.float32(i * (1. / bins))
        for conf in (np.nextafter(e, np.float32(0)), e, np.nextafter(e, np.float32(2))):
            if conf > 1:
                continue
            row = (rs.uniform(0, 0.01, size=D)).astype(np.float32)
            col = int(rs.randint(0, D))
            row[col] = conf
            rows.append(row)
            labels.append(col if rs.randint(0, 2) else int(rs.randint(0, D)))
    return np.stack(rows), np.array(labels, dtype=np.int64)


def _write(M, name, probs, y, bins):
    D = probs.shape[1]
    p64 = probs.astype(np.float64)
    onehot = np.zeros(probs.shape)
    onehot[np.arange(len(y)), y] = 1
    out = {"probs": probs, "y": y.astype(np.int64), "bins": np.int64(bins),
           "ece": np.float64(M.expected_calibration_error(p64, onehot, bins=bins)),
           "nll": np.float64(M.neg_log_likelihood(p64, onehot)),
           "acc": np.float64(M.accuracy(p64, onehot))}
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print("%s: B=%d D=%d bins=%d ece=%.9f nll=%.9f acc=%.6f (%d bytes)"
          % (name, probs.shape[0], D, bins, out["ece"], out["nll"], out["acc"],
             os.path.getsize(path)))


def main():
    M = _reference_metrics()
    rs = np.random.RandomState(20261019)
    probs, y = _softmax_rows(4099, 10, 11)
    ep, ey = _edge_rows(10, 15, rs)
    ties = np.stack([np.full(10, 0.1, np.float32), np.full(10, 0.25, np.float32)])
    _write(M, "m1", np.concatenate([probs, ep, ties]),
           np.concatenate([y, ey, np.array([0, 3], dtype=np.int64)]), 15)
    _write(M, "m2", *_softmax_rows(257, 100, 12), 15)
    _write(M, "m3", *_softmax_rows(600, 3, 13), 10)
    _write(M, "m4", *_softmax_rows(65, 2, 14), 1)


if __name__ == "__main__":
    main()
