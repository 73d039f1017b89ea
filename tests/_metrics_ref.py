"""float64 NumPy restatement of the reference's scoring (utils/metrics.py:6-15,
35-80) for label-vector targets, which also returns the per-bin counts,
confidence sums and correct counts the device record is compared with.  Test
infrastructure only: the product's own host path is utils/metrics.py of the
drop-in tree."""
import os

import numpy as np

METRICS_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics")
FIXTURES = ("m1", "m2", "m3", "m4")
FX = 4294967296.0


def load(name):
    f = np.load(os.path.join(METRICS_GOLDEN, name + ".npz"))
    return {k: f[k] for k in f.files}


def softmax_rows(B, D, seed):
    """Seeded fp32 probability rows with labels (peaked on the label)."""
    rs = np.random.RandomState(seed)
    y = rs.randint(0, D, size=B).astype(np.int64)
    x = rs.standard_normal((B, D))
    x[np.arange(B), y] += 2.0
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32), y


def score(probs, y, bins=15):
    """probs [B, D] (any float dtype; widened to float64 as Calibrator.predict
    does), y [B] labels in [0, D).  Returns a dict of float64 / int64 values."""
    p = np.asarray(probs).astype(np.float64)
    y = np.asarray(y).astype(np.int64)
    B = p.shape[0]
    rows = np.arange(B)
    # metrics.py:12-15: mean(-sum(onehot * log(p + 1e-7), axis=1)) = the label's term
    terms = -np.log(p[rows, y] + 1e-7)
    preds = np.argmax(p, axis=1)            # metrics.py:46, 80 (first maximum)
    conf = p[rows, preds]                   # metrics.py:49
    hits = preds == y                       # metrics.py:54, 80
    width = 1. / bins                       # metrics.py:57
    count = np.zeros(bins, dtype=np.int64)
    correct = np.zeros(bins, dtype=np.int64)
    conf_sum = np.zeros(bins, dtype=np.float64)
    conf_fx = np.zeros(bins, dtype=np.int64)
    ece = 0.
    for i in range(bins):                   # metrics.py:60-69
        low, high = i * width, (i + 1) * width
        sel = (low < conf) & (conf <= high)
        n = int(sel.sum())
        count[i] = n
        correct[i] = int(hits[sel].sum())
        conf_sum[i] = conf[sel].sum()
        conf_fx[i] = int(np.rint(conf[sel] * FX).astype(np.int64).sum())
        if n:
            ece += abs(np.mean(hits[sel].astype(np.float64)) - np.mean(conf[sel])) * n
    return {"n": B, "nll": float(np.mean(terms)), "nll_terms": terms,
            "acc": float(np.mean(hits)), "n_correct": int(hits.sum()),
            "ece": float(ece / B),          # metrics.py:71
            "count": count, "correct": correct, "conf_sum": conf_sum, "conf_fx": conf_fx}


def check_record_counts(rec, ref, bins):
    """Words [0, 1, 3], both per-bin count arrays and conf_fx equal the
    restatement exactly."""
    rec = np.asarray(rec).astype(np.int64)
    assert rec.shape == (4 + 3 * bins,)
    assert rec[0] == ref["n"] and rec[1] == 0 and rec[3] == ref["n_correct"]
    np.testing.assert_array_equal(rec[4:4 + bins], ref["count"])
    np.testing.assert_array_equal(rec[4 + bins:4 + 2 * bins], ref["conf_fx"])
    np.testing.assert_array_equal(rec[4 + 2 * bins:4 + 3 * bins], ref["correct"])
