"""Shared by the detection tests: the fixtures of tests/golden/detection
(written by gen_golden_detection.py from the reference's own functions) and
the two bounds of the comparison.

LLR:    |got - ref| <= 4 (D + 8) 2^-52 (1 + |ref|): both sides sum D positive
        terms of relative error a few 2^-53, differences of fp32-valued
        doubles are exact; the factor 4 is in hand.
Curves: |got - ref| <= 1e-13 (1 + |ref|): the reference's `1 + post` rounding
        costs <= 2^-53 / ln 2 per term, the weights sum to <= 1, and the sum
        over <= 1031 rows adds a few ulps.
"""
import os

import numpy as np

FIXTURES = ["d1", "d2", "d3", "d4", "d5", "d6", "d7"]
MULTI = ["d1", "d2", "d3", "d4", "d5", "d6"]  # [B, D] fixtures (d7: the binary form)
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detection")


def load(name):
    with np.load(os.path.join(DIR, name + ".npz")) as f:
        return {k: f[k] for k in f.files}


def llr_tol(ref, D):
    return 4 * (D + 8) * 2.0 ** -52 * (1 + np.abs(ref))


def curve_tol(ref):
    return 1e-13 * (1 + np.abs(ref))


def close(got, want, tol):
    """NaN positions agree; equal infinities agree; everything else within
    tol (elementwise).  Returns the largest |got - want| / tol met."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert (np.isnan(got) == np.isnan(want)).all()
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), want.shape)
    ok = ~np.isnan(want) & (got != want)
    assert np.isfinite(got[ok]).all() and np.isfinite(want[ok]).all()
    ratio = np.max(np.abs(got[ok] - want[ok]) / tol[ok], initial=0.0)
    assert ratio <= 1.0, "error / bound = %.3g" % ratio
    return float(ratio)


def edge_case():
    l = np.zeros((6, 3))
    y = np.array([0, 1, 2, 0, 1, 2])
    l[0, 0] = np.inf    # a positive of column 0 at LR = inf: log2(1 + 1 / inf) = 0
    l[1, 0] = np.inf    # a negative of column 0 at LR = inf: log2(1 + inf) = inf
    l[2, 1] = np.nan    # a negative of column 1
    l[4, 2] = -np.inf   # a negative of column 2 at LR = 0: log2(1 + 0) = 0
    l[3, 2] = 0.5       # so that no sum of column 2 is trivially zero
    return l, y, np.array([-1.0, 0.0, 2.0])


def check_edge_sums(sums):
    l, y, axis = edge_case()
    theta = np.log(np.array([10 ** v for v in axis]))
    assert (sums[0, 1] == np.inf).all()
    want = np.log1p(np.exp(-theta)) / np.log(2)          # rows 0 (a zero term) and 3 (LR = 1)
    close(sums[0, 0], want, 1e-13 * (1 + want))
    assert np.isnan(sums[1, 1]).all() and np.isfinite(sums[1, 0]).all()
    assert np.isfinite(sums[2]).all() and (sums[2] > 0).all()
    # column 2's negatives: rows 0, 1 (LR = 1), 3 (ln LR = 0.5), 4 (a zero term)
    want = (2 * np.log1p(np.exp(theta)) + np.log1p(np.exp(theta + 0.5))) / np.log(2)
    close(sums[2, 1], want, 1e-13 * (1 + want))
