"""Isotonic (pool-adjacent-violators) calibration: the reference's
PAVCalibrator, one isotonic regression per class on the class's softmax score.

The fit runs on the host: `host_fit` restates sklearn 1.7's isotonic fit in
float64 NumPy (sort, the absolute 1e-15 grouping of _make_unique, PAV on
integer (sum, count) blocks pooled on >=, the kept points), so it needs
neither sklearn nor the `np.float` alias the reference still uses.
`host_predict` is IsotonicRegression.predict with out_of_bounds='clip' (SciPy
interp1d's linear rule) and the row normalisation.

The prediction also runs on the device: `PavModel.from_host` uploads the
per-class points once and `predict(x, model, log_priors)` is ONE fused launch
(cnf_pav_predict, include/cnf.h) from fp32 logits on a ROCm device to fp32
calibrated probabilities there, ready for cnf_metrics.
"""
import ctypes

import numpy as np
import torch

from . import _lib, engine

MAX_ROWS = 1 << 26
EPS = 1e-15  # np.finfo(np.float64).resolution, sklearn's _make_unique tolerance

engine.stats.setdefault("pav_predict", 0)


def check_shape(D, B):
    if not 2 <= D <= _lib.MAX_DIM:
        raise ValueError("2 <= D <= %d, got %d" % (_lib.MAX_DIM, D))
    if B > MAX_ROWS:
        raise ValueError("at most 2^26 rows")


def _rows(x):
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 2):
        raise ValueError("x must be a [B, D] tensor on a ROCm device")
    x = x.detach().to(torch.float32).contiguous()
    check_shape(int(x.shape[1]), int(x.shape[0]))
    return x


class PavModel:
    """The fitted points of every class: device tensors thr_x, thr_y [D, cap]
    (cap = the largest count) and n_thr [D] for cnf_pav_predict, and the counts
    on the host."""

    def __init__(self, thr_x, thr_y, n_thr, counts):
        self.thr_x, self.thr_y, self.n_thr = thr_x, thr_y, n_thr
        self.counts = np.asarray(counts, dtype=np.int64)

    @classmethod
    def from_host(cls, points, device):
        """A model from per-class (x, y) host arrays (e.g. host_fit's)."""
        counts = [len(px) for px, _ in points]
        cap = max(1, max(counts))
        tx, ty = np.zeros((len(points), cap)), np.zeros((len(points), cap))
        for c, (px, py) in enumerate(points):
            tx[c, :len(px)], ty[c, :len(px)] = px, py
        return cls(torch.from_numpy(tx).to(device), torch.from_numpy(ty).to(device),
                   torch.tensor(counts, dtype=torch.int32, device=device), counts)


def predict(x, model, log_priors):
    """Calibrated fp32 probabilities of the ROCm fp32 tensor x [B, D] under
    `model`: one cnf_pav_predict launch.  log_priors: D host float64 values
    (one H2D copy) or a float64 device tensor."""
    x = _rows(x)
    B, D = int(x.shape[0]), int(x.shape[1])
    if model.thr_x.shape[0] != D:
        raise ValueError("the model has %d classes, x has %d" % (model.thr_x.shape[0], D))
    if torch.is_tensor(log_priors):
        lp = log_priors.to(device=x.device, dtype=torch.float64).reshape(-1).contiguous()
    else:
        lp = torch.from_numpy(np.ascontiguousarray(
            np.asarray(log_priors, dtype=np.float64).reshape(-1))).to(x.device)
    if lp.numel() != D:
        raise ValueError("log_priors must hold %d values" % D)
    tx, ty, nt = model.thr_x, model.thr_y, model.n_thr
    ops = engine._ops()
    if ops is not None:
        probs = ops.pav_predict(x, tx, ty, nt, lp)
        engine.stats["torch_ops"] += 1
    else:
        probs = torch.empty_like(x)
        with torch.cuda.device(x.device):
            st = _lib.lib().cnf_pav_predict(
                engine._ptr(x), ctypes.c_int32(D), ctypes.c_int64(B), engine._ptr(tx),
                engine._ptr(ty), engine._ptr(nt), ctypes.c_int32(tx.shape[1]), engine._ptr(lp),
                engine._ptr(probs), engine._stream(x.device))
        _lib.check("cnf_pav_predict", st)
    engine.stats["pav_predict"] += 1
    return probs


# ---- the same steps on the host, float64 NumPy --------------------------------
def group_starts(x):
    """Indices at which sklearn's _make_unique opens a group in the sorted
    array x: element 0, and every element with x - x_first_of_group >= 1e-15.
    Elements whose gap to their predecessor is >= 1e-15 open one for certain;
    only runs of smaller gaps need the walk, one binary search per step."""
    n = x.shape[0]
    start = np.ones(n, dtype=bool)
    start[1:] = x[1:] - x[:-1] >= EPS
    heads = np.flatnonzero(start[:-1] & ~start[1:])
    certain = start.copy()
    for s in heads:
        while True:
            # first j > s with x[j] - x[s] >= EPS (x is sorted, so this is monotone in j)
            lo, hi = s, n
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if x[mid] - x[s] >= EPS:
                    hi = mid
                else:
                    lo = mid
            if hi >= n or certain[hi]:
                break
            start[hi] = True
            s = hi
    return np.flatnonzero(start)


def _pav_blocks(sums, cnts):
    """PAV on (sum, count) groups, pooling while mean(top) >= mean(new),
    compared by cross-multiplication: exact for the integer sums of 0/1
    labels, float64 for soft targets.  Returns lists (sum, count, first group,
    last group) of the blocks."""
    S, C, F, L = [], [], [], []
    for g in range(len(sums)):
        s, c, f = sums[g].item(), int(cnts[g]), g
        while S and S[-1] * c >= s * C[-1]:
            s += S.pop()
            c += C.pop()
            f = F.pop()
            L.pop()
        S.append(s), C.append(c), F.append(f), L.append(g)
    return S, C, F, L


def host_fit_class(x, bit):
    """(X_thresholds_, y_thresholds_) of one class: x float64 scores, bit the
    targets of the class (0/1 labels are summed as integers; soft targets in
    float64)."""
    order = np.argsort(x, kind="stable")
    x, bit = x[order], np.asarray(bit)[order]
    bit = bit.astype(np.int64 if ((bit == 0) | (bit == 1)).all() else np.float64)
    starts = group_starts(x)
    sums = np.add.reduceat(bit, starts)
    cnts = np.diff(np.append(starts, x.shape[0]))
    S, C, F, L = _pav_blocks(sums, cnts)
    px, py = [], []
    for s, c, f, l in zip(S, C, F, L):
        v = s / c
        px.append(x[starts[f]]), py.append(v)
        if l != f:
            px.append(x[starts[l]]), py.append(v)
    return np.array(px, dtype=np.float64), np.array(py, dtype=np.float64)


def host_fit(probs, onehot):
    """Per-class points of float64 probs [B, D] against 0/1 targets [B, D]."""
    return [host_fit_class(np.ascontiguousarray(probs[:, c]), onehot[:, c])
            for c in range(probs.shape[1])]


def host_predict_class(px, py, s):
    """IsotonicRegression.predict with out_of_bounds='clip': SciPy interp1d's
    linear rule between the points, a constant for a single point."""
    if len(px) == 1:
        return np.full(s.shape, py[0])
    s = np.clip(s, px[0], px[-1])
    i = np.clip(np.searchsorted(px, s), 1, len(px) - 1)
    slope = (py[i] - py[i - 1]) / (px[i] - px[i - 1])
    return slope * (s - px[i - 1]) + py[i - 1]


def host_predict(points, probs):
    """The calibrated, row-normalised probabilities (PAVCalibrator.predict_post)."""
    out = np.zeros(probs.shape)
    for c, (px, py) in enumerate(points):
        out[:, c] = host_predict_class(px, py, probs[:, c])
    with np.errstate(invalid="ignore", divide="ignore"):
        out /= np.sum(out, axis=1, keepdims=True)
    return out
