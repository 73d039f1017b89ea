"""Float64 NumPy restatement of the isotonic calibrator (cnf_hip/pav.py's host
fit and cnf_pav_predict, include/cnf.h; the reference's PAVCalibrator over
sklearn 1.7's IsotonicRegression) shared by tests/test_pav_cpu.py and
tests/test_gpu_pav.py: sort, the absolute 1e-15 grouping of _make_unique,
PAV on integer (sum, count) blocks pooled on >= -- chunk-local stacks followed
by a merge of the chunk stacks, so the chunk count can be swept -- the kept
points, and predict with SciPy interp1d's linear rule.  `load()` reads the
fixtures tests/golden/pav/*.npz written by gen_golden_pav.py."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pav")
FIXTURES = ("ties", "mod", "sat", "degen", "one")
MODERATE = ("ties", "mod")
EPS = 1e-15


def load(name):
    f = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    D = f["x"].shape[1]
    off = np.concatenate([[0], np.cumsum(f["n_thr"])])
    f["thr"] = [(f["thr_x"][off[c]:off[c + 1]], f["thr_y"][off[c]:off[c + 1]]) for c in range(D)]
    return f


def softmax(t):
    e = np.exp(t - np.max(t, axis=1, keepdims=True))
    return e / np.sum(e, axis=1, keepdims=True)


def scores(x):
    """softmax of the centred rows, float64 [B, D]."""
    x = np.asarray(x, dtype=np.float64)
    return softmax(x - np.mean(x, axis=1, keepdims=True))


def group_starts(x):
    """The plain left-to-right walk of sklearn's _make_unique on sorted x."""
    starts, first = [0], x[0]
    for i in range(1, x.shape[0]):
        if x[i] - first >= EPS:
            starts.append(i)
            first = x[i]
    return np.array(starts)


def _push(st, b):
    while st and st[-1][0] * b[1] >= b[0] * st[-1][1]:  # mean(top) >= mean(b)
        t = st.pop()
        b = (b[0] + t[0], b[1] + t[1], t[2], b[3])
    st.append(b)


def pav_blocks(sums, cnts, chunks=1):
    """Blocks (sum, count, first group, last group): PAV inside each of
    `chunks` contiguous ranges of groups, then the chunk stacks merged in
    order with the same rule."""
    n = len(sums)
    edges = np.linspace(0, n, chunks + 1).astype(int)
    stacks = []
    for k in range(chunks):
        st = []
        for g in range(edges[k], edges[k + 1]):
            _push(st, (int(sums[g]), int(cnts[g]), g, g))
        stacks.append(st)
    out = []
    for st in stacks:
        for b in st:
            _push(out, b)
    return out


def fit_class(x, bit, chunks=1):
    """(thr_x, thr_y) of one class from float64 scores x and 0/1 labels bit."""
    order = np.argsort(x, kind="stable")
    x, bit = np.asarray(x)[order], np.asarray(bit)[order].astype(np.int64)
    starts = group_starts(x)
    sums = np.add.reduceat(bit, starts)
    cnts = np.diff(np.append(starts, x.shape[0]))
    px, py = [], []
    for s, c, f, l in pav_blocks(sums, cnts, chunks):
        px.append(x[starts[f]]), py.append(s / c)
        if l != f:
            px.append(x[starts[l]]), py.append(s / c)
    return np.array(px), np.array(py)


def fit(sc, y, chunks=1):
    """Per-class points from scores [B, D] and labels y [B]."""
    return [fit_class(sc[:, c], y == c, chunks) for c in range(sc.shape[1])]


def predict_class(px, py, s):
    if len(px) == 1:
        return np.full(s.shape, py[0])
    s = np.clip(s, px[0], px[-1])
    i = np.clip(np.searchsorted(px, s), 1, len(px) - 1)
    return (py[i] - py[i - 1]) / (px[i] - px[i - 1]) * (s - px[i - 1]) + py[i - 1]


def predict(points, x, log_priors):
    """PAVCalibrator.predict of fp32 / float64 logits x, in float64."""
    sc = scores(x)
    p = np.stack([predict_class(px, py, sc[:, c]) for c, (px, py) in enumerate(points)], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = p / np.sum(p, axis=1, keepdims=True)
        return softmax(np.log(p + 1e-7) - np.asarray(log_priors, dtype=np.float64))


def log_priors(y, D):
    c = np.bincount(y, minlength=D).astype(np.float64)
    with np.errstate(divide="ignore"):
        return np.log(c / c.sum())


def ulps(a, b):
    """Distance of two float64 arrays in units in the last place."""
    a = np.asarray(a, dtype=np.float64).view(np.int64)
    b = np.asarray(b, dtype=np.float64).view(np.int64)
    return np.abs(a - b)
