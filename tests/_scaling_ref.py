"""Float64 NumPy restatement of cnf_scaling_loss_grad / cnf_scaling_predict
(include/cnf.h) shared by tests/test_scaling_cpu.py and
tests/test_gpu_scaling.py: the raw sums, the sum of |terms| behind every
output word (the error scale of the evaluation tolerance), the reference's
`fun` / `jac` formed from the sums for each calibrator class, and
Calibrator.predict of a scaling map."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scaling")
FIXTURES = ("s1", "s2", "s3")
SCALAR, DIAG, FULL = 0, 1, 2
CLASSES = ("temp", "mlr", "vec", "mat")
KIND = {"temp": SCALAR, "mlr": SCALAR, "vec": DIAG, "mat": FULL}
# A float64 sum of B terms in any order is off by at most B * 2^-53 * sum|terms|;
# 1-2 ulp exp / log add a few 1e-16 per term: under 5e-13 * sum|terms| for
# B <= 4,099.  Every evaluation comparison is held to EVAL_TOL * sum|terms|.
EVAL_TOL = 1e-11


def load(name):
    f = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    if name == "s3":
        f.update(np.load(os.path.join(GOLDEN, "s3m.npz")))
    return f


def a_len(kind, D):
    return 1 if kind == SCALAR else D if kind == DIAG else D * D


def words(kind, D):
    return 1 + D + a_len(kind, D)


def softmax(t):
    e = np.exp(t - np.max(t, axis=1, keepdims=True))
    return e / np.sum(e, axis=1, keepdims=True)


def logits_map(x, kind, a, b):
    x = np.asarray(x, dtype=np.float64)
    D = x.shape[1]
    a = np.asarray(a, dtype=np.float64)
    bias = 0. if b is None else np.asarray(b, dtype=np.float64).reshape(D)
    if kind == SCALAR:
        return a.reshape(()) * x + bias
    if kind == DIAG:
        return a.reshape(D) * x + bias
    return x @ a.reshape(D, D) + bias


def sums(x, y, kind, a, b=None):
    """(sums, scale): the words of cnf_scaling_loss_grad with want_grad, and
    per word the sum of the absolute values of its terms."""
    x = np.asarray(x, dtype=np.float64)
    B, D = x.shape
    p = softmax(logits_map(x, kind, a, b))
    terms = -np.log(p[np.arange(B), y] + 1e-7)
    g = p.copy()
    g[np.arange(B), y] -= 1.0
    if kind == SCALAR:
        ga, sa = np.array([np.sum(g * x)]), np.array([np.sum(np.abs(g * x))])
    elif kind == DIAG:
        ga, sa = np.sum(g * x, axis=0), np.sum(np.abs(g * x), axis=0)
    else:
        ga, sa = (x.T @ g).ravel(), (np.abs(x).T @ np.abs(g)).ravel()
    s = np.concatenate([[np.sum(terms)], np.sum(g, axis=0), ga])
    scale = np.concatenate([[np.sum(np.abs(terms))], np.sum(np.abs(g), axis=0), sa])
    return s, scale


def assert_close(got, want, scale, B, what=""):
    """|got - want| <= EVAL_TOL * sum|terms| per word (B > 4,099: the bound
    B * 2^-53 grows with the rows, the twenty-fold slack stays)."""
    tol = max(EVAL_TOL, 20 * (B * 2.0 ** -53 + 4e-16)) * scale
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    bad = ~(err <= tol)
    assert not bad.any(), (what, int(bad.sum()), float(np.nanmax(err / np.maximum(scale, 1e-300))))


def forms(name, sums_fn, B, D):
    """(fun(x), jac(x), fun_scale(x), jac_scale(x)) of class `name` in the
    reference's own packing and formulas, from sums_fn(kind, a, b) ->
    (sums, scale).  The *_scale functions give the error scale of every
    returned number."""
    kind = KIND[name]

    def both(x, grad):
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        if name == "temp":
            T = x[0]
            s, sc = sums_fn(kind, [1. / T], None)
            return (s[0] / B, sc[0] / B) if not grad else \
                (np.array([-(s[1 + D] / B) / T ** 2]), np.array([sc[1 + D] / B / T ** 2]))
        if name == "mlr":
            s, sc = sums_fn(kind, x[:1], x[1:])
            return (s[0] / B, sc[0] / B) if not grad else \
                (np.concatenate([s[1 + D:], s[1:1 + D]]) / B,
                 np.concatenate([sc[1 + D:], sc[1:1 + D]]) / B)
        if name == "vec":
            s, sc = sums_fn(kind, x[D:], x[:D])
            if not grad:
                return s[0] / B, sc[0] / B
            db, dbs = np.sum(s[1:1 + D]) / (B * D), np.sum(sc[1:1 + D]) / (B * D)
            return (np.concatenate([np.full(D, db), s[1 + D:] / B]),
                    np.concatenate([np.full(D, dbs), sc[1 + D:] / B]))
        if not grad:  # matrix: the objective evaluates x @ (W + b)
            s, sc = sums_fn(kind, (x[D:].reshape(D, D) + x[:D]).ravel(), np.zeros(D))
            return s[0] / B, sc[0] / B
        s, sc = sums_fn(kind, x[D:], x[:D])
        return s[1:] / B, sc[1:] / B

    return (lambda x: both(x, False)[0], lambda x: both(x, True)[0],
            lambda x: both(x, False)[1], lambda x: both(x, True)[1])


def unpack(name, x, D):
    """(a, b) of cnf_scaling_predict from a class's fitted SciPy vector."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if name == "temp":
        return [1. / x[0]], None
    if name == "mlr":
        return x[:1], x[1:]
    return x[D:], x[:D]


def predict(x, kind, a, b, log_priors):
    """Calibrator.predict (calibrators.py:40-44) of the map, in float64."""
    x = np.asarray(x, dtype=np.float64)
    x = x - np.mean(x, axis=1, keepdims=True)
    p = softmax(logits_map(x, kind, a, b))
    return softmax(np.log(p + 1e-7) - np.asarray(log_priors, dtype=np.float64))


def log_priors(y, D):
    c = np.bincount(y, minlength=D).astype(np.float64)
    return np.log(c / c.sum())


def random_case(kind, D, B, seed, bias=True):
    """Seeded fp32 logits, labels and parameters of moderate size."""
    rs = np.random.RandomState(seed)
    y = rs.randint(0, D, size=B).astype(np.int64)
    x = rs.standard_normal((B, D))
    x[np.arange(B), y] += 2.0
    x = (1.8 * x).astype(np.float32)
    if kind == SCALAR:
        a = np.array([0.7])
    elif kind == DIAG:
        a = 0.7 + 0.2 * rs.standard_normal(D)
    else:
        a = (0.7 * np.eye(D) + 0.3 / np.sqrt(D) * rs.standard_normal((D, D))).ravel()
    b = 0.3 * rs.standard_normal(D) if (bias or kind != SCALAR) else None
    return x, y, a, b
