"""Float64 NumPy restatement of the radial flow (the reference's RadialLayer,
flows/flows.py:168-193, stacked by Flow.forward), of its hand-derived reverse
mode and of a radial calibrator's predict -- the formulas the kernels of
csrc/cnf_radial.hip implement.  tests/test_radial_cpu.py holds it to the
reference's float64 autograd gradients recorded in tests/golden/radial/*.npz;
it is the oracle for shapes too large for fixtures.

Per layer, with z0 [D], a [1], b [1]:
  sp = log1p(exp(b));  beta = sp - a
  d = x - z0;  r = ||d||;  h = 1 / (a + r);  z = x + beta h d;  log-det = 0
and for the upstream g = dL/dz, s = g.d per row:
  g_beta = sum h s;  g_r = -h^2 beta s;  g_d = beta h g + (g_r / r) d  (0 at r == 0)
  dL/dx = g + g_d;  dL/dz0 = -sum g_d;  dL/da = sum g_r - g_beta;  dL/db = g_beta sigmoid(b)

Parameters: a list of (z0 [D], a [1], b [1]) per layer.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRAD_FIXTURES = ["one", "d3", "d10", "d10n", "d17", "d100", "tape", "neg", "zero"]
FIXTURES = GRAD_FIXTURES + ["sing"]


def _scalar(v):
    return float(np.asarray(v, dtype=np.float64).reshape(-1)[0])


def forward(params, x):
    """(zs [L, B, D], rs [L, B]) in float64."""
    x = np.asarray(x, dtype=np.float64)
    zs, rs = [], []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for z0, a, b in params:
            a, b = _scalar(a), _scalar(b)
            beta = -a + np.log1p(np.exp(b))
            d = x - np.asarray(z0, dtype=np.float64)[None, :]
            r = np.sqrt(np.sum(d * d, axis=1))
            h = 1.0 / (a + r)
            x = x + (beta * h)[:, None] * d
            zs.append(x)
            rs.append(r)
    return np.stack(zs), np.stack(rs)


def _log_softmax(z):
    m = z.max(axis=1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=1, keepdims=True))


def loss_terms(z, y, kind):
    """(sum of per-row loss, sum of ce, 0), and the seed g [B, D] of the sum
    of the per-row loss (the log-det is 0: loss == ce)."""
    B, D = z.shape
    lp = _log_softmax(z)
    p = np.exp(lp)
    oh = np.eye(D)[y]
    lpy = lp[np.arange(B), y]
    if kind == "cal":
        py = np.exp(lpy)
        ce = -np.log(py + 1e-7)
        g = (py / (py + 1e-7))[:, None] * (p - oh)
    else:
        ce = -lpy
        g = p - oh
    return (ce.sum(), ce.sum(), 0.0), g


def vjp(params, x, gz=None, gz_all=None):
    """Hand reverse mode: (flat gradient in state_dict order -- z0, a, b per
    layer --, dx [B, D]) for upstream gradients of the final z and of every
    layer's output (None = zero)."""
    x = np.asarray(x, dtype=np.float64)
    B, D = x.shape
    L = len(params)
    zs, rs = forward(params, x)
    g = np.zeros((B, D))
    if gz is not None:
        g = g + np.asarray(gz, dtype=np.float64)
    if gz_all is not None:
        g = g + np.asarray(gz_all[L - 1], dtype=np.float64)
    out = [None] * L
    for l in range(L - 1, -1, -1):
        z0 = np.asarray(params[l][0], dtype=np.float64)
        a, b = _scalar(params[l][1]), _scalar(params[l][2])
        beta = -a + np.log1p(np.exp(b))
        x_l = zs[l - 1] if l > 0 else x
        d = x_l - z0[None, :]
        r = rs[l]
        h = 1.0 / (a + r)
        s = np.sum(g * d, axis=1)
        g_beta = float(np.sum(h * s))
        g_r = -h * h * beta * s
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(r != 0.0, g_r / r, 0.0)
        g_d = (beta * h)[:, None] * g + q[:, None] * d
        g = g + g_d
        if l > 0 and gz_all is not None:
            g = g + np.asarray(gz_all[l - 1], dtype=np.float64)
        sig = 1.0 / (1.0 + np.exp(-b))
        out[l] = np.concatenate([-g_d.sum(axis=0), [float(np.sum(g_r)) - g_beta], [g_beta * sig]])
    return np.concatenate(out), g


def loss_vjp(params, x, y, kind, grad_scale=1.0):
    """(terms, flat gradient of grad_scale * sum of the per-row loss, dx)."""
    zs, _ = forward(params, x)
    terms, g = loss_terms(zs[-1], np.asarray(y), kind)
    grads, dx = vjp(params, x, gz=g * grad_scale)
    return np.array(terms), grads, dx


def _softmax(q):
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(q - np.max(q, axis=1, keepdims=True))
        return e / np.sum(e, axis=1, keepdims=True)


def predict(params, x, log_priors):
    """Calibrator.predict around a radial flow, float64: probs [B, D]."""
    x = np.asarray(x, dtype=np.float64)
    xc = x - np.mean(x, axis=1, keepdims=True)
    zs, _ = forward(params, xc)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.log(_softmax(zs[-1]) + 1e-7) - np.asarray(log_priors, dtype=np.float64)
    return _softmax(q)


# ---- fixtures (tests/golden/radial, written by tests/golden/gen_golden_radial.py)

def load(name):
    """The fixture's arrays, the float64 outputs of <name>_f64.npz included."""
    root = os.path.join(GOLDEN, "radial")
    d = dict(np.load(os.path.join(root, name + ".npz")))
    d.update(np.load(os.path.join(root, name + "_f64.npz")))
    return d


def load_cal(name):
    return dict(np.load(os.path.join(GOLDEN, "radial_cal", name + ".npz")))


def params_of(d):
    return [(d["Z0"][l], d["A"][l:l + 1], d["Bv"][l:l + 1]) for l in range(d["Z0"].shape[0])]


def build_flow(d, device="cpu", factory=False):
    """The package's Flow of RadialLayers (RadialFlow when `factory`) holding
    the fixture's parameters."""
    import torch
    from flows.flows import Flow, RadialLayer
    L, D = d["Z0"].shape
    if factory:
        from flows._factory import RadialFlow
        flow = RadialFlow(D, layers=L)
    else:
        flow = Flow([RadialLayer(D) for _ in range(L)])
    with torch.no_grad():
        for l, ly in enumerate(flow.layers):
            ly.z0.copy_(torch.from_numpy(d["Z0"][l]))
            ly.a.copy_(torch.from_numpy(d["A"][l:l + 1]))
            ly.b.copy_(torch.from_numpy(d["Bv"][l:l + 1]))
    return flow.to(device)


def bar(floor, tol=1e-5):
    """The project's rule (tests/test_gpu_parity.py): the tolerance, or twice
    the reference's own fp32-vs-float64 error where that is larger."""
    return max(tol, 2.0 * float(floor))
