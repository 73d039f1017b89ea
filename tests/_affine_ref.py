"""Float64 NumPy restatement of the affine-constant flow (the reference's
AffineConstantLayer, flows/flows.py:40-65, stacked by Flow.forward /
Flow.backward), of its hand-derived reverse mode and of an affine calibrator's
predict -- the formulas the kernels of csrc/cnf_affine.hip implement.
tests/test_affine_cpu.py holds it to the reference's float64 values recorded in
tests/golden/affine/*.npz; it is the oracle for shapes too large for fixtures.

Per layer, with s [D], t [D]:
  forward  z = x exp(s) + t,    log-det = sum_d s      (one number for the batch)
  inverse  x = (z - t) exp(-s), log-det = -sum_d s
and for the upstream G = dL/dz and gld = dL/d(log-det):
  grad t = sum_rows G;  grad s = sum_rows G x exp(s) + gld;  dL/dx = G exp(s)

Parameters: a list of (s [D], t [D]) per layer.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["one", "d3", "d10", "init", "d17", "d100", "tape", "contract", "centre"]


def _f64(v):
    return np.asarray(v, dtype=np.float64).reshape(-1)


def forward(params, x):
    """(zs [L, B, D], log-det) in float64."""
    x = np.asarray(x, dtype=np.float64)
    zs, ld = [], 0.0
    for s, t in params:
        s, t = _f64(s), _f64(t)
        x = x * np.exp(s)[None, :] + t[None, :]
        zs.append(x)
        ld = ld + float(np.sum(s))
    return np.stack(zs), ld


def inverse(params, z):
    """Flow.backward: (xs [L, B, D] with xs[k] the rows after undoing layer
    L-1-k, log-det) in float64."""
    z = np.asarray(z, dtype=np.float64)
    xs, ld = [], 0.0
    for s, t in reversed(params):
        s, t = _f64(s), _f64(t)
        z = (z - t[None, :]) * np.exp(-s)[None, :]
        xs.append(z)
        ld = ld + float(np.sum(-s))
    return np.stack(xs), ld


def _log_softmax(z):
    m = z.max(axis=1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=1, keepdims=True))


def loss_terms(z, ld, y, kind, det=1.0):
    """((sum of per-row loss, sum of ce, B * ld), the seed g [B, D] of the sum
    of the per-row loss, the log-det's weight w: loss = ce - w * ld)."""
    B, D = z.shape
    lp = _log_softmax(z)
    p = np.exp(lp)
    oh = np.eye(D)[y]
    lpy = lp[np.arange(B), y]
    if kind == "cal":
        py = np.exp(lpy)
        ce = -np.log(py + 1e-7)
        g = (py / (py + 1e-7))[:, None] * (p - oh)
        w = 1.0
    else:
        ce = -lpy
        g = p - oh
        w = float(det)
    return (ce.sum() - w * B * ld, ce.sum(), B * ld), g, w


def vjp(params, x, gz=None, gz_all=None, gld=None):
    """Hand reverse mode: (flat gradient in state_dict order -- s, t per
    layer --, dx [B, D]) for upstream gradients of the final z, of every
    layer's output and of the log-det (None = zero)."""
    x = np.asarray(x, dtype=np.float64)
    B, D = x.shape
    L = len(params)
    zs, _ = forward(params, x)
    gl = 0.0 if gld is None else float(np.asarray(gld, dtype=np.float64).reshape(-1)[0])
    g = np.zeros((B, D))
    if gz is not None:
        g = g + np.asarray(gz, dtype=np.float64)
    if gz_all is not None:
        g = g + np.asarray(gz_all[L - 1], dtype=np.float64)
    out = [None] * L
    for l in range(L - 1, -1, -1):
        e = np.exp(_f64(params[l][0]))
        x_l = zs[l - 1] if l > 0 else x
        out[l] = np.concatenate([np.sum(g * x_l * e[None, :], axis=0) + gl, np.sum(g, axis=0)])
        g = g * e[None, :]
        if l > 0 and gz_all is not None:
            g = g + np.asarray(gz_all[l - 1], dtype=np.float64)
    return np.concatenate(out), g


def loss_vjp(params, x, y, kind, det=1.0, grad_scale=1.0):
    """(terms, flat gradient of grad_scale * sum of the per-row loss, dx)."""
    zs, ld = forward(params, x)
    terms, g, w = loss_terms(zs[-1], ld, np.asarray(y), kind, det)
    grads, dx = vjp(params, x, gz=g * grad_scale, gld=-w * grad_scale * x.shape[0])
    return np.array(terms), grads, dx


def _softmax(q):
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(q - np.max(q, axis=1, keepdims=True))
        return e / np.sum(e, axis=1, keepdims=True)


def predict(params, x, log_priors):
    """Calibrator.predict around an affine flow, float64: probs [B, D]."""
    x = np.asarray(x, dtype=np.float64)
    xc = x - np.mean(x, axis=1, keepdims=True)
    zs, _ = forward(params, xc)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.log(_softmax(zs[-1]) + 1e-7) - np.asarray(log_priors, dtype=np.float64)
    return _softmax(q)


# ---- the launch plan, restated (csrc/cnf_affine.hip over cnf_rowflow.h) ----------

ACC_D = 10   # kAccD: per-lane accumulators up to this width
SEG = 16     # kSeg: deep stacks checkpoint every SEG layers


def expected_plan(D, L, B):
    """cnf_affine_launch_plan from the constants of tests/_rowsweep.py."""
    import _rowsweep as S
    lpr, cpl = S.geometry(D)
    regt = L <= S.REG_L
    rega = regt and lpr == 1 and cpl <= ACC_D
    w = L * 2 * D + 4
    gacc = w > S.LDS_WORDS
    n = max(1, -(-B // (S.THREADS // lpr)))
    cap = max(4, min(S.BWD_CAP, (1 << 20) // w)) if gacc else S.BWD_CAP
    bwd = min(n, cap)
    return {"lpr": lpr, "cpl": cpl, "regt": int(regt), "rega": int(rega), "gacc": int(gacc),
            "fwd_blocks": min(n, S.FWD_CAP), "bwd_blocks": bwd,
            "bwd_units": bwd * (S.WAVES if gacc else 1)}


def workspace_floats(D, L, B):
    """The workspace formula of include/cnf.h: no tape term."""
    p = expected_plan(D, L, B)
    r64 = lambda n: (n + 63) // 64 * 64
    dp = p["lpr"] * p["cpl"]
    w = L * 2 * D + 4
    return r64(L * (2 * dp + 8)) + r64(w) + r64(max(p["bwd_units"] * w, 4 * p["fwd_blocks"]))


# ---- fixtures (tests/golden/affine, written by tests/golden/gen_golden_affine.py)

def load(name):
    """The fixture's arrays, the float64 outputs of <name>_f64.npz included."""
    root = os.path.join(GOLDEN, "affine")
    d = dict(np.load(os.path.join(root, name + ".npz")))
    d.update(np.load(os.path.join(root, name + "_f64.npz")))
    return d


def load_cal(name):
    return dict(np.load(os.path.join(GOLDEN, "affine_cal", name + ".npz")))


def params_of(d):
    return [(d["S"][l], d["T"][l]) for l in range(d["S"].shape[0])]


def flat_params(d):
    return np.concatenate([np.concatenate([d["S"][l], d["T"][l]]) for l in range(d["S"].shape[0])])


def build_flow(d, device="cpu", factory=False):
    """The package's Flow of AffineConstantLayers (AffineConstantFlow when
    `factory`) holding the fixture's parameters."""
    import torch
    from flows.flows import AffineConstantLayer, Flow
    L, D = d["S"].shape
    if factory:
        from flows._factory import AffineConstantFlow
        flow = AffineConstantFlow(D, layers=L)
    else:
        flow = Flow([AffineConstantLayer(D) for _ in range(L)])
    with torch.no_grad():
        for l, ly in enumerate(flow.layers):
            ly.s.copy_(torch.from_numpy(d["S"][l:l + 1]))
            ly.t.copy_(torch.from_numpy(d["T"][l:l + 1]))
    return flow.to(device)


def draw_params(rs, D, L):
    """The damped draw of the sweeps: s ~ min(0.3, 1 / L) N, t ~ min(0.5, 2 / L) N."""
    return {"S": (min(0.3, 1.0 / L) * rs.standard_normal((L, D))).astype(np.float32),
            "T": (min(0.5, 2.0 / L) * rs.standard_normal((L, D))).astype(np.float32)}
