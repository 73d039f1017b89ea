"""Float64 NumPy restatement of the planar flow (the reference's PlanarLayer,
flows/flows.py:129-165, stacked by Flow.forward) and of its hand-derived
reverse mode -- the formulas the kernels of csrc/cnf_planar.hip implement.
tests/test_planar_cpu.py holds it to the reference's float64 autograd
gradients recorded in tests/golden/planar/*.npz; it is the oracle for shapes
too large for fixtures.

Parameters: a list of (w [D], u [D], b [1]) per layer.
"""
import numpy as np


def layer_consts(w, u):
    w = np.asarray(w, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        wtu = float(w @ u)
        m = -1.0 + np.log1p(np.exp(wtu))
        nrm = float(np.sqrt(w @ w))
        u_hat = u + ((m - wtu) * w) / nrm
        c = float(w @ u_hat)
    return {"wtu": wtu, "m": m, "nrm": nrm, "u_hat": u_hat, "c": c}


def forward(params, x):
    """(zs [L, B, D], ld [B], hs [L, B]) in float64."""
    x = np.asarray(x, dtype=np.float64)
    zs, hs = [], []
    ld = np.zeros(x.shape[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        for w, u, b in params:
            k = layer_consts(w, u)
            w = np.asarray(w, dtype=np.float64)
            h = np.tanh(x @ w + float(np.asarray(b).reshape(-1)[0]))
            x = x + h[:, None] * k["u_hat"][None, :]
            ld = ld + np.log(np.abs(1.0 + (1.0 - h * h) * k["c"]))
            zs.append(x)
            hs.append(h)
    return np.stack(zs), ld, np.stack(hs)


def _log_softmax(z):
    m = z.max(axis=1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=1, keepdims=True))


def loss_terms(z, ld, y, kind, det=1.0):
    """(sum of per-row loss, sum of ce, sum of ld), and the seeds (g [B, D],
    gamma [B]) of the sum of the per-row loss."""
    B, D = z.shape
    lp = _log_softmax(z)
    p = np.exp(lp)
    oh = np.eye(D)[y]
    lpy = lp[np.arange(B), y]
    if kind == "cal":
        py = np.exp(lpy)
        ce = -np.log(py + 1e-7)
        loss = ce - ld
        g = (py / (py + 1e-7))[:, None] * (p - oh)
        gam = -np.ones(B)
    else:
        ce = -lpy
        loss = ce - det * ld
        g = p - oh
        gam = -det * np.ones(B)
    return (loss.sum(), ce.sum(), ld.sum()), g, gam


def vjp(params, x, gz=None, gz_all=None, gld=None):
    """Hand reverse mode: (flat gradient in state_dict order -- w, u, b per
    layer --, dx [B, D]) for upstream gradients of the final z, of every
    layer's output and of the summed log-det (None = zero)."""
    x = np.asarray(x, dtype=np.float64)
    B, D = x.shape
    L = len(params)
    zs, _, hs = forward(params, x)
    g = np.zeros((B, D))
    if gz is not None:
        g = g + np.asarray(gz, dtype=np.float64)
    if gz_all is not None:
        g = g + np.asarray(gz_all[L - 1], dtype=np.float64)
    gam = np.zeros(B) if gld is None else np.asarray(gld, dtype=np.float64).reshape(-1) * np.ones(B)
    out = [None] * L
    for l in range(L - 1, -1, -1):
        w = np.asarray(params[l][0], dtype=np.float64)
        u = np.asarray(params[l][1], dtype=np.float64)
        k = layer_consts(w, u)
        u_hat, c, nrm = k["u_hat"], k["c"], k["nrm"]
        h = hs[l]
        x_l = zs[l] - h[:, None] * u_hat[None, :]
        hp = 1.0 - h * h
        q = 1.0 + hp * c
        s = g @ u_hat
        g_a = s * hp + gam * (c / q) * (-2.0 * h * hp)
        G_uhat = h @ g
        G_c = float(np.sum(gam * hp / q))
        G_b = float(np.sum(g_a))
        G_w = g_a @ x_l
        g = g + g_a[:, None] * w[None, :]
        if l > 0 and gz_all is not None:
            g = g + np.asarray(gz_all[l - 1], dtype=np.float64)
        # once per layer: through c = w.u_hat and u_hat(w, u)
        kk = (k["m"] - k["wtu"]) / nrm
        sig = 1.0 / (1.0 + np.exp(-k["wtu"]))
        G_w = G_w + G_c * u_hat
        G_uhat = G_uhat + G_c * w
        t = float(G_uhat @ w)
        g_wtu = t * (sig - 1.0) / nrm
        g_u = G_uhat + g_wtu * w
        g_w = G_w + kk * G_uhat + g_wtu * u - t * kk * w / (nrm * nrm)
        out[l] = np.concatenate([g_w, g_u, [G_b]])
    return np.concatenate(out), g


def loss_vjp(params, x, y, kind, det=1.0, grad_scale=1.0):
    """(terms, flat gradient of grad_scale * sum of the per-row loss, dx)."""
    zs, ld, _ = forward(params, x)
    terms, g, gam = loss_terms(zs[-1], ld, np.asarray(y), kind, det)
    grads, dx = vjp(params, x, gz=g * grad_scale, gld=gam * grad_scale)
    return np.array(terms), grads, dx


# ---- fixtures (tests/golden/planar, written by tests/golden/gen_golden_planar.py)

def load(name):
    """The fixture's arrays, the float64 outputs of <name>_f64.npz included."""
    import os
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planar")
    d = dict(np.load(os.path.join(root, name + ".npz")))
    d.update(np.load(os.path.join(root, name + "_f64.npz")))
    return d


def params_of(d):
    return [(d["W"][l], d["U"][l], d["Bv"][l:l + 1]) for l in range(d["W"].shape[0])]


def build_flow(d, device="cpu"):
    """The package's Flow of PlanarLayers holding the fixture's parameters."""
    import torch
    from flows.flows import Flow, PlanarLayer
    L, D = d["W"].shape
    flow = Flow([PlanarLayer(D) for _ in range(L)])
    with torch.no_grad():
        for l, ly in enumerate(flow.layers):
            ly.w.copy_(torch.from_numpy(d["W"][l]))
            ly.u.copy_(torch.from_numpy(d["U"][l]))
            ly.b.copy_(torch.from_numpy(d["Bv"][l:l + 1]))
    return flow.to(device)


def bar(floor, tol=1e-5):
    """The project's rule (tests/test_gpu_parity.py): the tolerance, or twice
    the reference's own fp32-vs-float64 error where that is larger."""
    return max(tol, 2.0 * float(floor))
