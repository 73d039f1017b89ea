"""Float64 NumPy restatement of a mixed planar / radial / affine flow (the
reference's PlanarLayer, RadialLayer and AffineConstantLayer stacked in any
order by Flow.forward), of its hand-derived reverse mode and of a mixed
calibrator's predict -- what the kernels of csrc/cnf_mixed.hip implement.

It composes the single-family restatements layer by layer: a layer's forward,
and the reverse mode of that one layer from the gradient at its output, are
tests/_planar_ref.py, _radial_ref.py and _affine_ref.py applied to a stack of
one.  The log-det is a row's, [B]: 0, plus each planar layer's row term and
each affine layer's sum_d s, in layer order; a radial layer adds nothing.

Parameters: a list of (kind, tensors) per layer, kind "P" / "R" / "A" and
tensors (w, u, b) / (z0, a, b) / (s, t).
"""
import os

import numpy as np

import _affine_ref as AR
import _planar_ref as PR
import _radial_ref as RR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["pra", "d10", "deep", "contract", "d17", "d100", "ar", "one"]
KIND = {"P": 0, "R": 1, "A": 2}          # CNF_LAYER_*
FAMILY = {"P": "planar", "R": "radial", "A": "affine"}


def grad_floats(kind, D):
    return {"P": 2 * D + 1, "R": D + 2, "A": 2 * D}[kind]


def _layer_forward(kind, p, x):
    """(z [B, D], this layer's log-det per row [B])."""
    B = x.shape[0]
    if kind == "P":
        zs, ld, _ = PR.forward([p], x)
        return zs[0], np.asarray(ld, dtype=np.float64).reshape(-1) * np.ones(B)
    if kind == "R":
        zs, _ = RR.forward([p], x)
        return zs[0], np.zeros(B)
    zs, ld = AR.forward([p], x)
    return zs[0], np.full(B, float(ld))


def forward(params, x):
    """(zs [L, B, D], log-det [B]) in float64."""
    x = np.asarray(x, dtype=np.float64)
    zs, ld = [], np.zeros(x.shape[0])
    for kind, p in params:
        x, l = _layer_forward(kind, p, x)
        zs.append(x)
        ld = ld + l
    return np.stack(zs), ld


def loss_terms(z, ld, y, kind, det=1.0):
    """((sum of per-row loss, sum of ce, sum of ld), the seed g [B, D], the
    seed of the log-det [B]): the planar family's, whose log-det is a row's."""
    return PR.loss_terms(z, ld, y, kind, det)


def vjp(params, x, gz=None, gz_all=None, gld=None):
    """Hand reverse mode: (flat gradient in state_dict order, dx [B, D]) for
    upstream gradients of the final z, of every layer's output and of the
    per-row log-det (None = zero)."""
    x = np.asarray(x, dtype=np.float64)
    B, D = x.shape
    L = len(params)
    zs, _ = forward(params, x)
    g = np.zeros((B, D))
    if gz is not None:
        g = g + np.asarray(gz, dtype=np.float64)
    if gz_all is not None:
        g = g + np.asarray(gz_all[L - 1], dtype=np.float64)
    gam = np.zeros(B) if gld is None else np.asarray(gld, dtype=np.float64).reshape(-1) * np.ones(B)
    out = [None] * L
    for l in range(L - 1, -1, -1):
        kind, p = params[l]
        x_l = zs[l - 1] if l > 0 else x
        if kind == "P":
            out[l], g = PR.vjp([p], x_l, gz=g, gld=gam)
        elif kind == "R":
            out[l], g = RR.vjp([p], x_l, gz=g)
        else:  # one log-det for every row: its gradient is the rows' sum
            out[l], g = AR.vjp([p], x_l, gz=g, gld=np.array([gam.sum()]))
        if l > 0 and gz_all is not None:
            g = g + np.asarray(gz_all[l - 1], dtype=np.float64)
    return np.concatenate(out), g


def loss_vjp(params, x, y, kind, det=1.0, grad_scale=1.0):
    """(terms, flat gradient of grad_scale * sum of the per-row loss, dx)."""
    zs, ld = forward(params, x)
    terms, g, gam = loss_terms(zs[-1], ld, np.asarray(y), kind, det)
    grads, dx = vjp(params, x, gz=g * grad_scale, gld=gam * grad_scale)
    return np.array(terms), grads, dx


def predict(params, x, log_priors):
    """Calibrator.predict around a mixed flow, float64: probs [B, D]."""
    x = np.asarray(x, dtype=np.float64)
    xc = x - np.mean(x, axis=1, keepdims=True)
    zs, _ = forward(params, xc)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.log(AR._softmax(zs[-1]) + 1e-7) - np.asarray(log_priors, dtype=np.float64)
    return AR._softmax(q)


# ---- the launch plan, restated (csrc/cnf_mixed.hip over cnf_rowflow.h) ----------

ACC_D = 10   # kAccD: a one-lane row keeps its layers' inputs in registers up to this width
SEG = 16     # kSeg: the checkpointed kernel keeps the input of every SEG-th layer


def variant(D, L):
    """(regt, rega) of the reverse kernel."""
    import _rowsweep as S
    lpr, cpl = S.geometry(D)
    regt = L <= S.REG_L and (lpr != 1 or cpl <= ACC_D)
    return regt, regt and lpr == 1


def pw(D, L):
    return L * (2 * D + 2) + 4


def expected_plan(D, L, B):
    """cnf_mixed_launch_plan from the constants of tests/_rowsweep.py."""
    import _rowsweep as S
    lpr, cpl = S.geometry(D)
    regt, rega = variant(D, L)
    w = pw(D, L)
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
    w = pw(D, L)
    return r64(L * (2 * dp + 8)) + r64(w) + r64(max(p["bwd_units"] * w, 4 * p["fwd_blocks"]))


# ---- fixtures (tests/golden/mixed, written by tests/golden/gen_golden_mixed.py) ---

def load(name):
    """The fixture's arrays, the float64 outputs of <name>_f64.npz included."""
    root = os.path.join(GOLDEN, "mixed")
    d = dict(np.load(os.path.join(root, name + ".npz")))
    d.update(np.load(os.path.join(root, name + "_f64.npz")))
    return d


def load_cal(name):
    return dict(np.load(os.path.join(GOLDEN, "mixed_cal", name + ".npz")))


def order_of(d):
    return str(d["order"])


def params_of(d):
    """The fixture's layers: parameter l is d["p<l>_<name>"]."""
    out = []
    for l, kind in enumerate(order_of(d)):
        names = {"P": ("w", "u", "b"), "R": ("z0", "a", "b"), "A": ("s", "t")}[kind]
        out.append((kind, tuple(np.asarray(d["p%d_%s" % (l, n)]) for n in names)))
    return out


def flat_params(params):
    return np.concatenate([np.asarray(t, dtype=np.float64).reshape(-1)
                           for _, p in params for t in p])


def build_flow(params, device="cpu", factory=False):
    """The package's Flow (MixedFlow when `factory`) holding these layers."""
    import torch
    from flows.flows import AffineConstantLayer, Flow, PlanarLayer, RadialLayer
    D = int(np.asarray(params[0][1][0]).size)
    if factory:
        from flows._factory import MixedFlow
        flow = MixedFlow(D, layers="".join(k for k, _ in params))
    else:
        cls = {"P": PlanarLayer, "R": RadialLayer, "A": AffineConstantLayer}
        flow = Flow([cls[k](D) for k, _ in params])
    names = {"P": ("w", "u", "b"), "R": ("z0", "a", "b"), "A": ("s", "t")}
    with torch.no_grad():
        for ly, (k, p) in zip(flow.layers, params):
            for n, v in zip(names[k], p):
                t = getattr(ly, n)
                t.copy_(torch.from_numpy(np.asarray(v, dtype=np.float32)).reshape(t.shape))
    return flow.to(device)


def draw_params(rs, D, order, contract=False):
    """A damped draw for the sweeps and fixtures: planar and radial as their
    families' sweeps draw them, affine s ~ min(0.3, 1 / L) N, t ~ min(0.5,
    2 / L) N (contract: s = -6, t = 3)."""
    L = len(order)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    out = []
    for kind in order:
        if kind == "P":
            sc = min(0.5, 1.0 / np.sqrt(D))
            out.append(("P", (f32(sc * rs.standard_normal(D)), f32(sc * rs.standard_normal(D)),
                              f32(0.5 * rs.standard_normal(1)))))
        elif kind == "R":
            out.append(("R", (f32(0.5 * rs.standard_normal(D)),
                              f32(np.abs(1.0 + 0.5 * rs.standard_normal(1))),
                              f32(0.5 * rs.standard_normal(1)))))
        elif contract:
            out.append(("A", (f32(np.full(D, -6.0)), f32(np.full(D, 3.0)))))
        else:
            out.append(("A", (f32(min(0.3, 1.0 / L) * rs.standard_normal(D)),
                              f32(min(0.5, 2.0 / L) * rs.standard_normal(D)))))
    return out


def bar(floor, tol=1e-5):
    """The bar of a compared quantity whose reference floor is `floor`: tol
    where the reference's own fp32 run meets it, else twice that floor."""
    return max(tol, 2.0 * float(floor))
