"""Radial flows without a GPU: the float64 restatement of the forward, the hand
reverse mode and the predict (tests/_radial_ref.py) against the reference's
float64 record (tests/golden/radial), the cnf_radial_* C ABI's envelope,
workspace sizing and argument validation, RadialStack.compatible, the
factories the calibration notebooks import, and a CPU TorchFlowCalibrator fit
against the reference's own run (tests/golden/radial_cal)."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

import _radial_ref as R
from _golden import rel_err
from cnf_hip import _lib, engine
from test_gpu_vjp import _grad_err

P = ctypes.c_void_p
I32, I64 = ctypes.c_int32, ctypes.c_int64


# ---- the float64 restatement against the reference's float64 record --------------

@pytest.mark.parametrize("name", R.FIXTURES)
def test_restatement_forward_matches_float64_reference(name):
    d = R.load(name)
    zs, rs = R.forward(R.params_of(d), d["x"])
    assert rel_err(zs, d["zs64"]) <= 1e-12            # NaN positions coincide (sing)
    assert rel_err(R.predict(R.params_of(d), d["x"], d["log_priors"]), d["probs64"]) <= 1e-12
    if name not in ("zero", "sing"):
        assert rs.min() >= 1e-3 and float(d["amin"]) >= 0.05 and float(d["rmin"]) >= 1e-3


@pytest.mark.parametrize("name", R.GRAD_FIXTURES)
def test_restatement_gradients_match_float64_autograd(name):
    d = R.load(name)
    params, B = R.params_of(d), d["x"].shape[0]
    for kind in ("cal", "ce"):
        terms, grads, _ = R.loss_vjp(params, d["x"], d["y"], kind, grad_scale=1.0 / B)
        ref_loss = float(d["loss_%s_64" % kind])
        assert abs(terms[0] / B - ref_loss) <= 1e-12 * (abs(ref_loss) + 1)
        assert terms[2] == 0.0
        assert np.isfinite(grads).all()
        assert _grad_err(grads, d["g_%s_64" % kind]) <= 1e-10, (name, kind)


def test_special_fixtures_are_what_they_say():
    z = R.load("zero")
    assert np.array_equal(z["x"][5], z["Z0"][0]) and np.isfinite(z["zs"]).all()
    s = R.load("sing")
    assert float(s["A"][0]) == 0.0 and np.array_equal(s["x"][5], s["Z0"][0])
    nan_rows = np.isnan(s["zs"]).any(axis=(0, 2))
    assert nan_rows[5] and nan_rows.sum() == 1 and "g_cal" not in s
    n = R.load("neg")
    assert float(n["A"][1]) == np.float32(-0.3)
    assert R.load("tape")["Z0"].shape[0] == _lib.RADIAL_REG_LAYERS + 1


def test_restatement_upstream_gradients_match_autograd():
    """gz_all and dx of the hand reverse mode against torch autograd in
    float64 with random upstream weights on every layer's output."""
    d = R.load("d17")
    flow = R.build_flow(d).double()
    rs = np.random.RandomState(5)
    L, B, D = d["zs"].shape
    gz_all = rs.standard_normal((L, B, D))
    x = torch.from_numpy(d["x"]).double().requires_grad_(True)
    zs, ld = flow(x)
    obj = (torch.stack(zs) * torch.from_numpy(gz_all)).sum()
    res = torch.autograd.grad(obj, list(flow.parameters()) + [x])
    ref = torch.cat([g.reshape(-1) for g in res[:-1]]).numpy()
    grads, dx = R.vjp(R.params_of(d), d["x"], gz_all=gz_all)
    assert _grad_err(grads, ref) <= 1e-10
    assert _grad_err(dx, res[-1].numpy()) <= 1e-10


# ---- the CPU modules ----------------------------------------------------------------

@pytest.mark.parametrize("name", R.FIXTURES)
def test_cpu_flow_matches_reference(name):
    d = R.load(name)
    flow = R.build_flow(d)
    n0 = engine.stats["radial_forward"]
    with torch.no_grad():
        zs, ld = flow(torch.from_numpy(d["x"]))
    assert engine.stats["radial_forward"] == n0       # host tensors stay on torch ops
    assert ld.dim() == 0 and ld.dtype == torch.float32 and float(ld) == 0.0
    got = torch.stack(zs).numpy()
    assert rel_err(got, d["zs64"]) <= R.bar(d["floor_zs"]) and rel_err(got, d["zs"]) <= 1e-5


def test_notebook_import_line():
    from flows.normalizing_flows_torch import PlanarFlow, RadialFlow, AffineConstantFlow
    from flows import _factory
    assert PlanarFlow is _factory.PlanarFlow and RadialFlow is _factory.RadialFlow
    assert AffineConstantFlow is _factory.AffineConstantFlow


def test_radial_flow_factory():
    from flows.flows import Flow, RadialLayer
    from flows.normalizing_flows_torch import RadialFlow
    torch.manual_seed(3)
    flow = RadialFlow(3)
    assert isinstance(flow, Flow) and len(flow.layers) == 10
    assert all(isinstance(ly, RadialLayer) for ly in flow.layers)
    assert len(RadialFlow(4, layers=2, dev="cpu", epochs=3).layers) == 2   # calibrator kwargs
    assert list(flow.state_dict())[:3] == ["layers.0.z0", "layers.0.a", "layers.0.b"]
    x = torch.randn(7, 3)
    with torch.no_grad():
        z, ld = flow(x)
        zs, ld_all = flow.forward_all(x)
    assert z.shape == (7, 3) and ld.dim() == 0 and float(ld) == 0.0 and ld.dtype == torch.float32
    assert isinstance(zs, list) and len(zs) == 10 and torch.equal(zs[-1], z)
    assert ld_all.dim() == 0 and float(ld_all) == 0.0
    # the layers in the reference's order, by hand
    h = x
    with torch.no_grad():
        for ly in flow.layers:
            b_hat = -ly.a + torch.log1p(torch.exp(ly.b))
            diff = h - ly.z0
            hh = 1. / (ly.a + torch.norm(diff, dim=1, keepdim=True))
            h = h + b_hat * hh.expand_as(diff) * diff
    assert torch.equal(h, z)
    with pytest.raises(ValueError, match="Flow inverse not tractable!"):
        Flow.backward(flow, z)


def test_affine_constant_flow_factory():
    from flows.flows import AffineConstantLayer
    from flows.normalizing_flows_torch import AffineConstantFlow
    torch.manual_seed(4)
    flow = AffineConstantFlow(3, layers=5)
    assert len(flow.layers) == 5 and all(isinstance(ly, AffineConstantLayer) for ly in flow.layers)
    assert len(AffineConstantFlow(3).layers) == 5
    with torch.no_grad():
        for p in flow.parameters():
            p.normal_(0, 0.3)
    x = torch.randn(9, 3)
    with torch.no_grad():
        z, ld = flow(x)
        zs, ld_all = flow.forward_all(x)
        h, cum = x, 0.0
        for ly in flow.layers:                       # Flow.forward of the reference, by hand
            h = h * torch.exp(ly.s) + ly.t
            cum = cum + torch.sum(ly.s, dim=1)
    assert torch.equal(z, h) and torch.equal(ld, cum) and ld.shape == (1,)
    assert len(zs) == 5 and torch.equal(zs[-1], z) and torch.equal(ld_all, ld)


def test_radial_flow_pickle_round_trip():
    from flows.normalizing_flows_torch import RadialFlow
    torch.manual_seed(5)
    flow = RadialFlow(4, layers=3)
    x = torch.randn(5, 4)
    with torch.no_grad():
        z, _ = flow(x)
    flow._rstack = object()                           # a binding must not travel
    flow.layers[0]._stack = object()
    back = pickle.loads(pickle.dumps(flow))
    assert back._rstack is None and back._rstack_key is None and back.layers[0]._stack is None
    with torch.no_grad():
        z2, ld2 = back(x)
    assert torch.equal(z, z2) and float(ld2) == 0.0
    assert all(torch.equal(p, q) for p, q in zip(flow.parameters(), back.parameters()))


def test_cpu_calibrator_fit_matches_reference_run():
    """The CPU loop (the reference's own, on torch ops) around RadialFlow: the
    bars tests/test_calibrator.py uses for it."""
    import calibrators as C
    from flows.normalizing_flows_torch import RadialFlow
    d = R.load_cal("full")
    tol = 1e-5
    torch.manual_seed(int(d["seed"]))
    n0 = dict(engine.stats)
    cal = C.TorchFlowCalibrator(RadialFlow, d["logits"], np.eye(3)[d["labels"]],
                                layers=d["Z0"].shape[0], epochs=int(d["epochs"]),
                                batch_size=int(d["batch_size"]), dev=torch.device("cpu"))
    assert all(engine.stats[k] == n0[k] for k in n0 if k.startswith("radial_"))
    for k in ("loss", "ce", "log_det"):
        got = np.array([float(v) for v in cal.history[k]])
        assert np.max(np.abs(got - d[k]) / (np.abs(d[k]) + 1)) <= tol, k
    assert not np.array([float(v) for v in cal.history["log_det"]]).any()
    for l, ly in enumerate(cal.flow.layers):
        for got, ref in ((ly.z0, d["Z0"][l]), (ly.a, d["A"][l:l + 1]), (ly.b, d["Bv"][l:l + 1])):
            assert np.max(np.abs(got.detach().numpy() - ref)) <= tol * (np.max(np.abs(ref)) + 1e-3)
    assert np.max(np.abs(cal.predict(d["held"]) - d["pred"])) <= tol


# ---- C ABI ------------------------------------------------------------------------------

def test_exports_match_header():
    names = [n for n in _lib.EXPORTS if n.startswith("cnf_radial_")]
    assert sorted(names) == sorted("cnf_radial_" + s for s in (
        "param_count", "workspace_bytes", "launch_plan", "forward", "forward_loss", "vjp",
        "loss_vjp", "predict", "score"))
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in names)


def test_param_count_matches_state_dict():
    from cnf_hip.radial import param_count
    from flows.flows import Flow, RadialLayer
    for D, L in [(3, 10), (10, 10), (100, 4), (1, 1), (256, 64)]:
        flow = Flow([RadialLayer(D) for _ in range(L)])
        assert param_count(D, L) == sum(p.numel() for p in flow.parameters()) == L * (D + 2)


@pytest.mark.parametrize("D,L,status", [(0, 1, -2), (3, 0, -2), (-1, 1, -2), (257, 1, -3),
                                        (3, 65, -3), (256, 64, 0), (1, 1, 0)])
def test_envelope(D, L, status):
    lib = _lib.lib()
    n, b = I64(), ctypes.c_size_t()
    assert lib.cnf_radial_param_count(I32(D), I32(L), ctypes.byref(n)) == status
    assert lib.cnf_radial_workspace_bytes(I32(D), I32(L), I64(8), ctypes.byref(b)) == status


def _r64(n):
    return (n + 63) // 64 * 64


def _plan_floats(D, L, B):
    """The workspace formula of include/cnf.h, restated."""
    lpr = 1 if D <= 16 else 16 if D <= 64 else 64
    dp = (D + lpr - 1) // lpr * lpr
    pw = L * (D + 2) + 4
    ceil = lambda a, b: -(-a // b)
    f = max(1, min(1024, ceil(B * lpr, 256)))
    c = max(1, min(256, ceil(B * lpr, 256)))
    u = c if pw <= 3072 else 4 * min(c, max(4, min(256, (1 << 20) // pw)))
    tape = _r64(L * B) if L > _lib.RADIAL_REG_LAYERS else 0
    return _r64(L * (dp + 8)) + _r64(pw) + _r64(max(u * pw, 4 * f)) + tape


@pytest.mark.parametrize("D,L", [(1, 1), (3, 10), (3, 11), (10, 10), (16, 64), (17, 3), (64, 48),
                                 (100, 4), (256, 64)])
@pytest.mark.parametrize("B", [0, 1, 63, 256, 257, 777, 65537, 1 << 20])
def test_workspace_bytes_formula(D, L, B):
    from cnf_hip.radial import workspace_bytes
    assert workspace_bytes(D, L, B) == 4 * _plan_floats(D, L, B)


def _args(L=2, bad=None):
    arr = (P * (3 * L))(*[4096 + 64 * i for i in range(3 * L)])
    if bad is not None:
        arr[bad[0]] = bad[1]
    return arr


def test_argument_validation_without_gpu():
    """Every error is returned before any launch (no GPU here)."""
    from cnf_hip.radial import workspace_bytes
    lib = _lib.lib()
    D, L, B = 3, 2, 8
    ws = workspace_bytes(D, L, B)
    sz, F = ctypes.c_size_t, ctypes.c_float
    fwd = lambda params, x, z, za, b, w, wb, d=D: lib.cnf_radial_forward(
        I32(d), I32(L), params, P(x), P(z), P(za), I64(b), P(w), sz(wb), P(0))
    assert fwd(_args(), 16, 16, 0, -1, 16, ws) == -4
    assert fwd(None, 16, 16, 0, B, 16, ws) == -1
    assert fwd(_args(bad=(4, 0)), 16, 16, 0, B, 16, ws) == -1
    assert fwd(_args(bad=(4, 4098)), 16, 16, 0, B, 16, ws) == -6
    assert fwd(_args(), 0, 16, 0, B, 16, ws) == -1
    assert fwd(_args(), 16, 16, 0, B, 16, ws - 4) == -1
    assert fwd(_args(), 16, 18, 0, B, 16, ws) == -6
    assert fwd(_args(), 16, 16, 0, B, 16, ws, d=300) == -3
    assert fwd(_args(), 0, 0, 0, 0, 0, 0) == 0                          # B == 0: a no-op
    fl = lambda y, kind, terms: lib.cnf_radial_forward_loss(
        I32(D), I32(L), _args(), P(16), P(y), I32(kind), P(0), P(terms), I64(B), P(16), sz(ws),
        P(0))
    assert fl(0, 0, 16) == -1 and fl(16, 0, 0) == -1 and fl(20, 0, 16) == -6
    assert fl(16, 7, 16) == -2
    vjp = lambda gz, grads, dx: lib.cnf_radial_vjp(
        I32(D), I32(L), _args(), P(16), P(gz), P(0), P(grads), P(dx), I64(B), P(16), sz(ws), P(0))
    assert vjp(16, 0, 0) == -1 and vjp(18, 16, 0) == -6 and vjp(16, 16, 18) == -6
    lv = lambda y, terms, grads, kind=0: lib.cnf_radial_loss_vjp(
        I32(D), I32(L), _args(), P(16), P(y), I32(kind), F(1.0), P(terms), P(grads), P(0), I64(B),
        P(16), sz(ws), P(0))
    assert lv(0, 16, 16) == -1 and lv(16, 0, 16) == -1 and lv(16, 16, 0) == -1
    assert lv(16, 16, 16, kind=2) == -2
    pr = lambda lp, probs: lib.cnf_radial_predict(
        I32(D), I32(L), _args(), P(16), P(lp), P(probs), I64(B), P(16), sz(ws), P(0))
    assert pr(0, 16) == -1 and pr(16, 0) == -1 and pr(18, 16) == -6
    sc = lambda y, bins, rec, d=D, b=B: lib.cnf_radial_score(
        I32(d), I32(L), _args(), P(16), P(16), P(y), I32(bins), P(rec), I64(b), P(16), sz(ws), P(0))
    assert sc(16, 0, 16) == -2 and sc(16, _lib.MAX_BINS + 1, 16) == -2 and sc(16, 15, 16, d=1) == -2
    assert sc(16, 15, 0) == -1 and sc(0, 15, 16) == -1 and sc(20, 15, 16) == -6
    assert sc(16, 15, 16, b=(1 << 26) + 1) == -4
    assert sc(0, 15, 16, b=0) == 0


def test_compatible():
    from cnf_hip.radial import RadialStack
    from flows.flows import PlanarLayer, RadialLayer
    ok = [RadialLayer(5) for _ in range(3)]
    assert RadialStack.compatible(ok) and RadialStack.compatible(ok, "cpu")
    assert not RadialStack.compatible(ok, "cuda:0")            # parameters sit on the host
    assert not RadialStack.compatible([])
    assert not RadialStack.compatible(ok + [RadialLayer(4)])   # widths differ
    assert not RadialStack.compatible(ok + [PlanarLayer(5)])
    assert not RadialStack.compatible([RadialLayer(5).double()])
    st = RadialStack(ok)
    assert st.dim == 5 and st.L == 3 and st.param_count() == 21
    assert [p.shape for p in st.param_tensors()[:3]] == [(5,), (1,), (1,)]
    assert [g.shape for g in st.split(torch.zeros(21))[:3]] == [(5,), (1,), (1,)]
