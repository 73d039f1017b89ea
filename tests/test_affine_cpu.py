"""Affine-constant flows without a GPU: the float64 restatement of the forward,
the inverse, the hand reverse mode and the predict (tests/_affine_ref.py)
against the reference's float64 record (tests/golden/affine), the cnf_affine_*
C ABI's envelope, workspace sizing, launch plan and argument validation,
AffineStack.compatible, the pickle round trip, and the CPU flow and CPU
TorchFlowCalibrator fit against the reference's own runs."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

import _affine_ref as A
import _affine_sweep as AS
import _rowsweep as S
from _golden import rel_err
from cnf_hip import _lib, engine, rowstack
from test_gpu_vjp import _grad_err

P = ctypes.c_void_p
I32, I64 = ctypes.c_int32, ctypes.c_int64
OUT_COND, GRAD_COND = S.OUT_COND, S.GRAD_COND


# ---- the float64 restatement against the reference's float64 record --------------

@pytest.mark.parametrize("name", A.FIXTURES)
def test_restatement_matches_float64_reference(name):
    d = A.load(name)
    params = A.params_of(d)
    zs, ld = A.forward(params, d["x"])
    assert rel_err(zs, d["zs64"]) <= 1e-12 and abs(ld - float(d["ld64"][0])) <= 1e-12
    xs, ild = A.inverse(params, d["zs64"][-1])
    assert rel_err(xs, d["xs64"]) <= 1e-9 and abs(ild - float(d["ild64"][0])) <= 1e-12
    assert rel_err(A.predict(params, d["x"], d["log_priors"]), d["probs64"]) <= 1e-12
    assert d["ld"].shape == (1,) and d["ild"].shape == (1,)       # also at B == 1


@pytest.mark.parametrize("name", A.FIXTURES)
def test_restatement_gradients_match_float64_autograd(name):
    d = A.load(name)
    params, B = A.params_of(d), d["x"].shape[0]
    for kind, det in (("cal", 1.0), ("ce", float(d["det"]))):
        terms, grads, _ = A.loss_vjp(params, d["x"], d["y"], kind, det, 1.0 / B)
        ref_loss = float(d["loss_%s_64" % kind])
        assert abs(terms[0] / B - ref_loss) <= 1e-12 * (abs(ref_loss) + 1)
        assert abs(terms[2] - B * float(d["ld64"][0])) <= 1e-9
        assert _grad_err(grads, d["g_%s_64" % kind]) <= 1e-10, (name, kind)


def test_fixtures_are_what_they_say():
    """The recorded fp32-vs-float64 floors lie within a quarter of each bar
    (the inverse of `contract` excepted: inverting exp(-6) loses its input)."""
    for name in A.FIXTURES:
        d = A.load(name)
        assert max(float(d[k]) for k in ("floor_zs", "floor_ld", "floor_probs")) <= OUT_COND, name
        assert max(float(d["floor_g_cal"]), float(d["floor_g_ce"])) <= GRAD_COND, name
        assert (float(d["floor_xs"]) <= OUT_COND) == (name != "contract"), name
    i = A.load("init")
    assert not i["S"].any() and not i["T"].any() and np.array_equal(i["zs"][-1], i["x"])
    assert np.abs(i["g_cal"]).max() > 0
    c = A.load("contract")
    assert (c["S"][0] == -6).all() and (c["T"][0] == 3).all() and c["S"].shape == (10, 10)
    c = A.load("centre")
    assert (c["S"][0] == 0).all() and (c["T"][0] == -5).all() and abs(c["x"].mean() - 5) < 0.1
    assert A.load("tape")["S"].shape[0] == S.REG_L + 1


def test_restatement_upstream_gradients_match_autograd():
    """gz_all, gld and dx of the hand reverse mode against torch autograd in
    float64 with random upstream weights on every layer's output and on the
    log-det."""
    d = A.load("d17")
    flow = A.build_flow(d).double()
    rs = np.random.RandomState(5)
    L, B, D = d["zs"].shape
    gz_all, gld = rs.standard_normal((L, B, D)), rs.standard_normal(1)
    x = torch.from_numpy(d["x"]).double().requires_grad_(True)
    zs, ld = flow(x)
    obj = (torch.stack(zs) * torch.from_numpy(gz_all)).sum() + (ld * torch.from_numpy(gld)).sum()
    res = torch.autograd.grad(obj, list(flow.parameters()) + [x])
    ref = torch.cat([g.reshape(-1) for g in res[:-1]]).numpy()
    grads, dx = A.vjp(A.params_of(d), d["x"], gz_all=gz_all, gld=gld)
    assert _grad_err(grads, ref) <= 1e-10 and _grad_err(dx, res[-1].numpy()) <= 1e-10


# ---- the CPU modules ----------------------------------------------------------------

@pytest.mark.parametrize("name", A.FIXTURES)
def test_cpu_flow_matches_reference(name):
    d = A.load(name)
    flow = A.build_flow(d)
    n0 = dict(engine.stats)
    with torch.no_grad():
        zs, ld = flow(torch.from_numpy(d["x"]))
        xs, ild = flow.backward(zs[-1])
        z1, ld1 = flow.layers[0](torch.from_numpy(d["x"]))
    assert engine.stats == n0                         # host tensors stay on torch ops
    assert ld.shape == (1,) and ild.shape == (1,) and ld1.shape == (1,)
    assert np.array_equal(torch.stack(zs).numpy(), d["zs"]) and np.array_equal(ld.numpy(), d["ld"])
    assert np.array_equal(torch.stack(xs).numpy(), d["xs"]) and np.array_equal(ild.numpy(), d["ild"])
    assert torch.equal(z1, zs[0])


def test_layer_family_and_switch():
    from flows import flows as FL
    assert FL.AffineConstantLayer._family == "affine" and FL.AFFINE_NATIVE is True
    assert "_astack" in FL.Flow._BINDINGS
    assert rowstack.stack_class("affine").__name__ == "AffineStack"
    assert all("affine_" + k in engine.stats
               for k in ("forward", "inverse", "vjp", "loss_vjp", "predict", "score"))


def test_pickle_round_trip():
    from flows.normalizing_flows_torch import AffineConstantFlow
    flow = AffineConstantFlow(4, layers=3)
    with torch.no_grad():
        for p in flow.parameters():
            p.normal_(0, 0.3)
    x = torch.randn(5, 4)
    with torch.no_grad():
        z, ld = flow(x)
    flow._astack = object()                           # a binding must not travel
    flow.layers[0]._stack = object()
    back = pickle.loads(pickle.dumps(flow))
    assert back._astack is None and back._astack_key is None and back.layers[0]._stack is None
    with torch.no_grad():
        z2, ld2 = back(x)
        x2, ild = back.backward(z2)
    assert torch.equal(z, z2) and torch.equal(ld, ld2) and ld2.shape == (1,) and ild.shape == (1,)
    assert list(flow.state_dict())[:2] == ["layers.0.s", "layers.0.t"]


def test_cpu_calibrator_fit_matches_reference_run():
    """The CPU loop (the reference's own, on torch ops) around
    AffineConstantFlow, log-det history included."""
    import calibrators as C
    from flows.normalizing_flows_torch import AffineConstantFlow
    for name in ("full", "mb128"):
        d = A.load_cal(name)
        tol = 1e-5
        torch.manual_seed(int(d["seed"]))
        n0 = dict(engine.stats)
        cal = C.TorchFlowCalibrator(AffineConstantFlow, d["logits"], np.eye(3)[d["labels"]],
                                    layers=d["S"].shape[0], epochs=int(d["epochs"]),
                                    batch_size=int(d["batch_size"]), dev=torch.device("cpu"))
        assert engine.stats == n0
        for k in ("loss", "ce", "log_det"):
            got = np.array([float(v) for v in cal.history[k]])
            assert np.max(np.abs(got - d[k]) / (np.abs(d[k]) + 1)) <= tol, k
        assert np.array([float(v) for v in cal.history["log_det"]]).any()
        for l, ly in enumerate(cal.flow.layers):
            for got, ref in ((ly.s, d["S"][l:l + 1]), (ly.t, d["T"][l:l + 1])):
                assert np.max(np.abs(got.detach().numpy() - ref)) <= tol
        assert np.max(np.abs(cal.predict(d["held"]) - d["pred"])) <= tol


# ---- C ABI ------------------------------------------------------------------------------

def test_exports_match_header():
    names = [n for n in _lib.EXPORTS if n.startswith("cnf_affine_")]
    assert sorted(names) == sorted("cnf_affine_" + s for s in (
        "param_count", "workspace_bytes", "launch_plan", "forward", "inverse", "forward_loss",
        "vjp", "loss_vjp", "predict", "score"))
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in names)
    src = open(A.os.path.join(A.os.path.dirname(A.GOLDEN), "..", "include", "cnf.h")).read()
    assert "#define CNF_AFFINE_MAX_LAYERS 64" in src and _lib.AFFINE_MAX_LAYERS == 64
    assert all("int %s(" % n in src for n in names)


def test_param_count_matches_state_dict():
    from cnf_hip.affine import param_count
    from flows.flows import AffineConstantLayer, Flow
    for D, L in [(3, 5), (10, 5), (100, 4), (1, 1), (256, 64)]:
        flow = Flow([AffineConstantLayer(D) for _ in range(L)])
        assert param_count(D, L) == sum(p.numel() for p in flow.parameters()) == 2 * L * D


@pytest.mark.parametrize("D,L,status", [(0, 1, -2), (3, 0, -2), (-1, 1, -2), (257, 1, -3),
                                        (3, 65, -3), (256, 64, 0), (1, 1, 0)])
def test_envelope(D, L, status):
    lib = _lib.lib()
    n, b = I64(), ctypes.c_size_t()
    out = (I32 * 8)()
    assert lib.cnf_affine_param_count(I32(D), I32(L), ctypes.byref(n)) == status
    assert lib.cnf_affine_workspace_bytes(I32(D), I32(L), I64(8), ctypes.byref(b)) == status
    assert lib.cnf_affine_launch_plan(I32(D), I32(L), I64(8), out) == status


@pytest.mark.parametrize("D,L", [(1, 1), (3, 5), (3, 11), (10, 10), (16, 64), (17, 3), (64, 48),
                                 (100, 4), (256, 64)])
@pytest.mark.parametrize("B", [0, 1, 63, 256, 257, 777, 65537, 1 << 20])
def test_workspace_bytes_formula(D, L, B):
    """No tape term at any depth; the siblings' byte counts did not move."""
    from cnf_hip.affine import workspace_bytes
    assert workspace_bytes(D, L, B) == 4 * A.workspace_floats(D, L, B)
    for fam in S.FAMILIES:
        assert rowstack.workspace_bytes(fam, D, L, B) == 4 * S.workspace_floats(fam, D, L, B)


def test_sibling_workspace_bytes_did_not_move():
    """Literals worked out from the formulas of include/cnf.h for the planar
    and radial families (a register-depth and a tape-depth stack of each): the
    plan's new family word for the tape leaves them where they were."""
    assert rowstack.workspace_bytes("planar", 10, 10, 777) == 5888
    assert rowstack.workspace_bytes("planar", 3, 11, 300) == 15360
    assert rowstack.workspace_bytes("radial", 3, 11, 300) == 14592
    assert rowstack.workspace_bytes("radial", 100, 4, 70) == 33792
    assert rowstack.workspace_bytes("radial", 256, 64, 251) == 16846336


@pytest.mark.parametrize("case", AS.CASES, ids=AS.IDS)
def test_launch_plan_of_every_sweep_case(case):
    want = case.plan()                                   # the restated plan + the case's literals
    assert rowstack.launch_plan("affine", case.D, case.L, case.B) == want
    assert rowstack.launch_plan("affine", case.D, case.L, 0) == A.expected_plan(case.D, case.L, 1)


def test_launch_plan_argument_errors():
    lib = _lib.lib()
    out = (I32 * 8)()
    assert lib.cnf_affine_launch_plan(I32(3), I32(5), I64(8), None) == -1
    assert lib.cnf_affine_launch_plan(I32(3), I32(5), I64(-1), out) == -4
    assert lib.cnf_affine_launch_plan(I32(3), I32(5), I64((1 << 31) + 1), out) == -4
    assert lib.cnf_affine_launch_plan(I32(3), I32(5), I64(1 << 31), out) == 0


def _args(L=2, bad=None):
    arr = (P * (2 * L))(*[4096 + 64 * i for i in range(2 * L)])
    if bad is not None:
        arr[bad[0]] = bad[1]
    return arr


def test_argument_validation_without_gpu():
    """Every error is returned before any launch (no GPU here)."""
    from cnf_hip.affine import workspace_bytes
    lib = _lib.lib()
    D, L, B = 3, 2, 8
    ws = workspace_bytes(D, L, B)
    sz, F = ctypes.c_size_t, ctypes.c_float
    for entry in (lib.cnf_affine_forward, lib.cnf_affine_inverse):
        fwd = lambda params, x, z, ld, za, b, w, wb, d=D: entry(
            I32(d), I32(L), params, P(x), P(z), P(ld), P(za), I64(b), P(w), sz(wb), P(0))
        assert fwd(_args(), 16, 16, 16, 0, -1, 16, ws) == -4
        assert fwd(_args(), 16, 16, 16, 0, (1 << 31) + 1, 16, ws) == -4
        assert fwd(None, 16, 16, 16, 0, B, 16, ws) == -1
        assert fwd(_args(bad=(3, 0)), 16, 16, 16, 0, B, 16, ws) == -1
        assert fwd(_args(bad=(3, 4098)), 16, 16, 16, 0, B, 16, ws) == -6
        assert fwd(_args(), 0, 16, 16, 0, B, 16, ws) == -1
        assert fwd(_args(), 16, 16, 16, 0, B, 0, ws) == -1
        assert fwd(_args(), 16, 16, 16, 0, B, 16, ws - 4) == -1
        assert fwd(_args(), 16, 18, 16, 0, B, 16, ws) == -6
        assert fwd(_args(), 16, 16, 18, 0, B, 16, ws) == -6
        assert fwd(_args(), 16, 16, 16, 18, B, 16, ws) == -6
        assert fwd(_args(), 16, 16, 16, 0, B, 16, ws, d=300) == -3
        assert fwd(_args(), 0, 0, 0, 0, 0, 0, 0) == 0                     # B == 0: a no-op
    fl = lambda y, kind, terms: lib.cnf_affine_forward_loss(
        I32(D), I32(L), _args(), P(16), P(y), I32(kind), F(1.0), P(0), P(0), P(terms), I64(B),
        P(16), sz(ws), P(0))
    assert fl(0, 0, 16) == -1 and fl(16, 0, 0) == -1 and fl(20, 0, 16) == -6
    assert fl(16, 7, 16) == -2
    vjp = lambda gz, gld, grads, dx: lib.cnf_affine_vjp(
        I32(D), I32(L), _args(), P(16), P(gz), P(0), P(gld), P(grads), P(dx), I64(B), P(16),
        sz(ws), P(0))
    assert vjp(16, 0, 0, 0) == -1 and vjp(18, 0, 16, 0) == -6 and vjp(16, 0, 16, 18) == -6
    assert vjp(16, 18, 16, 0) == -6
    lv = lambda y, terms, grads, kind=0, wb=ws: lib.cnf_affine_loss_vjp(
        I32(D), I32(L), _args(), P(16), P(y), I32(kind), F(1.0), F(1.0), P(terms), P(grads), P(0),
        I64(B), P(16), sz(wb), P(0))
    assert lv(0, 16, 16) == -1 and lv(16, 0, 16) == -1 and lv(16, 16, 0) == -1
    assert lv(16, 16, 16, kind=2) == -2 and lv(16, 16, 16, wb=ws - 1) == -1
    pr = lambda lp, probs: lib.cnf_affine_predict(
        I32(D), I32(L), _args(), P(16), P(lp), P(probs), I64(B), P(16), sz(ws), P(0))
    assert pr(0, 16) == -1 and pr(16, 0) == -1 and pr(18, 16) == -6
    sc = lambda y, bins, rec, d=D, b=B: lib.cnf_affine_score(
        I32(d), I32(L), _args(), P(16), P(16), P(y), I32(bins), P(rec), I64(b), P(16), sz(ws), P(0))
    assert sc(16, 0, 16) == -2 and sc(16, _lib.MAX_BINS + 1, 16) == -2 and sc(16, 15, 16, d=1) == -2
    assert sc(16, 15, 0) == -1 and sc(0, 15, 16) == -1 and sc(20, 15, 16) == -6
    assert sc(16, 15, 16, b=(1 << 26) + 1) == -4
    assert sc(0, 15, 16, b=0) == 0


def test_compatible():
    from cnf_hip.affine import AffineStack
    from cnf_hip.planar import PlanarStack
    from flows.flows import AffineConstantLayer, PlanarLayer
    ok = [AffineConstantLayer(5) for _ in range(3)]
    assert AffineStack.compatible(ok) and AffineStack.compatible(ok, "cpu")
    assert not AffineStack.compatible(ok, "cuda:0")            # parameters sit on the host
    assert not AffineStack.compatible([])
    assert not AffineStack.compatible(ok + [AffineConstantLayer(4)])   # widths differ
    assert not AffineStack.compatible(ok + [PlanarLayer(5)])           # a mixed flow
    assert not AffineStack.compatible(ok + [AffineConstantLayer(5, scale=False)])
    assert not AffineStack.compatible([AffineConstantLayer(5, shift=False)] + ok)
    assert not AffineStack.compatible([AffineConstantLayer(5).double()])
    nc = AffineConstantLayer(5)
    nc.s = torch.nn.Parameter(torch.zeros(5, 1).t())           # [1, 5] with stride (1, 1)...
    nc.t = torch.nn.Parameter(torch.zeros(1, 10)[:, ::2])      # ... and a strided one
    assert not nc.t.is_contiguous() and not AffineStack.compatible([nc])
    col = AffineConstantLayer(5)
    col.s = torch.nn.Parameter(torch.zeros(5, 1))              # [D, 1] broadcasts over the rows
    assert col.s.is_contiguous() and not AffineStack.compatible([col])
    col.s, col.t = torch.nn.Parameter(torch.zeros(1, 5)), torch.nn.Parameter(torch.zeros(5, 1))
    assert not AffineStack.compatible([col])
    assert not PlanarStack.compatible(ok) and PlanarStack.compatible([PlanarLayer(5)])
    st = AffineStack(ok)
    assert st.dim == 5 and st.L == 3 and st.param_count() == 30
    assert [p.shape for p in st.param_tensors()[:2]] == [(1, 5), (1, 5)]
    assert [g.shape for g in st.split(torch.zeros(30))[:2]] == [(1, 5), (1, 5)]
