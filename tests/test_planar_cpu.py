"""Planar flows without a GPU: the cnf_planar_* C ABI's argument validation and
workspace sizing, PlanarStack.compatible, the CPU Flow / PlanarLayer against
the reference's recorded outputs (tests/golden/planar), and the float64
restatement of the forward and the hand reverse mode (tests/_planar_ref.py)
against the reference's float64 autograd gradients."""
import ctypes

import numpy as np
import pytest
import torch

import _planar_ref as R
from _golden import rel_err
from cnf_hip import _lib
from cnf_hip.planar import PlanarStack, param_count, workspace_bytes
from flows.flows import Flow, NvpCouplingLayer, PlanarLayer
from test_gpu_vjp import _grad_err

FIXTURES = ["one", "d3", "d10", "d10n", "d17", "d100", "tape"]
P = ctypes.c_void_p
I32, I64 = ctypes.c_int32, ctypes.c_int64


# ---- C ABI ------------------------------------------------------------------

def test_param_count_matches_state_dict():
    for D, L in [(3, 10), (10, 10), (100, 4), (1, 1), (256, 64)]:
        flow = Flow([PlanarLayer(D) for _ in range(L)])
        assert param_count(D, L) == sum(p.numel() for p in flow.parameters()) == L * (2 * D + 1)
    assert list(Flow([PlanarLayer(3)]).state_dict()) == ["layers.0.w", "layers.0.u", "layers.0.b"]


@pytest.mark.parametrize("D,L,status", [(0, 1, -2), (3, 0, -2), (-1, 1, -2), (257, 1, -3),
                                        (3, 65, -3), (256, 64, 0), (1, 1, 0)])
def test_envelope(D, L, status):
    lib = _lib.lib()
    n, b = I64(), ctypes.c_size_t()
    assert lib.cnf_planar_param_count(I32(D), I32(L), ctypes.byref(n)) == status
    assert lib.cnf_planar_workspace_bytes(I32(D), I32(L), I64(8), ctypes.byref(b)) == status


def _r64(n):
    return (n + 63) // 64 * 64


def _plan_floats(D, L, B):
    """The workspace formula of include/cnf.h, restated."""
    lpr = 1 if D <= 16 else 16 if D <= 64 else 64
    dp = (D + lpr - 1) // lpr * lpr
    pw = L * (2 * D + 2) + 4
    ceil = lambda a, b: -(-a // b)
    f = max(1, min(1024, ceil(B * lpr, 256)))
    c = max(1, min(256, ceil(B * lpr, 256)))
    if pw <= 3072:
        u = c
    else:
        u = 4 * min(c, max(4, min(256, (1 << 20) // pw)))
    tape = _r64(L * B) if L > _lib.PLANAR_REG_LAYERS else 0
    return _r64(L * (2 * dp + 8)) + _r64(pw) + _r64(max(u * pw, 4 * f)) + tape


@pytest.mark.parametrize("D,L", [(1, 1), (3, 10), (3, 11), (10, 10), (16, 64), (17, 3), (64, 23),
                                 (65, 24), (100, 4), (256, 64)])
@pytest.mark.parametrize("B", [0, 1, 63, 256, 257, 777, 65537, 1 << 20])
def test_workspace_bytes_formula(D, L, B):
    assert workspace_bytes(D, L, B) == 4 * _plan_floats(D, L, B)


def test_workspace_batch_limits():
    lib = _lib.lib()
    b = ctypes.c_size_t()
    assert lib.cnf_planar_workspace_bytes(I32(3), I32(2), I64(-1), ctypes.byref(b)) == -4
    assert lib.cnf_planar_workspace_bytes(I32(3), I32(2), I64((1 << 31) + 1), ctypes.byref(b)) == -4
    assert lib.cnf_planar_workspace_bytes(I32(3), I32(2), I64(1 << 31), ctypes.byref(b)) == 0
    assert lib.cnf_planar_workspace_bytes(I32(3), I32(2), I64(8), None) == -1


def _args(L=2, bad=None):
    arr = (P * (3 * L))(*[4096 + 64 * i for i in range(3 * L)])
    if bad is not None:
        arr[bad[0]] = bad[1]
    return arr


def test_forward_argument_validation_without_gpu():
    """Every error is returned before any launch (no GPU here)."""
    lib = _lib.lib()
    D, L, B = 3, 2, 8
    ws = workspace_bytes(D, L, B)
    fwd = lambda params, x, z, ld, za, b, w, wb, d=D, l=L: lib.cnf_planar_forward(
        I32(d), I32(l), params, P(x), P(z), P(ld), P(za), I64(b), P(w), ctypes.c_size_t(wb), P(0))
    assert fwd(_args(), 16, 16, 16, 0, -1, 16, ws) == -4
    assert fwd(None, 16, 16, 16, 0, B, 16, ws) == -1
    assert fwd(_args(bad=(4, 0)), 16, 16, 16, 0, B, 16, ws) == -1      # a NULL parameter
    assert fwd(_args(bad=(4, 4098)), 16, 16, 16, 0, B, 16, ws) == -6   # a misaligned one
    assert fwd(_args(), 0, 16, 16, 0, B, 16, ws) == -1                 # x
    assert fwd(_args(), 16, 16, 16, 0, B, 0, ws) == -1                 # workspace
    assert fwd(_args(), 16, 16, 16, 0, B, 16, ws - 4) == -1            # too small
    assert fwd(_args(), 18, 16, 16, 0, B, 16, ws) == -6
    assert fwd(_args(), 16, 18, 16, 0, B, 16, ws) == -6
    assert fwd(_args(), 16, 16, 16, 0, B, 18, ws) == -6
    assert fwd(_args(), 16, 16, 16, 0, B, 16, ws, d=300) == -3
    assert fwd(_args(), 16, 16, 16, 0, B, 16, ws, d=0) == -2
    assert fwd(_args(), 0, 0, 0, 0, 0, 0, 0) == 0                      # B == 0: a no-op


def test_loss_and_vjp_argument_validation_without_gpu():
    lib = _lib.lib()
    D, L, B = 3, 2, 8
    ws = workspace_bytes(D, L, B)
    sz = ctypes.c_size_t
    F = ctypes.c_float
    fl = lambda y, kind, terms, b=B: lib.cnf_planar_forward_loss(
        I32(D), I32(L), _args(), P(16), P(y), I32(kind), F(1.0), P(0), P(0), P(terms), I64(b),
        P(16), sz(ws), P(0))
    assert fl(0, 0, 16) == -1
    assert fl(16, 0, 0) == -1
    assert fl(20, 0, 16) == -6        # int64 labels: 8-byte alignment
    assert fl(16, 7, 16) == -2        # unknown loss kind
    assert fl(16, 0, 16, b=-3) == -4
    vjp = lambda gz, grads, dx: lib.cnf_planar_vjp(
        I32(D), I32(L), _args(), P(16), P(gz), P(0), P(0), P(grads), P(dx), I64(B), P(16), sz(ws),
        P(0))
    assert vjp(16, 0, 0) == -1
    assert vjp(18, 16, 0) == -6
    assert vjp(16, 16, 18) == -6
    lv = lambda y, terms, grads, kind=0: lib.cnf_planar_loss_vjp(
        I32(D), I32(L), _args(), P(16), P(y), I32(kind), F(1.0), F(1.0), P(terms), P(grads), P(0),
        I64(B), P(16), sz(ws), P(0))
    assert lv(0, 16, 16) == -1
    assert lv(16, 0, 16) == -1
    assert lv(16, 16, 0) == -1
    assert lv(16, 16, 16, kind=2) == -2


# ---- PlanarStack.compatible ---------------------------------------------------

def test_compatible():
    ok = [PlanarLayer(5) for _ in range(3)]
    assert PlanarStack.compatible(ok)
    assert PlanarStack.compatible(ok, "cpu")
    assert not PlanarStack.compatible(ok, "cuda:0")           # parameters sit on the host
    assert not PlanarStack.compatible([])
    assert not PlanarStack.compatible(ok + [PlanarLayer(4)])  # widths differ
    assert not PlanarStack.compatible(ok + [NvpCouplingLayer(5, [5, 5])])
    dbl = [PlanarLayer(5).double()]
    assert not PlanarStack.compatible(dbl)
    plain = PlanarLayer(params={"w": torch.rand(1, 5), "u": torch.rand(1, 5), "b": torch.rand(1)})
    assert PlanarStack.compatible([plain])                     # squeezed: b is 0-d
    strided = PlanarLayer(params={"w": torch.rand(10)[::2], "u": torch.rand(5), "b": torch.rand(1)})
    assert not PlanarStack.compatible([strided])
    st = PlanarStack(ok)
    assert st.dim == 5 and st.L == 3 and st.param_count() == 33
    assert [p.shape for p in st.param_tensors()[:3]] == [(5,), (5,), (1,)]
    assert [g.shape for g in st.split(torch.zeros(33))[:3]] == [(5,), (5,), (1,)]


def test_cpu_dispatch_is_untouched():
    """Host tensors never reach the native path; Flow.backward keeps raising."""
    from cnf_hip import engine
    flow = Flow([PlanarLayer(4) for _ in range(2)])
    n0 = engine.stats["planar_forward"]
    zs, ld = flow(torch.randn(6, 4))
    assert len(zs) == 2 and ld.shape == (6,) and engine.stats["planar_forward"] == n0
    with pytest.raises(ValueError, match="Flow inverse not tractable!"):
        flow.backward(zs[-1])


# ---- the CPU modules against the reference's record -----------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_cpu_flow_matches_reference(name):
    d = R.load(name)
    flow = R.build_flow(d)
    with torch.no_grad():
        zs, ld = flow(torch.from_numpy(d["x"]))
        z, ld2 = flow.transform(torch.from_numpy(d["x"]))
    assert ld.dim() == (0 if d["x"].shape[0] == 1 else 1)
    got = torch.stack(zs).numpy()
    assert rel_err(got, d["zs64"]) <= R.bar(d["floor_zs"])
    assert rel_err(ld.reshape(-1).numpy(), d["ld64"]) <= R.bar(d["floor_ld"])
    assert rel_err(got, d["zs"]) <= 1e-5 and torch.equal(z, zs[-1]) and torch.equal(ld, ld2)


def test_cpu_single_layer_matches_reference():
    d = R.load("d10n")
    flow = R.build_flow(d)
    x = torch.from_numpy(d["x"])
    with torch.no_grad():
        z, ld = flow.layers[0](x)
    zs, _, _ = R.forward(R.params_of(d)[:1], d["x"])
    assert rel_err(z.numpy(), zs[0]) <= 1e-5 and ld.shape == (777,)
    assert rel_err(z.numpy(), d["zs"][0]) <= 1e-6


def test_cpu_nan_positions_coincide():
    d = R.load("nan")
    with torch.no_grad():
        zs, ld = R.build_flow(d)(torch.from_numpy(d["x"]))
    got = torch.stack(zs).numpy()
    assert np.isnan(d["zs"][1]).all() and not np.isnan(d["zs"][0]).any()
    assert (np.isnan(got) == np.isnan(d["zs"])).all()
    assert np.isnan(ld.numpy()).all() and np.isnan(d["ld"]).all()
    zr, lr, _ = R.forward(R.params_of(d), d["x"])
    assert (np.isnan(zr) == np.isnan(d["zs64"])).all() and np.isnan(lr).all()


# ---- the float64 restatement against the reference's float64 autograd -----------

@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_float64_reference(name):
    d = R.load(name)
    params, B = R.params_of(d), d["x"].shape[0]
    zs, ld, _ = R.forward(params, d["x"])
    assert rel_err(zs, d["zs64"]) <= 1e-12
    assert rel_err(ld, d["ld64"]) <= 1e-12
    for kind, det in (("cal", 1.0), ("ce", float(d["det"]))):
        terms, grads, _ = R.loss_vjp(params, d["x"], d["y"], kind, det, grad_scale=1.0 / B)
        ref_loss = float(d["loss_%s_64" % kind])
        assert abs(terms[0] / B - ref_loss) <= 1e-12 * (abs(ref_loss) + 1)
        assert _grad_err(grads, d["g_%s_64" % kind]) <= 1e-12, (name, kind)


def test_restatement_upstream_gradients_match_autograd():
    """gz, gz_all, gld and dx of the hand reverse mode against torch autograd in
    float64 with random upstream weights on every output."""
    d = R.load("d17")
    flow = R.build_flow(d).double()
    rs = np.random.RandomState(5)
    L, B, D = d["zs"].shape
    gz_all, gld = rs.standard_normal((L, B, D)), rs.standard_normal(B)
    x = torch.from_numpy(d["x"]).double().requires_grad_(True)
    zs, ld = flow(x)
    obj = (torch.stack(zs) * torch.from_numpy(gz_all)).sum() + (ld * torch.from_numpy(gld)).sum()
    res = torch.autograd.grad(obj, list(flow.parameters()) + [x])
    ref = torch.cat([g.reshape(-1) for g in res[:-1]]).numpy()
    grads, dx = R.vjp(R.params_of(d), d["x"], gz_all=gz_all, gld=gld)
    assert _grad_err(grads, ref) <= 1e-12
    assert _grad_err(dx, res[-1].numpy()) <= 1e-12
