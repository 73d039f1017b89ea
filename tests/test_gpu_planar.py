"""The native planar-flow path (cnf_planar_*, csrc/cnf_planar.hip) on the GPU
against the reference's float64 record (tests/golden/planar) and the float64
restatement tests/_planar_ref.py.

Bars.  Outputs: max(1e-5, 2 * floor) under _golden.rel_err, floor = the
reference's own fp32-vs-float64 error recorded with the fixture (the rule
tests/test_gpu_parity.py uses for the inverse).  Losses: 1e-5 relative.
Gradients: max(1e-4, 2 * floor) under test_gpu_vjp._grad_err.
"""
import numpy as np
import pytest
import torch

import _planar_ref as R
from _golden import rel_err
from cnf_hip import _lib, engine
from conftest import RECORDS
from flows import flows as FL
from flows._factory import PlanarFlow
from test_gpu_vjp import _grad_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURES = ["one", "d3", "d10", "d10n", "d17", "d100", "tape"]
_cache = {}


def fx(name):
    """(fixture arrays, Flow on the device, x on the device), loaded once."""
    if name not in _cache:
        d = R.load(name)
        _cache[name] = (d, R.build_flow(d, DEV), torch.from_numpy(d["x"]).to(DEV))
    return _cache[name]


def _flat_grads(flow):
    return torch.cat([p.grad.reshape(-1) for p in flow.parameters()]).cpu().numpy()


@pytest.mark.parametrize("name", FIXTURES)
def test_forward_matches_float64_record(name):
    d, flow, x = fx(name)
    n0 = engine.stats["planar_forward"]
    with torch.no_grad():
        zs, ld = flow(x)
        z, ld2 = flow.transform(x)
    assert engine.stats["planar_forward"] == n0 + 2, "native path did not run"
    L, B, D = d["zs"].shape
    assert len(zs) == L and ld.dim() == (0 if B == 1 else 1)
    # zs: views of one [L, B, D] buffer
    assert all(zs[l].data_ptr() == zs[0].data_ptr() + 4 * l * B * D for l in range(L))
    got = torch.stack(zs).cpu().numpy()
    ez, el = rel_err(got, d["zs64"]), rel_err(ld.reshape(-1).cpu().numpy(), d["ld64"])
    et = rel_err(z.cpu().numpy(), d["zs64"][-1])
    print("%s: zs %.2e (bar %.2e) ld %.2e (bar %.2e) transform %.2e"
          % (name, ez, R.bar(d["floor_zs"]), el, R.bar(d["floor_ld"]), et))
    RECORDS.setdefault("planar_parity", []).append(
        {"fixture": name, "zs": ez, "zs_bar": R.bar(d["floor_zs"]), "ld": el,
         "ld_bar": R.bar(d["floor_ld"])})
    assert ez <= R.bar(d["floor_zs"]) and et <= R.bar(d["floor_zs"])
    assert el <= R.bar(d["floor_ld"])
    assert torch.equal(z, zs[-1]) and torch.equal(ld, ld2)


@pytest.mark.parametrize("name", ["one", "d3", "d17", "d100"])
def test_single_layer_matches_restatement(name):
    """PlanarLayer.forward alone: the same kernel with L = 1."""
    d, flow, x = fx(name)
    n0 = engine.stats["planar_forward"]
    with torch.no_grad():
        z, ld = flow.layers[0](x)
    assert engine.stats["planar_forward"] == n0 + 1
    zs, lr, _ = R.forward(R.params_of(d)[:1], d["x"])
    assert ld.dim() == (0 if x.shape[0] == 1 else 1)
    assert rel_err(z.cpu().numpy(), zs[0]) <= 1e-5
    assert rel_err(ld.reshape(-1).cpu().numpy(), lr) <= 1e-5


@pytest.mark.parametrize("B", [63, 64, 65])
def test_batch_slices(B):
    d, flow, x = fx("d10n")
    with torch.no_grad():
        zs, ld = flow(x[:B])
    assert rel_err(torch.stack(zs).cpu().numpy(), d["zs64"][:, :B]) <= R.bar(d["floor_zs"])
    assert rel_err(ld.cpu().numpy(), d["ld64"][:B]) <= R.bar(d["floor_ld"])


def test_nan_positions_coincide():
    d, flow, x = fx("nan")
    with torch.no_grad():
        zs, ld = flow(x)
    got = torch.stack(zs).cpu().numpy()
    assert (np.isnan(got) == np.isnan(d["zs"])).all()
    assert rel_err(got, d["zs64"]) <= 1e-5                  # NaNs coincide, the rest agrees
    assert np.isnan(ld.cpu().numpy()).all()


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("kind", ["cal", "ce"])
def test_loss_and_grads_match_reference_autograd(name, kind):
    d, flow, x = fx(name)
    y = torch.from_numpy(d["y"]).to(DEV)
    B = x.shape[0]
    det = 1.0 if kind == "cal" else float(d["det"])
    k = _lib.LOSS_CAL if kind == "cal" else _lib.LOSS_CE
    stack = flow._planar_stack()
    terms, grads, dx = stack.loss_and_grads(x, y, kind=k, det=det, grad_scale=1.0 / B, need_dx=True)
    t2, _, _ = stack.forward_loss(x, y, kind=k, det=det)
    ref = float(d["loss_%s_64" % kind])
    loss = float(terms[0]) / B
    ge = _grad_err(grads.cpu().numpy(), d["g_%s_64" % kind])
    gbar = R.bar(d["floor_g_%s" % kind], 1e-4)
    _, _, dxr = R.loss_vjp(R.params_of(d), d["x"], d["y"], kind, det, 1.0 / B)
    de = _grad_err(dx.cpu().numpy(), dxr)
    print("%s %s: loss %.3e grads %.2e (bar %.2e) dx %.2e" % (name, kind, abs(loss - ref), ge, gbar,
                                                             de))
    RECORDS.setdefault("planar_grads", []).append(
        {"fixture": name, "kind": kind, "loss_rel": abs(loss - ref) / (abs(ref) + 1), "grads": ge,
         "bar": gbar, "dx": de})
    assert abs(loss - ref) <= 1e-5 * (abs(ref) + 1)
    assert abs(float(t2[0]) / B - ref) <= 1e-5 * (abs(ref) + 1)
    assert ge <= gbar and de <= gbar


@pytest.mark.parametrize("name", ["d3", "d10n", "d17", "tape"])
def test_plain_backward_runs_native_vjp(name):
    """loss.backward() through Flow.forward: the autograd Function's backward
    is cnf_planar_vjp (gz_all and gld arrive from autograd)."""
    d, flow, x = fx(name)
    y = torch.from_numpy(d["y"]).to(DEV)
    flow.zero_grad()
    n0 = engine.stats["planar_vjp"]
    zs, ld = flow(x)
    ce = torch.log(torch.softmax(zs[-1], dim=1).gather(1, y.view(-1, 1)) + 1e-7)
    loss = -torch.mean(ce.squeeze() + ld)
    loss.backward()
    assert engine.stats["planar_vjp"] == n0 + 1, "cnf_planar_vjp did not run"
    ref = float(d["loss_cal_64"])
    assert abs(loss.item() - ref) <= 1e-5 * (abs(ref) + 1)
    assert _grad_err(_flat_grads(flow), d["g_cal_64"]) <= R.bar(d["floor_g_cal"], 1e-4)
    flow.zero_grad()


@pytest.mark.parametrize("name", ["d10n", "d17", "d100", "tape"])
def test_upstream_gradients_match_float64_autograd(name):
    """Random upstream weights on every zs[l] and on the log-det; parameter
    gradients and dx against CPU float64 autograd of the same modules."""
    d, flow, x = fx(name)
    L, B, D = d["zs"].shape
    rs = np.random.RandomState(11)
    gz_all, gld = rs.standard_normal((L, B, D)), rs.standard_normal(B)
    f64 = R.build_flow(d).double()
    x64 = torch.from_numpy(d["x"]).double().requires_grad_(True)
    zs, ld = f64(x64)
    obj = (torch.stack(zs) * torch.from_numpy(gz_all)).sum() + (ld * torch.from_numpy(gld)).sum()
    res = torch.autograd.grad(obj, list(f64.parameters()) + [x64])
    ref = torch.cat([g.reshape(-1) for g in res[:-1]]).numpy()
    flow.zero_grad()
    xg = x.clone().requires_grad_(True)
    zs, ld = flow(xg)
    obj = (torch.stack(zs) * torch.from_numpy(gz_all).float().to(DEV)).sum() \
        + (ld * torch.from_numpy(gld).float().to(DEV)).sum()
    obj.backward()
    # the project's gradient bar (the fixtures' floors are all below half of it)
    ge, de = _grad_err(_flat_grads(flow), ref), _grad_err(xg.grad.cpu().numpy(), res[-1].numpy())
    print("%s: grads %.2e dx %.2e" % (name, ge, de))
    assert ge <= 1e-4 and de <= 1e-4
    flow.zero_grad()
    # final-output gradient only (gz), through transform
    xg = x.clone().requires_grad_(True)
    z, _ = flow.transform(xg)
    (z * torch.from_numpy(gz_all[-1]).float().to(DEV)).sum().backward()
    gr, dxr = R.vjp(R.params_of(d), d["x"], gz=gz_all[-1])
    assert _grad_err(_flat_grads(flow), gr) <= 1e-4 and _grad_err(xg.grad.cpu().numpy(), dxr) <= 1e-4
    flow.zero_grad()


@pytest.mark.parametrize("name", ["d10", "d17", "tape"])
def test_bitwise_repeatable(name):
    d, flow, x = fx(name)
    y = torch.from_numpy(d["y"]).to(DEV)
    stack = flow._planar_stack()
    a = stack.loss_and_grads(x, y, need_dx=True)
    a = [t.clone() for t in a]
    b = stack.loss_and_grads(x, y, need_dx=True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    with torch.no_grad():
        z1, l1 = flow.transform(x)
        z2, l2 = flow.transform(x)
    assert torch.equal(z1, z2) and torch.equal(l1, l2)
    t1 = stack.forward_loss(x, y)[0].clone()
    assert torch.equal(t1, stack.forward_loss(x, y)[0])


def test_grid_stride_one_row_past_the_cap():
    """256 rows per pass x 1024 blocks (forward) + 1; the reverse grid (256
    blocks) is then in its fifth pass."""
    B, D, L = 256 * 1024 + 1, 3, 2
    rs = np.random.RandomState(21)
    params = [((rs.standard_normal(D) * 0.5).astype(np.float32),
               (rs.standard_normal(D) * 0.5).astype(np.float32),
               (rs.standard_normal(1) * 0.5).astype(np.float32)) for _ in range(L)]
    d = {"W": np.stack([p[0] for p in params]), "U": np.stack([p[1] for p in params]),
         "Bv": np.concatenate([p[2] for p in params])}
    flow = R.build_flow(d, DEV)
    xh = rs.standard_normal((B, D)).astype(np.float32)
    yh = rs.randint(0, D, size=B)
    x, y = torch.from_numpy(xh).to(DEV), torch.from_numpy(yh).to(DEV)
    with torch.no_grad():
        zs, ld = flow(x)
    zr, lr, _ = R.forward(params, xh)
    assert rel_err(torch.stack(zs).cpu().numpy(), zr) <= 1e-5
    assert rel_err(ld.cpu().numpy(), lr) <= 1e-5
    terms, grads, dx = flow._planar_stack().loss_and_grads(x, y, grad_scale=1.0 / B, need_dx=True)
    tr, gr, dxr = R.loss_vjp(params, xh, yh, "cal", 1.0, 1.0 / B)
    assert rel_err(terms.cpu().numpy() / B, tr / B) <= 1e-5
    assert _grad_err(grads.cpu().numpy(), gr) <= 1e-4
    assert _grad_err(dx.cpu().numpy(), dxr) <= 1e-4


# ---- the calibrator -----------------------------------------------------------------

def _fit(native, batch_size, monkeypatch):
    from calibrators import TorchFlowCalibrator
    monkeypatch.setattr(FL, "PLANAR_NATIVE", native)
    rs = np.random.RandomState(31)
    N, D = 300, 3
    logits = 2.0 * rs.standard_normal((N, D))
    target = np.eye(D)[rs.randint(0, D, size=N)]
    torch.manual_seed(7)
    cal = TorchFlowCalibrator(PlanarFlow, logits, target, layers=4, epochs=5,
                              batch_size=batch_size, dev=torch.device(DEV))
    hist = {k: np.array([float(v) for v in cal.history[k]]) for k in cal.history}
    return cal, hist


@pytest.mark.parametrize("batch_size", [300, 128])
def test_calibrator_fit_matches_torch_op_path(batch_size, monkeypatch):
    """TorchFlowCalibrator on the fused kernels against the same seeded run on
    the torch ops (CNF_PLANAR_NATIVE=0).

    Bound.  A gradient within 1e-4 of its largest element (the bar above)
    perturbs Adam's normalised step lr * m / sqrt(v) of an element whose
    gradient is at least 1/100 of the largest by at most 2 * 100 * 1e-4 of lr;
    compounded over the steps: steps * lr * 2e-2 per parameter.  (A wrong
    gradient term moves a parameter by ~lr per step, 50 times this.)  The
    history then differs by at most that times the L1 norm of the torch-op
    path's loss gradient, plus the 1e-5 bar of the evaluation itself."""
    n0 = engine.stats["planar_loss_vjp"]
    cal_n, hist_n = _fit(True, batch_size, monkeypatch)
    steps = 5 * -(-300 // batch_size)
    assert engine.stats["planar_loss_vjp"] == n0 + steps, "the fused training step did not run"
    n1 = engine.stats["planar_loss_vjp"]
    cal_t, hist_t = _fit(False, batch_size, monkeypatch)
    assert engine.stats["planar_loss_vjp"] == n1
    pbar = steps * 1e-3 * 2e-2
    pn = torch.cat([p.detach().reshape(-1) for p in cal_n.flow.parameters()]).numpy()
    pt = torch.cat([p.detach().reshape(-1) for p in cal_t.flow.parameters()]).numpy()
    pdiff = float(np.max(np.abs(pn - pt)))
    # L1 norm of the torch-op path's loss gradient at its final parameters (CPU)
    flow = cal_t.flow
    flow.zero_grad()
    z, ld = flow(cal_t.logits)
    ce = torch.log(torch.softmax(z, dim=1).gather(1, cal_t.target.view(-1, 1)) + 1e-7)
    (-torch.mean(ce.squeeze() + ld)).backward()
    g1 = float(sum(p.grad.abs().sum() for p in flow.parameters()))
    flow.zero_grad()
    hdiff = {k: float(np.max(np.abs(hist_n[k] - hist_t[k]) / (np.abs(hist_t[k]) + 1)))
             for k in hist_n}
    hbar = 1e-5 + pbar * g1
    print("batch %d: params %.2e (bar %.2e) history %s (bar %.2e)" % (batch_size, pdiff, pbar,
                                                                      hdiff, hbar))
    RECORDS.setdefault("planar_calibrator", []).append(
        {"batch_size": batch_size, "steps": steps, "param_diff": pdiff, "param_bar": pbar,
         "history_diff": hdiff, "history_bar": hbar})
    assert len(hist_n["loss"]) == 5 and np.isfinite(hist_n["loss"]).all()
    assert pdiff <= pbar
    assert max(hdiff.values()) <= hbar


# ---- 2^20 rows ----------------------------------------------------------------------------

def test_million_rows_once_each():
    """2^20 x 10, L = 10: forward, forward-loss and loss-vjp once each, against
    the restatement on a fixed 4096-row sample, and repeatable."""
    B, D, L = 1 << 20, 10, 10
    rs = np.random.RandomState(41)
    params = [((rs.standard_normal(D) * 0.5).astype(np.float32),
               (rs.standard_normal(D) * 0.5).astype(np.float32),
               (rs.standard_normal(1) * 0.5).astype(np.float32)) for _ in range(L)]
    d = {"W": np.stack([p[0] for p in params]), "U": np.stack([p[1] for p in params]),
         "Bv": np.concatenate([p[2] for p in params])}
    flow = R.build_flow(d, DEV)
    g = torch.Generator(device="cpu").manual_seed(42)
    xc = torch.randn(B, D, generator=g)
    yc = torch.randint(0, D, (B,), generator=g)
    x, y = xc.to(DEV), yc.to(DEV)
    idx = np.arange(4096) * 251 + 17            # fixed sample, spread over the batch
    stack = flow._planar_stack()
    with torch.no_grad():
        z, ld = flow.transform(x)
    terms, _, _ = stack.forward_loss(x, y)
    terms2, grads, dx = stack.loss_and_grads(x, y, grad_scale=1.0 / B, need_dx=True)
    torch.cuda.synchronize()
    zr, lr, _ = R.forward(params, xc.numpy()[idx])
    assert rel_err(z[idx].cpu().numpy(), zr[-1]) <= 1e-5
    assert rel_err(ld[idx].cpu().numpy(), lr) <= 1e-5
    # the sums: from the device's own per-row outputs, added in float64
    zs_all = z.cpu().numpy().astype(np.float64)
    tr, _, _ = R.loss_terms(zs_all, ld.cpu().numpy().astype(np.float64), yc.numpy(), "cal")
    assert rel_err(terms.cpu().numpy() / B, np.array(tr) / B) <= 1e-5
    # the two entry points add in different grids: the same sums to fp32 rounding
    assert rel_err(terms2.cpu().numpy() / B, np.array(tr) / B) <= 1e-5
    # dx is per row: the sample against the restatement
    _, _, dxr = R.loss_vjp(params, xc.numpy()[idx], yc.numpy()[idx], "cal", 1.0, 1.0 / B)
    assert _grad_err(dx[idx].cpu().numpy(), dxr) <= 1e-4
    # the parameter gradient sums every row: the restatement over the whole batch
    _, gr, _ = R.loss_vjp(params, xc.numpy(), yc.numpy(), "cal", 1.0, 1.0 / B)
    assert _grad_err(grads.cpu().numpy(), gr) <= 1e-4
    t3, g3, dx3 = stack.loss_and_grads(x, y, grad_scale=1.0 / B, need_dx=True)
    assert torch.equal(terms2, t3) and torch.equal(grads, g3) and torch.equal(dx, dx3)
