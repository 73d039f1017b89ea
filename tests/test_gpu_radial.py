"""The native radial-flow path (cnf_radial_*, csrc/cnf_radial.hip) on the GPU
against the reference's float64 record (tests/golden/radial) and the float64
restatement tests/_radial_ref.py.

Bars (the planar family's rules).  Outputs and probabilities: max(1e-5,
2 * floor) under _golden.rel_err, floor = the reference's own fp32-vs-float64
error recorded with the fixture.  Losses: 1e-5 relative.  Gradients:
max(1e-4, 2 * floor) under test_gpu_vjp._grad_err.  The score record: word for
word that of calibration_record(predict(...)).
"""
import numpy as np
import pytest
import torch

import _radial_ref as R
from _golden import rel_err
from cnf_hip import _lib, engine
from cnf_hip.metrics import calibration_record
from flows import flows as FL
from test_gpu_vjp import _grad_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_cache = {}


def fx(name):
    """(fixture arrays, Flow on the device, x on the device), loaded once."""
    if name not in _cache:
        d = R.load(name)
        _cache[name] = (d, R.build_flow(d, DEV), torch.from_numpy(d["x"]).to(DEV))
    return _cache[name]


def _flat_grads(flow):
    return torch.cat([p.grad.reshape(-1) for p in flow.parameters()]).cpu().numpy()


def _is_zero_logdet(ld):
    return torch.is_tensor(ld) and ld.dim() == 0 and ld.dtype == torch.float32 \
        and float(ld) == 0.0


# ---- forward --------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.GRAD_FIXTURES)
def test_forward_matches_float64_record(name):
    d, flow, x = fx(name)
    n0 = engine.stats["radial_forward"]
    with torch.no_grad():
        zs, ld = flow(x)
        z, ld2 = flow.transform(x)
    assert engine.stats["radial_forward"] == n0 + 2, "native path did not run"
    L, B, D = d["zs"].shape
    assert len(zs) == L and _is_zero_logdet(ld) and _is_zero_logdet(ld2)
    # zs: views of one [L, B, D] buffer
    assert all(zs[l].data_ptr() == zs[0].data_ptr() + 4 * l * B * D for l in range(L))
    got = torch.stack(zs).cpu().numpy()
    ez, et = rel_err(got, d["zs64"]), rel_err(z.cpu().numpy(), d["zs64"][-1])
    print("%s: zs %.2e transform %.2e (bar %.2e)" % (name, ez, et, R.bar(d["floor_zs"])))
    assert np.isfinite(got).all()
    assert ez <= R.bar(d["floor_zs"]) and et <= R.bar(d["floor_zs"])
    assert torch.equal(z, zs[-1])


@pytest.mark.parametrize("name", ["one", "d3", "d17", "d100"])
def test_single_layer_matches_restatement(name):
    """RadialLayer.forward alone: the same kernel with L = 1."""
    d, flow, x = fx(name)
    n0 = engine.stats["radial_forward"]
    with torch.no_grad():
        z, ld = flow.layers[0](x)
    assert engine.stats["radial_forward"] == n0 + 1 and _is_zero_logdet(ld)
    zs, _ = R.forward(R.params_of(d)[:1], d["x"])
    assert rel_err(z.cpu().numpy(), zs[0]) <= 1e-5


@pytest.mark.parametrize("B", [63, 64, 65])
def test_batch_slices(B):
    d, flow, x = fx("d10n")
    with torch.no_grad():
        zs, ld = flow(x[:B])
    assert rel_err(torch.stack(zs).cpu().numpy(), d["zs64"][:, :B]) <= R.bar(d["floor_zs"])


def _random_stack(rs, D, L):
    params = [((rs.standard_normal(D) * 0.5).astype(np.float32),
               (np.abs(rs.standard_normal(1)) * 0.5 + 0.1).astype(np.float32),
               (rs.standard_normal(1) * 0.5).astype(np.float32)) for _ in range(L)]
    d = {"Z0": np.stack([p[0] for p in params]), "A": np.concatenate([p[1] for p in params]),
         "Bv": np.concatenate([p[2] for p in params])}
    return params, R.build_flow(d, DEV)


@pytest.mark.parametrize("D,B", [(3, 256 * 1024 + 1), (17, 16 * 1024 + 1), (100, 4 * 1024 + 1)])
def test_grid_stride_one_row_past_the_cap(D, B):
    """One row past the forward grid cap of each lanes-per-row geometry (1024
    blocks of 256 / 16 / 4 rows): block 0 takes a second pass of one row; the
    reverse grid (256 blocks) is then in its fifth pass.  Sampled rows against
    the restatement (a >= 0.1, so a + r stays away from 0); a second call is
    bitwise equal."""
    L = 2
    rs = np.random.RandomState(21 + D)
    params, flow = _random_stack(rs, D, L)
    xh = rs.standard_normal((B, D)).astype(np.float32)
    yh = rs.randint(0, D, size=B)
    x, y = torch.from_numpy(xh).to(DEV), torch.from_numpy(yh).to(DEV)
    idx = np.concatenate([[0], np.sort(rs.choice(B - 2, 1024, replace=False)) + 1, [B - 1]])
    with torch.no_grad():
        zs, _ = flow(x)
        z, _ = flow.transform(x)
    zr, _ = R.forward(params, xh[idx])
    assert rel_err(torch.stack(zs)[:, idx].cpu().numpy(), zr) <= 1e-5
    assert rel_err(z[idx].cpu().numpy(), zr[-1]) <= 1e-5
    stack = flow._radial_stack()
    terms, grads, dx = stack.loss_and_grads(x, y, grad_scale=1.0 / B, need_dx=True)
    _, _, dxr = R.loss_vjp(params, xh[idx], yh[idx], "cal", 1.0 / B)
    assert _grad_err(dx[idx].cpu().numpy(), dxr) <= 1e-4
    tr, gr, _ = R.loss_vjp(params, xh, yh, "cal", 1.0 / B)
    assert rel_err(terms.cpu().numpy() / B, tr / B) <= 1e-5
    assert _grad_err(grads.cpu().numpy(), gr) <= 1e-4
    lp = np.log(np.arange(1, D + 1) / (D * (D + 1) / 2.0))
    probs = stack.predict(x, lp)
    assert rel_err(probs[idx].cpu().numpy(), R.predict(params, xh[idx], lp)) <= 1e-5
    with torch.no_grad():
        z2, _ = flow.transform(x)
    t2, g2, dx2 = stack.loss_and_grads(x, y, grad_scale=1.0 / B, need_dx=True)
    assert torch.equal(z, z2) and torch.equal(probs, stack.predict(x, lp))
    assert torch.equal(terms, t2) and torch.equal(grads, g2) and torch.equal(dx, dx2)
    rec = stack.score(x[:1 << 16], lp, y[:1 << 16], 15)
    assert torch.equal(rec, calibration_record(probs[:1 << 16], y[:1 << 16], 15))


# ---- special cases ------------------------------------------------------------------

def test_zero_radius_row_is_finite():
    """Row 5 of x is layer 0's z0 bit for bit: r == 0, no 0/0 anywhere."""
    d, flow, x = fx("zero")
    y = torch.from_numpy(d["y"]).to(DEV)
    B = x.shape[0]
    stack = flow._radial_stack()
    terms, grads, dx = stack.loss_and_grads(x, y, grad_scale=1.0 / B, need_dx=True)
    assert bool(torch.isfinite(grads).all()) and bool(torch.isfinite(dx).all())
    assert _grad_err(grads.cpu().numpy(), d["g_cal_64"]) <= R.bar(d["floor_g_cal"], 1e-4)
    _, _, dxr = R.loss_vjp(R.params_of(d), d["x"], d["y"], "cal", 1.0 / B)
    assert _grad_err(dx.cpu().numpy(), dxr) <= R.bar(d["floor_g_cal"], 1e-4)
    with torch.no_grad():
        zs, _ = flow(x)
    assert torch.equal(zs[0][5], x[5])               # beta * h * 0 added to the row


def test_singular_row_is_nan_and_the_others_agree():
    d, flow, x = fx("sing")
    with torch.no_grad():
        zs, _ = flow(x)
    got = torch.stack(zs).cpu().numpy()
    assert (np.isnan(got) == np.isnan(d["zs"])).all() and np.isnan(got[:, 5]).all()
    assert rel_err(got, d["zs64"]) <= R.bar(d["floor_zs"])    # NaNs coincide, the rest agrees


# ---- loss and gradients ---------------------------------------------------------------

@pytest.mark.parametrize("name", R.GRAD_FIXTURES)
@pytest.mark.parametrize("kind", ["cal", "ce"])
def test_loss_and_grads_match_reference_autograd(name, kind):
    d, flow, x = fx(name)
    y = torch.from_numpy(d["y"]).to(DEV)
    B = x.shape[0]
    k = _lib.LOSS_CAL if kind == "cal" else _lib.LOSS_CE
    stack = flow._radial_stack()
    n0, n1 = engine.stats["radial_loss_vjp"], engine.stats["radial_forward"]
    terms, grads, dx = stack.loss_and_grads(x, y, kind=k, grad_scale=1.0 / B, need_dx=True)
    t2, _ = stack.forward_loss(x, y, kind=k)
    assert engine.stats["radial_loss_vjp"] == n0 + 1 and engine.stats["radial_forward"] == n1 + 1
    ref = float(d["loss_%s_64" % kind])
    loss = float(terms[0]) / B
    ge = _grad_err(grads.cpu().numpy(), d["g_%s_64" % kind])
    gbar = R.bar(d["floor_g_%s" % kind], 1e-4)
    _, _, dxr = R.loss_vjp(R.params_of(d), d["x"], d["y"], kind, 1.0 / B)
    de = _grad_err(dx.cpu().numpy(), dxr)
    print("%s %s: loss %.3e grads %.2e (bar %.2e) dx %.2e" % (name, kind, abs(loss - ref), ge, gbar,
                                                             de))
    assert abs(loss - ref) <= 1e-5 * (abs(ref) + 1)
    assert abs(float(t2[0]) / B - ref) <= 1e-5 * (abs(ref) + 1)
    assert float(terms[2]) == 0.0 and float(t2[2]) == 0.0
    assert float(terms[1]) == float(terms[0]) and float(t2[1]) == float(t2[0])
    assert ge <= gbar and de <= gbar


@pytest.mark.parametrize("name", ["d10", "d17", "tape"])
def test_bitwise_repeatable(name):
    d, flow, x = fx(name)
    y = torch.from_numpy(d["y"]).to(DEV)
    stack = flow._radial_stack()
    a = [t.clone() for t in stack.loss_and_grads(x, y, need_dx=True)]
    b = stack.loss_and_grads(x, y, need_dx=True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    t1 = stack.forward_loss(x, y)[0].clone()
    assert torch.equal(t1, stack.forward_loss(x, y)[0])


# ---- autograd -------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["d3", "d10n", "d17", "d100", "tape"])
def test_autograd_matches_the_torch_op_path(name, monkeypatch):
    """Random upstream weights on every zs[l] (want_all) and on the final z
    only (transform): parameter gradients and dx of the native backward
    (cnf_radial_vjp) against torch autograd of the torch-op path on the same
    device."""
    d, flow, x = fx(name)
    L, B, D = d["zs"].shape
    rs = np.random.RandomState(11)
    w_all = torch.from_numpy(rs.standard_normal((L, B, D))).float().to(DEV)

    def grads_of(want_all):
        flow.zero_grad()
        xg = x.clone().requires_grad_(True)
        if want_all:
            zs, ld = flow(xg)
            obj = (torch.stack(zs) * w_all).sum()
        else:
            z, ld = flow.transform(xg)
            obj = (z * w_all[-1]).sum()
        obj.backward()
        out = _flat_grads(flow), xg.grad.cpu().numpy()
        flow.zero_grad()
        return out

    gbar = R.bar(d["floor_g_cal"], 1e-4)
    for want_all in (True, False):
        monkeypatch.setattr(FL, "RADIAL_NATIVE", True)
        n0 = engine.stats["radial_vjp"]
        gn, dxn = grads_of(want_all)
        assert engine.stats["radial_vjp"] == n0 + 1, "cnf_radial_vjp did not run"
        monkeypatch.setattr(FL, "RADIAL_NATIVE", False)
        gt, dxt = grads_of(want_all)
        assert engine.stats["radial_vjp"] == n0 + 1
        ge, de = _grad_err(gn, gt), _grad_err(dxn, dxt)
        print("%s want_all=%s: grads %.2e dx %.2e (bar %.2e)" % (name, want_all, ge, de, gbar))
        assert ge <= gbar and de <= gbar


def test_stale_parameter_raises():
    d, flow, x = fx("d3")
    flow.zero_grad()
    zs, _ = flow(x)
    with torch.no_grad():
        flow.layers[0].a.add_(0.0)                  # bumps the version counter
    with pytest.raises(RuntimeError, match="radial-layer parameter changed"):
        zs[-1].sum().backward()
    flow.zero_grad()


# ---- predict --------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.GRAD_FIXTURES)
def test_predict_matches_float64_record(name):
    d, flow, x = fx(name)
    stack = flow._radial_stack()
    lp = torch.as_tensor(d["log_priors"], dtype=torch.float32, device=DEV)
    n0 = engine.stats["radial_predict"]
    probs = stack.predict(x, lp)
    assert engine.stats["radial_predict"] == n0 + 1
    p = probs.cpu().numpy()
    ep, pb = rel_err(p, d["probs64"]), R.bar(d["floor_probs"])
    print("%s: probs %.2e (bar %.2e)" % (name, ep, pb))
    assert ep <= pb
    assert np.abs(p.astype(np.float64).sum(axis=1) - 1).max() <= 1e-6
    # the composition predict fuses: centre, run, torch's softmaxes
    xc = x - x.mean(dim=1, keepdim=True)
    z, _, _ = stack.run(xc)
    comp = torch.softmax(torch.log(torch.softmax(z, dim=1) + 1e-7) - lp, dim=1)
    assert rel_err(p, comp.cpu().numpy()) <= pb


def test_wrong_prior_count():
    d, flow, x = fx("d3")
    stack = flow._radial_stack()
    n0, n1 = engine.stats["radial_predict"], engine.stats["radial_score"]
    with pytest.raises(ValueError, match="log_priors must have 3 entries"):
        stack.predict(x, np.zeros(4))
    with pytest.raises(ValueError, match="log_priors must have 3 entries"):
        stack.score(x, np.zeros(2), torch.zeros(x.shape[0], dtype=torch.int64, device=DEV))
    assert engine.stats["radial_predict"] == n0 and engine.stats["radial_score"] == n1


# ---- score ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.GRAD_FIXTURES)
@pytest.mark.parametrize("bins", [1, 15, _lib.MAX_BINS])
def test_score_equals_predict_then_metrics(name, bins):
    d, flow, x = fx(name)
    stack = flow._radial_stack()
    lp = torch.as_tensor(d["log_priors"], dtype=torch.float32, device=DEV)
    y = torch.from_numpy(d["y"]).to(DEV)
    n0 = engine.stats["radial_score"]
    rec = stack.score(x, lp, y, bins)
    assert engine.stats["radial_score"] == n0 + 1
    want = calibration_record(stack.predict(x, lp), y, bins)
    assert rec.shape == (4 + 3 * bins,) and torch.equal(rec, want)
    assert int(rec[0]) == x.shape[0] and int(rec[1]) == 0
    # accumulating into a non-zero record adds
    acc = want.clone() + 7
    out = stack.score(x, lp, y, bins, record=acc)
    assert out.data_ptr() == acc.data_ptr() and torch.equal(acc, 2 * want + 7)


@pytest.mark.parametrize("name", ["d3", "d17", "d100"])
def test_score_labels_outside_the_range_are_invalid(name):
    d, flow, x = fx(name)
    stack = flow._radial_stack()
    D = x.shape[1]
    lp = torch.as_tensor(d["log_priors"], dtype=torch.float32, device=DEV)
    y = torch.from_numpy(d["y"]).to(DEV).clone()
    y[0], y[3], y[-1] = -1, D, D + 5
    rec = stack.score(x, lp, y, 15)
    assert int(rec[1]) == 3 and int(rec[0]) == x.shape[0] - 3
    assert torch.equal(rec, calibration_record(stack.predict(x, lp), y, 15))


# ---- the switch -------------------------------------------------------------------------

def test_switch_off_takes_no_native_launch(monkeypatch):
    d, flow, x = fx("d10")
    monkeypatch.setattr(FL, "RADIAL_NATIVE", False)
    n0 = {k: v for k, v in engine.stats.items() if k.startswith("radial_")}
    with torch.no_grad():
        zs, ld = flow(x)
        z, _ = flow.transform(x)
        z1, _ = flow.layers[0](x)
    assert {k: v for k, v in engine.stats.items() if k.startswith("radial_")} == n0
    assert _is_zero_logdet(ld)
    assert rel_err(torch.stack(zs).cpu().numpy(), d["zs64"]) <= R.bar(d["floor_zs"])
    assert torch.equal(z, zs[-1]) and torch.equal(z1, zs[0])
