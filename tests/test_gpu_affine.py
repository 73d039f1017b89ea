"""The native affine-constant path (cnf_affine_*, csrc/cnf_affine.hip) on the
GPU against the reference's float64 record (tests/golden/affine) and the
float64 restatement tests/_affine_ref.py.

Bars (tests/_rowsweep.py's, not re-tuned): rel_err <= OUT_BAR = 1e-5 for
outputs, log-dets, probabilities and loss terms; grad_err <= GRAD_BAR = 1e-4
for gradients and dx; the score record word for word that of
calibration_record(predict(...)).  Every fixture's recorded fp32-vs-float64
floors lie within a quarter of these (tests/test_affine_cpu.py), the last step
of `contract`'s inverse excepted (test_inverse_matches_float64_record).
"""
import numpy as np
import pytest
import torch

import _affine_ref as A
from _golden import rel_err
from _rowsweep import GRAD_BAR, OUT_BAR, OUT_COND
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
        d = A.load(name)
        _cache[name] = (d, A.build_flow(d, DEV), torch.from_numpy(d["x"]).to(DEV))
    return _cache[name]


def _flat_grads(flow):
    return torch.cat([p.grad.reshape(-1) for p in flow.parameters()]).cpu().numpy()


def _affine_stats():
    return {k: v for k, v in engine.stats.items() if k.startswith("affine_")}


def _moved(before):
    return {k: v - before[k] for k, v in _affine_stats().items() if v != before[k]}


# ---- forward and inverse --------------------------------------------------------------

@pytest.mark.parametrize("name", A.FIXTURES)
def test_forward_matches_float64_record(name):
    d, flow, x = fx(name)
    n0 = _affine_stats()
    with torch.no_grad():
        zs, ld = flow(x)
        z, ld2 = flow.transform(x)
    assert _moved(n0) == {"affine_forward": 2}, "native path did not run"
    L, B, D = d["zs"].shape
    cpu_ld = A.build_flow(d)(torch.from_numpy(d["x"]))[1]
    assert len(zs) == L and ld.shape == ld2.shape == cpu_ld.shape == (1,)
    assert ld.dtype == torch.float32 and ld.device == x.device
    assert all(zs[l].data_ptr() == zs[0].data_ptr() + 4 * l * B * D for l in range(L))
    got = torch.stack(zs).cpu().numpy()
    ez, el = rel_err(got, d["zs64"]), rel_err(ld.cpu().numpy(), d["ld64"])
    print("%s: zs %.2e ld %.2e" % (name, ez, el))
    assert np.isfinite(got).all() and ez <= OUT_BAR and el <= OUT_BAR
    assert torch.equal(z, zs[-1]) and torch.equal(ld, ld2)
    with torch.no_grad():
        zs2, ld3 = flow(x)
    assert torch.equal(torch.stack(zs2), torch.stack(zs)) and torch.equal(ld3, ld)


@pytest.mark.parametrize("name", A.FIXTURES)
def test_inverse_matches_float64_record(name):
    d, flow, x = fx(name)
    z = torch.from_numpy(d["zs"][-1]).to(DEV)          # the reference's fp32 z
    n0 = _affine_stats()
    with torch.no_grad():
        xs, ild = flow.backward(z)
        xf, ild2 = flow.inverse_transform(z)
    assert _moved(n0) == {"affine_inverse": 2}
    assert len(xs) == d["xs"].shape[0] and ild.shape == ild2.shape == (1,)
    got = torch.stack(xs).cpu().numpy()
    el = rel_err(ild.cpu().numpy(), d["ild64"])
    # Step by step: a step enters at OUT_BAR when the reference's own fp32 value
    # lies within a quarter of it of the float64 one.  Undoing `contract`'s
    # layer 0 multiplies what the earlier steps left by exp(6): that one step
    # is held to the project's rule for such outputs, twice the reference's own
    # fp32-vs-float64 error.
    for k in range(got.shape[0]):
        floor = rel_err(d["xs"][k], d["xs64"][k])
        bar = OUT_BAR if floor <= OUT_COND else 2.0 * floor
        ex = rel_err(got[k], d["xs64"][k])
        print("%s: xs[%d] %.2e (floor %.2e, bar %.2e)" % (name, k, ex, floor, bar))
        assert (bar == OUT_BAR) == (name != "contract" or k < got.shape[0] - 1)
        assert ex <= bar
    print("%s: ild %.2e" % (name, el))
    assert el <= OUT_BAR
    assert torch.equal(xf, xs[-1]) and torch.equal(ild, ild2)


@pytest.mark.parametrize("name", [n for n in A.FIXTURES if n != "contract"])
def test_inverse_of_forward_is_the_input(name):
    d, flow, x = fx(name)
    assert float(d["floor_rt"]) <= OUT_COND              # admitted: fp32 itself returns to x
    with torch.no_grad():
        z, ld = flow.transform(x)
        xb, ild = flow.inverse_transform(z)
    assert rel_err(xb.cpu().numpy(), d["x"]) <= OUT_BAR
    assert abs(float(ld) + float(ild)) <= OUT_BAR * (abs(float(ld)) + 1)


@pytest.mark.parametrize("name", ["one", "d3", "d17", "d100"])
def test_single_layer_launches(name):
    """AffineConstantLayer.forward / .backward alone: the same kernels, L = 1."""
    d, flow, x = fx(name)
    n0 = _affine_stats()
    with torch.no_grad():
        z, ld = flow.layers[0](x)
        xb, ild = flow.layers[0].backward(z)
    assert _moved(n0) == {"affine_forward": 1, "affine_inverse": 1}
    assert ld.shape == (1,) and ild.shape == (1,)
    zs, ldr = A.forward(A.params_of(d)[:1], d["x"])
    assert rel_err(z.cpu().numpy(), zs[0]) <= OUT_BAR and abs(float(ld) - ldr) <= OUT_BAR
    assert rel_err(xb.cpu().numpy(), d["x"]) <= OUT_BAR and float(ild) == -float(ld)


@pytest.mark.parametrize("B", [63, 64, 65])
def test_batch_slices(B):
    d, flow, x = fx("d10")
    with torch.no_grad():
        zs, ld = flow(x[:B])
    assert rel_err(torch.stack(zs).cpu().numpy(), d["zs64"][:, :B]) <= OUT_BAR and ld.shape == (1,)


# ---- loss and gradients ---------------------------------------------------------------

@pytest.mark.parametrize("name", A.FIXTURES)
@pytest.mark.parametrize("kind", ["cal", "ce"])
def test_loss_and_grads_match_reference_autograd(name, kind):
    d, flow, x = fx(name)
    y = torch.from_numpy(d["y"]).to(DEV)
    B = x.shape[0]
    k, det = (_lib.LOSS_CAL, 1.0) if kind == "cal" else (_lib.LOSS_CE, float(d["det"]))
    stack = _stack(flow, x)
    n0 = _affine_stats()
    terms, grads, dx = stack.loss_and_grads(x, y, kind=k, det=det, grad_scale=1.0 / B,
                                            need_dx=True)
    t2, z2, ld2 = stack.forward_loss(x, y, kind=k, det=det, want_outputs=True)
    assert _moved(n0) == {"affine_loss_vjp": 1, "affine_forward": 1}
    tr, gr, dxr = A.loss_vjp(A.params_of(d), d["x"], d["y"], kind, det, 1.0 / B)
    ref = float(d["loss_%s_64" % kind])
    et = max(rel_err(terms.cpu().numpy() / B, tr / B), rel_err(t2.cpu().numpy() / B, tr / B))
    ge = _grad_err(grads.cpu().numpy(), d["g_%s_64" % kind])
    de = _grad_err(dx.cpu().numpy(), dxr)
    print("%s %s: terms %.2e grads %.2e dx %.2e" % (name, kind, et, ge, de))
    assert abs(float(terms[0]) / B - ref) <= OUT_BAR * (abs(ref) + 1)
    assert et <= OUT_BAR and ge <= GRAD_BAR and de <= GRAD_BAR
    assert ld2.shape == (1,) and rel_err(z2.cpu().numpy(), d["zs64"][-1]) <= OUT_BAR
    a = stack.loss_and_grads(x, y, kind=k, det=det, grad_scale=1.0 / B, need_dx=True)
    assert torch.equal(a[0], terms) and torch.equal(a[1], grads) and torch.equal(a[2], dx)
    assert torch.equal(stack.forward_loss(x, y, kind=k, det=det)[0], t2)


def _stack(flow, x):
    cls = FL._row_class(list(flow.layers), x)
    assert cls is not None and cls.family == "affine"
    return flow._row_stack(cls, list(flow.layers))


@pytest.mark.parametrize("name", A.FIXTURES)
def test_vjp_matches_restatement(name):
    """gz only, and gz_all with the one-number gld."""
    d, flow, x = fx(name)
    L, B, D = d["zs"].shape
    rs = np.random.RandomState(11)
    gz_all = rs.standard_normal((L, B, D)).astype(np.float32)
    gld = rs.standard_normal(1).astype(np.float32)
    stack = _stack(flow, x)
    params = A.params_of(d)
    n0 = _affine_stats()
    dx1, g1 = stack.vjp(x, torch.from_numpy(gz_all[-1]).to(DEV), None, False, True)
    dx2, g2 = stack.vjp(x, torch.from_numpy(gz_all).to(DEV), torch.from_numpy(gld).to(DEV), True,
                        True)
    assert _moved(n0) == {"affine_vjp": 2}
    r1, rdx1 = A.vjp(params, d["x"], gz=gz_all[-1])
    r2, rdx2 = A.vjp(params, d["x"], gz_all=gz_all, gld=gld)
    errs = (_grad_err(g1.cpu().numpy(), r1), _grad_err(dx1.cpu().numpy(), rdx1),
            _grad_err(g2.cpu().numpy(), r2), _grad_err(dx2.cpu().numpy(), rdx2))
    print("%s: %s" % (name, " ".join("%.2e" % e for e in errs)))
    assert max(errs) <= GRAD_BAR
    dx3, g3 = stack.vjp(x, torch.from_numpy(gz_all).to(DEV), torch.from_numpy(gld).to(DEV), True,
                        True)
    assert torch.equal(g2, g3) and torch.equal(dx2, dx3)


# ---- autograd -------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["d3", "d10", "d17", "d100", "tape", "centre"])
def test_autograd_matches_the_torch_op_path(name, monkeypatch):
    """Random upstream weights on every zs[l] (want_all) and on the final z
    only (transform), each with a gradient on the [1] log-det: the native
    backward (cnf_affine_vjp) against torch autograd of the torch-op path on
    the same device."""
    d, flow, x = fx(name)
    L, B, D = d["zs"].shape
    rs = np.random.RandomState(11)
    w_all = torch.from_numpy(rs.standard_normal((L, B, D))).float().to(DEV)
    w_ld = torch.from_numpy(rs.standard_normal(1)).float().to(DEV)

    def grads_of(want_all):
        flow.zero_grad()
        xg = x.clone().requires_grad_(True)
        if want_all:
            zs, ld = flow(xg)
            obj = (torch.stack(zs) * w_all).sum()
        else:
            z, ld = flow.transform(xg)
            obj = (z * w_all[-1]).sum()
        assert ld.shape == (1,) and ld.requires_grad
        (obj + (ld * w_ld).sum()).backward()
        out = _flat_grads(flow), xg.grad.cpu().numpy()
        flow.zero_grad()
        return out

    for want_all in (True, False):
        monkeypatch.setattr(FL, "AFFINE_NATIVE", True)
        n0 = _affine_stats()
        gn, dxn = grads_of(want_all)
        assert _moved(n0) == {"affine_forward": 1, "affine_vjp": 1}
        monkeypatch.setattr(FL, "AFFINE_NATIVE", False)
        gt, dxt = grads_of(want_all)
        assert _moved(n0) == {"affine_forward": 1, "affine_vjp": 1}
        ge, de = _grad_err(gn, gt), _grad_err(dxn, dxt)
        print("%s want_all=%s: grads %.2e dx %.2e" % (name, want_all, ge, de))
        assert ge <= GRAD_BAR and de <= GRAD_BAR


def test_stale_parameter_raises():
    d, flow, x = fx("d3")
    flow.zero_grad()
    zs, _ = flow(x)
    with torch.no_grad():
        flow.layers[0].s.add_(0.0)                  # bumps the version counter
    with pytest.raises(RuntimeError, match="affine-layer parameter changed"):
        zs[-1].sum().backward()
    flow.zero_grad()


def test_empty_batch_keeps_the_logdet_and_its_gradient():
    """B == 0 launches nothing, yet the log-det and its gradient do not depend
    on the rows: the host side forms both, as the torch ops do."""
    d, flow, x = fx("d3")
    cflow = A.build_flow(d)
    cflow.zero_grad()
    czs, cld = cflow(torch.from_numpy(d["x"][:0]))
    (2.0 * cld).sum().backward()
    flow.zero_grad()
    n0 = _affine_stats()
    zs, ld = flow(x[:0])
    assert _moved(n0) == {"affine_forward": 1} and ld.shape == cld.shape == (1,)
    assert len(zs) == len(czs) and zs[-1].shape == (0, 3)
    assert rel_err(ld.detach().cpu().numpy(), cld.detach().numpy()) <= OUT_BAR
    (2.0 * ld).sum().backward()
    assert _moved(n0) == {"affine_forward": 1, "affine_vjp": 1}
    for ly, cly in zip(flow.layers, cflow.layers):                   # 2 on every s, nothing on t
        assert torch.equal(ly.s.grad.cpu(), cly.s.grad) and float(cly.s.grad.min()) == 2.0
        assert cly.t.grad is None and (ly.t.grad is None or not bool(ly.t.grad.any()))
    flow.zero_grad()


# ---- predict and score ------------------------------------------------------------------

@pytest.mark.parametrize("name", A.FIXTURES)
def test_predict_matches_float64_record(name):
    d, flow, x = fx(name)
    stack = _stack(flow, x)
    lp = torch.as_tensor(d["log_priors"], dtype=torch.float32, device=DEV)
    n0 = _affine_stats()
    probs = stack.predict(x, lp)
    assert _moved(n0) == {"affine_predict": 1}
    p = probs.cpu().numpy()
    ep = rel_err(p, d["probs64"])
    print("%s: probs %.2e" % (name, ep))
    assert ep <= OUT_BAR
    assert np.abs(p.astype(np.float64).sum(axis=1) - 1).max() <= 1e-6
    assert torch.equal(probs, stack.predict(x, lp))


@pytest.mark.parametrize("name", [n for n in A.FIXTURES if n != "one"])
@pytest.mark.parametrize("bins", [1, 15])
def test_score_equals_predict_then_metrics(name, bins):
    d, flow, x = fx(name)
    stack = _stack(flow, x)
    lp = torch.as_tensor(d["log_priors"], dtype=torch.float32, device=DEV)
    y = torch.from_numpy(d["y"]).to(DEV)
    n0 = _affine_stats()
    rec = stack.score(x, lp, y, bins)
    assert _moved(n0) == {"affine_score": 1}
    want = calibration_record(stack.predict(x, lp), y, bins)
    assert rec.shape == (4 + 3 * bins,) and torch.equal(rec, want)
    assert int(rec[0]) == x.shape[0] and int(rec[1]) == 0
    acc = want.clone() + 7
    out = stack.score(x, lp, y, bins, record=acc)
    assert out.data_ptr() == acc.data_ptr() and torch.equal(acc, 2 * want + 7)


def test_score_of_a_single_row():
    d, flow, x = fx("one")
    stack = _stack(flow, x)
    lp = torch.as_tensor(d["log_priors"], dtype=torch.float32, device=DEV)
    y = torch.from_numpy(d["y"]).to(DEV)
    for bins in (1, 15):
        assert torch.equal(stack.score(x, lp, y, bins),
                           calibration_record(stack.predict(x, lp), y, bins))


@pytest.mark.parametrize("name", ["d3", "d17", "d100"])
def test_score_labels_outside_the_range_are_invalid(name):
    d, flow, x = fx(name)
    stack = _stack(flow, x)
    D = x.shape[1]
    lp = torch.as_tensor(d["log_priors"], dtype=torch.float32, device=DEV)
    y = torch.from_numpy(d["y"]).to(DEV).clone()
    y[0], y[3], y[-1] = -1, D, D + 5
    rec = stack.score(x, lp, y, 15)
    assert int(rec[1]) == 3 and int(rec[0]) == x.shape[0] - 3
    assert torch.equal(rec, calibration_record(stack.predict(x, lp), y, 15))


# ---- what stays on the torch ops -----------------------------------------------------------

def test_switch_off_takes_no_native_launch(monkeypatch):
    d, flow, x = fx("d10")
    monkeypatch.setattr(FL, "AFFINE_NATIVE", False)
    n0 = _affine_stats()
    with torch.no_grad():
        zs, ld = flow(x)
        z, _ = flow.transform(x)
        z1, _ = flow.layers[0](x)
        xs, ild = flow.backward(z)
    assert _affine_stats() == n0 and ld.shape == (1,) and ild.shape == (1,)
    cz, cld = A.build_flow(d)(torch.from_numpy(d["x"]))
    assert rel_err(torch.stack(zs).cpu().numpy(), torch.stack(cz).detach().numpy()) <= OUT_BAR
    assert rel_err(ld.cpu().numpy(), cld.detach().numpy()) <= OUT_BAR
    assert torch.equal(z, zs[-1]) and torch.equal(z1, zs[0])


def test_layer_without_scale_stays_on_torch_ops():
    """A scale=False layer (its log-det has B entries) and the flow that holds
    it: no fused stack; the flow's other layer may launch on its own."""
    from flows.flows import AffineConstantLayer, Flow
    torch.manual_seed(3)
    flow = Flow([AffineConstantLayer(4, scale=False), AffineConstantLayer(4)])
    with torch.no_grad():
        for p in flow.parameters():
            p.normal_(0, 0.3)
    x = torch.randn(9, 4)
    with torch.no_grad():
        cz, cld = flow(x)
        cs, csl = flow.layers[0](x)
    flow.to(DEV)
    n0 = _affine_stats()
    with torch.no_grad():
        s1, sl = flow.layers[0](x.to(DEV))
    assert _affine_stats() == n0                     # the scale=False layer itself
    assert sl.shape == csl.shape == (9,) and rel_err(s1.cpu().numpy(), cs.numpy()) <= OUT_BAR
    with torch.no_grad():
        zs, ld = flow(x.to(DEV))
    assert _moved(n0) in ({}, {"affine_forward": 1})
    assert ld.shape == cld.shape == (9,)
    assert rel_err(torch.stack(zs).cpu().numpy(), torch.stack(cz).numpy()) <= OUT_BAR
    assert rel_err(ld.cpu().numpy(), cld.numpy()) <= OUT_BAR


def test_inverse_under_autograd_stays_on_torch_ops():
    d, flow, x = fx("d3")
    z = torch.from_numpy(d["zs"][-1]).to(DEV).requires_grad_(True)
    flow.zero_grad()
    n0 = _affine_stats()
    xs, ild = flow.backward(z)
    (xs[-1].sum() + ild.sum()).backward()
    assert _affine_stats() == n0 and ild.shape == (1,)
    cflow = A.build_flow(d)
    zc = torch.from_numpy(d["zs"][-1]).requires_grad_(True)
    cxs, cild = cflow.backward(zc)
    (cxs[-1].sum() + cild.sum()).backward()
    assert rel_err(xs[-1].detach().cpu().numpy(), cxs[-1].detach().numpy()) <= OUT_BAR
    assert _grad_err(z.grad.cpu().numpy(), zc.grad.numpy()) <= GRAD_BAR
    assert _grad_err(_flat_grads(flow), _flat_grads(cflow)) <= GRAD_BAR
    flow.zero_grad()
