"""The native mixed row-wise path (cnf_mixed_*, csrc/cnf_mixed.hip) on the GPU
against the reference's float64 record (tests/golden/mixed) and the float64
restatement tests/_mixed_ref.py.

Bars (tests/_rowsweep.py's, not re-tuned): rel_err <= OUT_BAR = 1e-5 for
outputs, log-dets and loss terms; grad_err <= GRAD_BAR = 1e-4 for gradients
and dx; probabilities under _rowsweep.probs_err with max(1e-5, twice the fp32
CPU path's own error, which the fixture records); the score record word for
word that of calibration_record(predict(...)).  `contract`'s layer outputs are
held step by step by the affine test's rule: OUT_BAR where the reference's own
fp32 floor is <= OUT_COND, else twice that floor.
"""
import numpy as np
import pytest
import torch

import _affine_ref as AR
import _mixed_ref as M
import _planar_ref as PR
import _radial_ref as RR
from _golden import rel_err
from _rowsweep import GRAD_BAR, OUT_BAR, OUT_COND, probs_err
from cnf_hip import _lib, engine
from cnf_hip.metrics import calibration_record
from cnf_hip.mixed import MixedStack
from flows import flows as FL
from test_gpu_vjp import _grad_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_cache = {}


def fx(name):
    """(fixture arrays, layers, Flow on the device, x on the device), loaded once."""
    if name not in _cache:
        d = M.load(name)
        ps = M.params_of(d)
        _cache[name] = (d, ps, M.build_flow(ps, DEV), torch.from_numpy(d["x"]).to(DEV))
    return _cache[name]


def _flat_grads(flow):
    return torch.cat([p.grad.reshape(-1) for p in flow.parameters()]).cpu().numpy()


_FAMILIES = ("mixed_", "planar_", "radial_", "affine_")


def _stats():
    return {k: v for k, v in engine.stats.items() if k.startswith(_FAMILIES)}


def _moved(before):
    return {k: v - before[k] for k, v in _stats().items() if v != before[k]}


def _stack(flow, x):
    cls = FL._row_class(list(flow.layers), x)
    assert cls is MixedStack
    return flow._row_stack(cls, list(flow.layers))


def _rows(ld, B):
    return np.asarray(ld, dtype=np.float64).reshape(-1) * np.ones(B)


# ---- forward ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", M.FIXTURES)
def test_forward_matches_float64_record(name):
    d, ps, flow, x = fx(name)
    n0 = _stats()
    with torch.no_grad():
        zs, ld = flow(x)
        z, ld2 = flow.transform(x)
    assert _moved(n0) == {"mixed_forward": 2}, "one mixed launch per call, no per-family launch"
    L, B, D = d["zs"].shape
    cpu_ld = M.build_flow(ps)(torch.from_numpy(d["x"]))[1]
    want = {"ar": (1,), "one": (1,)}.get(name, (B,))
    assert len(zs) == L and tuple(ld.shape) == tuple(ld2.shape) == tuple(cpu_ld.shape) == want
    assert tuple(d["ld"].shape) == want
    assert ld.dtype == torch.float32 and ld.device == x.device
    assert all(zs[l].data_ptr() == zs[0].data_ptr() + 4 * l * B * D for l in range(L))
    got = torch.stack(zs).cpu().numpy()
    ez, el = rel_err(got, d["zs64"]), rel_err(ld.cpu().numpy(), d["ld64"])
    print("%s: zs %.2e ld %.2e" % (name, ez, el))
    assert np.isfinite(got).all() and el <= OUT_BAR
    for k in range(L):    # step by step (the affine test's rule)
        floor = float(d["floor_zs_step"][k])
        bar = OUT_BAR if floor <= OUT_COND else 2.0 * floor
        ek = rel_err(got[k], d["zs64"][k])
        print("%s: zs[%d] %.2e (floor %.2e, bar %.2e)" % (name, k, ek, floor, bar))
        assert ek <= bar
    assert torch.equal(z, zs[-1]) and torch.equal(ld, ld2)
    with torch.no_grad():
        zs2, ld3 = flow(x)
    assert torch.equal(torch.stack(zs2), torch.stack(zs)) and torch.equal(ld3, ld)


def test_mixed_flow_factory_runs_fused():
    d, ps, _, x = fx("pra")
    flow = M.build_flow(ps, DEV, factory=True)
    n0 = _stats()
    with torch.no_grad():
        z, ld = flow(x)
    assert _moved(n0) == {"mixed_forward": 1} and ld.shape == (x.shape[0],)
    assert rel_err(z.cpu().numpy(), d["zs64"][-1]) <= OUT_BAR


@pytest.mark.parametrize("B", [63, 64, 65])
def test_batch_slices(B):
    d, ps, flow, x = fx("d10")
    with torch.no_grad():
        zs, ld = flow(x[:B])
    assert rel_err(torch.stack(zs).cpu().numpy(), d["zs64"][:, :B]) <= OUT_BAR
    assert rel_err(ld.cpu().numpy(), d["ld64"][:B]) <= OUT_BAR


# ---- loss and gradients ---------------------------------------------------------------

@pytest.mark.parametrize("name", M.FIXTURES)
@pytest.mark.parametrize("kind", ["cal", "ce"])
def test_loss_and_grads_match_reference_autograd(name, kind):
    d, ps, flow, x = fx(name)
    y = torch.from_numpy(d["y"]).to(DEV)
    B = x.shape[0]
    k, det = (_lib.LOSS_CAL, 1.0) if kind == "cal" else (_lib.LOSS_CE, float(d["det"]))
    stack = _stack(flow, x)
    n0 = _stats()
    terms, grads, dx = stack.loss_and_grads(x, y, kind=k, det=det, grad_scale=1.0 / B,
                                            need_dx=True)
    t2, z2, ld2 = stack.forward_loss(x, y, kind=k, det=det, want_outputs=True)
    assert _moved(n0) == {"mixed_loss_vjp": 1, "mixed_forward": 1}
    tr, gr, dxr = M.loss_vjp(ps, d["x"], d["y"], kind, det, 1.0 / B)
    ref = float(d["loss_%s_64" % kind])
    et = max(rel_err(terms.cpu().numpy() / B, tr / B), rel_err(t2.cpu().numpy() / B, tr / B))
    ge = _grad_err(grads.cpu().numpy(), d["g_%s_64" % kind])
    de = _grad_err(dx.cpu().numpy(), dxr)
    print("%s %s: terms %.2e grads %.2e dx %.2e" % (name, kind, et, ge, de))
    assert abs(float(terms[0]) / B - ref) <= OUT_BAR * (abs(ref) + 1)
    assert et <= OUT_BAR and ge <= GRAD_BAR and de <= GRAD_BAR
    assert ld2.shape == (B,) and rel_err(z2.cpu().numpy(), d["zs64"][-1]) <= OUT_BAR
    assert rel_err(ld2.cpu().numpy(), _rows(d["ld64"], B)) <= OUT_BAR
    a = stack.loss_and_grads(x, y, kind=k, det=det, grad_scale=1.0 / B, need_dx=True)
    assert torch.equal(a[0], terms) and torch.equal(a[1], grads) and torch.equal(a[2], dx)
    assert torch.equal(stack.forward_loss(x, y, kind=k, det=det)[0], t2)
    # dx off: the same gradient
    b = stack.loss_and_grads(x, y, kind=k, det=det, grad_scale=1.0 / B, need_dx=False)
    assert b[2] is None and torch.equal(b[1], grads)


@pytest.mark.parametrize("name", M.FIXTURES)
def test_vjp_matches_restatement(name):
    """Final-only and all-layer upstream, with and without gld, dx on and off."""
    d, ps, flow, x = fx(name)
    L, B, D = d["zs"].shape
    rs = np.random.RandomState(11)
    gz_all = rs.standard_normal((L, B, D)).astype(np.float32)
    gld = rs.standard_normal(B).astype(np.float32)
    stack = _stack(flow, x)
    ga, gl = torch.from_numpy(gz_all).to(DEV), torch.from_numpy(gld).to(DEV)
    n0 = _stats()
    dx1, g1 = stack.vjp(x, ga[-1], None, False, True)
    dx2, g2 = stack.vjp(x, ga, gl, True, True)
    dx3, g3 = stack.vjp(x, ga[-1], gl, False, True)
    dx4, g4 = stack.vjp(x, ga, None, True, False)
    assert _moved(n0) == {"mixed_vjp": 4} and dx4 is None
    r1, rdx1 = M.vjp(ps, d["x"], gz=gz_all[-1])
    r2, rdx2 = M.vjp(ps, d["x"], gz_all=gz_all, gld=gld)
    r3, rdx3 = M.vjp(ps, d["x"], gz=gz_all[-1], gld=gld)
    r4, _ = M.vjp(ps, d["x"], gz_all=gz_all)
    errs = (_grad_err(g1.cpu().numpy(), r1), _grad_err(dx1.cpu().numpy(), rdx1),
            _grad_err(g2.cpu().numpy(), r2), _grad_err(dx2.cpu().numpy(), rdx2),
            _grad_err(g3.cpu().numpy(), r3), _grad_err(dx3.cpu().numpy(), rdx3),
            _grad_err(g4.cpu().numpy(), r4))
    print("%s: %s" % (name, " ".join("%.2e" % e for e in errs)))
    assert max(errs) <= GRAD_BAR
    dx5, g5 = stack.vjp(x, ga, gl, True, True)
    assert torch.equal(g2, g5) and torch.equal(dx2, dx5)


# ---- autograd -------------------------------------------------------------------------

@pytest.mark.parametrize("name", M.FIXTURES)
def test_autograd_matches_the_cpu_flow(name):
    """Random upstream weights on every zs[l] (want_all) and on the final z
    only (transform), each with a gradient on the log-det in the loop's shape:
    the native backward (cnf_mixed_vjp) against torch autograd of the same flow
    on the CPU."""
    d, ps, flow, x = fx(name)
    cflow = M.build_flow(ps)
    L, B, D = d["zs"].shape
    rs = np.random.RandomState(11)
    w_all = torch.from_numpy(rs.standard_normal((L, B, D))).float()
    w_ld = torch.from_numpy(rs.standard_normal(d["ld"].shape)).float()

    def grads_of(f, xin, dev, want_all):
        f.zero_grad()
        xg = xin.clone().requires_grad_(True)
        if want_all:
            zs, ld = f(xg)
            obj = (torch.stack(zs) * w_all.to(dev)).sum()
        else:
            z, ld = f.transform(xg)
            obj = (z * w_all[-1].to(dev)).sum()
        assert tuple(ld.shape) == tuple(d["ld"].shape) and ld.requires_grad
        (obj + (ld * w_ld.to(dev)).sum()).backward()
        out = _flat_grads(f), xg.grad.cpu().numpy()
        f.zero_grad()
        return out

    for want_all in (True, False):
        n0 = _stats()
        gn, dxn = grads_of(flow, x, DEV, want_all)
        assert _moved(n0) == {"mixed_forward": 1, "mixed_vjp": 1}
        gt, dxt = grads_of(cflow, torch.from_numpy(d["x"]), "cpu", want_all)
        ge, de = _grad_err(gn, gt), _grad_err(dxn, dxt)
        print("%s want_all=%s: grads %.2e dx %.2e" % (name, want_all, ge, de))
        assert ge <= GRAD_BAR and de <= GRAD_BAR


def test_stale_parameter_raises():
    d, ps, flow, x = fx("pra")
    flow.zero_grad()
    zs, _ = flow(x)
    with torch.no_grad():
        flow.layers[0].w.add_(0.0)                  # bumps the version counter
    with pytest.raises(RuntimeError, match="mixed-layer parameter changed"):
        zs[-1].sum().backward()
    flow.zero_grad()


def test_empty_batch():
    d, ps, flow, x = fx("pra")
    stack = _stack(flow, x[:2])
    n0 = _stats()
    with torch.no_grad():
        zs, ld = flow(x[:0])
    assert _moved(n0) == {"mixed_forward": 1}
    assert len(zs) == 3 and zs[-1].shape == (0, 3) and ld.shape == (0,)
    y0 = torch.zeros(0, dtype=torch.int64, device=DEV)
    grads = torch.full((stack.param_count(),), 7.0, device=DEV)
    terms = torch.full((3,), 7.0, device=DEV)
    stack.loss_and_grads(x[:0], y0, grads_out=grads, terms_out=terms)
    assert not bool(grads.any()) and not bool(terms.any())
    dx, g = stack.vjp(x[:0], None, None, False, True)
    assert dx.shape == (0, 3) and not bool(g.any())
    assert stack.predict(x[:0], d["log_priors"]).shape == (0, 3)
    rec = stack.score(x[:0], d["log_priors"], y0, 15)
    assert not bool(rec.any())


# ---- predict and score ------------------------------------------------------------------

@pytest.mark.parametrize("name", M.FIXTURES)
def test_predict_matches_float64_record(name):
    d, ps, flow, x = fx(name)
    stack = _stack(flow, x)
    lp = torch.as_tensor(d["log_priors"], dtype=torch.float32, device=DEV)
    n0 = _stats()
    probs, ld = stack.predict(x, lp, want_logdet=True)
    assert _moved(n0) == {"mixed_predict": 1}
    p = probs.cpu().numpy()
    bar = max(OUT_BAR, 2.0 * probs_err(d["probs"], d["probs64"]))
    ep, er = probs_err(p, d["probs64"]), probs_err(p, M.predict(ps, d["x"], d["log_priors"]))
    xc = d["x"].astype(np.float64) - d["x"].astype(np.float64).mean(axis=1, keepdims=True)
    el = rel_err(ld.cpu().numpy(), M.forward(ps, xc)[1])
    print("%s: probs %.2e (restated %.2e, bar %.2e) ld %.2e" % (name, ep, er, bar, el))
    assert ep <= bar and er <= bar and el <= OUT_BAR
    assert np.abs(p.astype(np.float64).sum(axis=1) - 1).max() <= 1e-6
    assert torch.equal(probs, stack.predict(x, lp))


@pytest.mark.parametrize("name", M.FIXTURES)
@pytest.mark.parametrize("bins", [1, 15])
def test_score_equals_predict_then_metrics(name, bins):
    d, ps, flow, x = fx(name)
    stack = _stack(flow, x)
    lp = torch.as_tensor(d["log_priors"], dtype=torch.float32, device=DEV)
    y = torch.from_numpy(d["y"]).to(DEV)
    n0 = _stats()
    rec = stack.score(x, lp, y, bins)
    assert _moved(n0) == {"mixed_score": 1}
    want = calibration_record(stack.predict(x, lp), y, bins)
    assert rec.shape == (4 + 3 * bins,) and torch.equal(rec, want)
    assert int(rec[0]) == x.shape[0] and int(rec[1]) == 0
    acc = want.clone() + 7
    out = stack.score(x, lp, y, bins, record=acc)
    assert out.data_ptr() == acc.data_ptr() and torch.equal(acc, 2 * want + 7)


@pytest.mark.parametrize("name", ["pra", "d17", "d100"])
def test_score_labels_outside_the_range_are_invalid(name):
    d, ps, flow, x = fx(name)
    stack = _stack(flow, x)
    D = x.shape[1]
    lp = torch.as_tensor(d["log_priors"], dtype=torch.float32, device=DEV)
    y = torch.from_numpy(d["y"]).to(DEV).clone()
    y[0], y[3], y[-1] = -1, D, D + 5
    rec = stack.score(x, lp, y, 15)
    assert int(rec[1]) == 3 and int(rec[0]) == x.shape[0] - 3
    assert torch.equal(rec, calibration_record(stack.predict(x, lp), y, 15))


# ---- the switch, and what stays on the loop ------------------------------------------------

@pytest.mark.parametrize("name", ["pra", "d17", "ar", "one"])
def test_switch_off_takes_the_layer_loop(name, monkeypatch):
    d, ps, flow, x = fx(name)
    with torch.no_grad():
        fz, fld = flow(x)
    monkeypatch.setattr(FL, "MIXED_NATIVE", False)
    n0 = _stats()
    with torch.no_grad():
        zs, ld = flow(x)
    moved = _moved(n0)
    assert moved and not any(k.startswith("mixed_") for k in moved), moved
    assert tuple(ld.shape) == tuple(fld.shape) == tuple(d["ld"].shape)
    assert rel_err(torch.stack(zs).cpu().numpy(), d["zs64"]) <= OUT_BAR
    assert rel_err(ld.cpu().numpy(), d["ld64"]) <= OUT_BAR
    assert rel_err(torch.stack(fz).cpu().numpy(), torch.stack(zs).cpu().numpy()) <= OUT_BAR
    assert rel_err(fld.cpu().numpy(), ld.cpu().numpy()) <= OUT_BAR


def test_orders_the_loop_rejects_stay_on_the_loop():
    """P,A on one row: the loop cannot add the affine [1] into the planar 0-d
    log-det and raises; so does the flow on the device, with no mixed launch."""
    d, ps, flow, x = fx("contract")
    n0 = _stats()
    with pytest.raises(RuntimeError):
        with torch.no_grad():
            flow(x[:1])
    assert not any(k.startswith("mixed_") for k in _moved(n0))


# ---- single-kind stacks through the mixed ABI ------------------------------------------------

def _single(kind, D, L, B, seed):
    rs = np.random.RandomState(seed)
    ps = M.draw_params(rs, D, kind * L)
    x = (2.0 * rs.standard_normal((B, D))).astype(np.float32)
    y = rs.randint(0, D, size=B).astype(np.int64)
    flow = M.build_flow(ps, DEV)
    return ps, x, y, MixedStack(list(flow.layers)), flow


@pytest.mark.parametrize("kind,D,L", [("P", 5, 4), ("R", 5, 4), ("A", 5, 4), ("P", 20, 12),
                                      ("R", 20, 12), ("A", 70, 3)])
def test_single_kind_stack_against_its_family(kind, D, L):
    """A stack of one kind is valid at the ABI: against that family's own
    float64 restatement."""
    B = 133
    ps, x, y, stack, flow = _single(kind, D, L, B, 40 + D + L)
    fam = [p for _, p in ps]
    xt, yt = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    n0 = _stats()
    fin, ld, allt = stack.run(xt, want_all=True)
    terms, grads, dx = stack.loss_and_grads(xt, yt, kind=_lib.LOSS_CE, det=0.7,
                                            grad_scale=1.0 / B, need_dx=True)
    assert _moved(n0) == {"mixed_forward": 1, "mixed_loss_vjp": 1}
    if kind == "P":
        zs, rld, _ = PR.forward(fam, x)
        tr, gr, dxr = PR.loss_vjp(fam, x, y, "ce", 0.7, 1.0 / B)
    elif kind == "R":
        zs, _ = RR.forward(fam, x)
        rld = np.zeros(B)
        tr, gr, dxr = RR.loss_vjp(fam, x, y, "ce", 1.0 / B)
    else:
        zs, rld = AR.forward(fam, x)
        tr, gr, dxr = AR.loss_vjp(fam, x, y, "ce", 0.7, 1.0 / B)
    errs = (rel_err(allt.cpu().numpy(), zs), rel_err(ld.cpu().numpy(), _rows(rld, B)),
            rel_err(terms.cpu().numpy() / B, np.asarray(tr) / B))
    ge, de = _grad_err(grads.cpu().numpy(), gr), _grad_err(dx.cpu().numpy(), dxr)
    print("%s d%d l%d: %s grads %.2e dx %.2e" % (kind, D, L, " ".join("%.2e" % e for e in errs),
                                                   ge, de))
    assert max(errs) <= OUT_BAR and ge <= GRAD_BAR and de <= GRAD_BAR
    # the flow of one family still takes its own stack
    n0 = _stats()
    with torch.no_grad():
        flow(xt)
    assert _moved(n0) == {M.FAMILY[kind] + "_forward": 1}
