"""Reverse mode of every narrow-table shape against float64 CPU autograd.

For each of the 18 shapes of kVTable (cnf_vjp.hip; 15 of them also in
kV2Part{A,B,C}, cnf_vjp2_*.hip), six kink-guarded stacks at sigma 0.2:

  A  RealNVP, L=3            k_vjp2 [scale][.][no perm]   (k_vjp outside the V2 table)
  B  RealNVP, L=4, flip      k_vjp2 [scale][.][perm]
  C  NICE,    L=4            k_vjp2 [NICE][.][no perm]
  D  NICE,    L=3, flip      k_vjp2 [NICE][.][perm]
  E  shift=False, L=3, flip  k_vjp (no shift net: never k_vjp2)
  F  RealNVP, L=9            k_vjp (L > kV2LMax), layerwise where its LDS passes 64 KB

[.] = [generic, loss]: the generic objective runs the generic instantiation,
loss_and_grads the loss one.  Every test first asserts vjp_kernel_name(), so a
dispatch change cannot quietly turn the sweep into a test of another kernel.

Batches 1 and 131: one full 128-row k_vjp2 tile plus an odd tail (the last
lane's pair holds one row), three 64-row k_vjp blocks.  Bars: the project's
1e-4 on every parameter gradient and dx (tests/test_gpu_vjp._grad_err), loss
sums within 1e-5 x the sum of the per-row magnitudes.  The kink guard
(_sweep.guarded_flow) picks the seed on the CPU from the float64 reference; no
row is excluded from any comparison."""
import copy

import numpy as np
import pytest
import torch

import _sweep
from cnf_hip import engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BMAX = 131
BS = (1, BMAX)
GRAD_TOL = 1e-4

# name -> (L, scale, shift, flip)
STACKS = {
    "A": (3, True, True, False),
    "B": (4, True, True, True),
    "C": (4, False, True, False),
    "D": (3, False, True, True),
    "E": (3, True, False, True),
    "F": (9, True, True, False),
}


def _expected_path(D, hidden, name):
    L, scale, shift, _ = STACKS[name]
    return _sweep.expected_vjp_path(D, hidden, L, scale, shift)


_cache = {}


def _case(D, hidden, name):
    key = (D, tuple(hidden), name)
    if key not in _cache:
        L, scale, shift, flip = STACKS[name]
        x, y, _ = _sweep.inputs(BMAX, D, seed=1)
        flow, seed, x = _sweep.guarded_flow(D, L, hidden, x, scale, shift, flip)
        g = torch.Generator().manual_seed(2)
        w = torch.randn(L, BMAX, D, generator=g)
        wl = torch.randn(BMAX, generator=g)
        _cache.clear()  # one case alive at a time
        _cache[key] = dict(flow=flow, f64=_sweep.ref64(flow), fg=copy.deepcopy(flow).to(DEV),
                           x=x, y=y, w=w, wl=wl, seed=seed, L=L)
    return _cache[key]


def _params(f):
    return [(k, p) for k, p in f.named_parameters() if p.requires_grad]


def _ref_generic(c, B, every_layer):
    f = c["f64"]
    f.zero_grad()
    x = c["x"][:B].double().requires_grad_(True)
    zs, ld = f(x)
    w, wl = c["w"][:, :B].double(), c["wl"][:B].double()
    obj = (ld.reshape(-1) * wl).sum()
    for l in (range(c["L"]) if every_layer else [c["L"] - 1]):
        obj = obj + (zs[l] * w[l]).sum()
    obj.backward()
    return [p.grad.numpy().copy() for _, p in _params(f)], x.grad.numpy().copy()


def _gpu_generic(c, B, every_layer):
    fg = c["fg"]
    fg.zero_grad()
    x = c["x"][:B].to(DEV).requires_grad_(True)
    w, wl = c["w"][:, :B].to(DEV), c["wl"][:B].to(DEV)
    n0, t0 = engine.stats["vjp"], engine.stats["torch_ops"]
    if every_layer:
        zs, ld = fg(x)
        obj = (ld.reshape(-1) * wl).sum()
        for l in range(c["L"]):
            obj = obj + (zs[l] * w[l]).sum()
    else:  # final output only: the upstream gradient arrives as gz, not gz_all
        z, ld = fg.transform(x)
        obj = (ld.reshape(-1) * wl).sum() + (z * w[-1]).sum()
    obj.backward()
    assert engine.stats["vjp"] == n0 + 1 or engine.stats["torch_ops"] > t0, "native vjp did not run"
    return [p.grad.cpu().numpy() for _, p in _params(fg)], x.grad.cpu().numpy()


def _worst(got, ref, names):
    worst, where = 0.0, None
    for g, r, k in zip(got, ref, names):
        assert np.isfinite(g).all(), k
        e = _sweep.grad_err(g, r)
        if e > worst:
            worst, where = e, k
    return worst, where


CASES = [(D, h, s) for D, h, _ in _sweep.NARROW for s in STACKS]
IDS = ["%s-%s" % (_sweep.shape_id(D, h), s) for D, h, s in CASES]


@pytest.mark.parametrize("D,hidden,name", CASES, ids=IDS)
def test_generic_vjp_against_float64_autograd(D, hidden, name):
    c = _case(D, hidden, name)
    path = _expected_path(D, hidden, name)
    stack = c["fg"]._native_stack()
    assert stack.vjp_kernel_name() == path
    names = [k for k, _ in _params(c["fg"])]
    worst_all = 0.0
    for B in BS:
        for every_layer in (True, False):
            ref_g, ref_dx = _ref_generic(c, B, every_layer)
            got_g, got_dx = _gpu_generic(c, B, every_layer)
            wg, where = _worst(got_g, ref_g, names)
            wx = _sweep.grad_err(got_dx, ref_dx)
            print("%s %s B=%d every_layer=%d seed=%d: grads %.2e (%s) dx %.2e"
                  % (_sweep.shape_id(D, hidden), name, B, every_layer, c["seed"], wg, where, wx))
            assert wg <= GRAD_TOL, (B, every_layer, wg, where)
            assert wx <= GRAD_TOL, (B, every_layer, wx)
            worst_all = max(worst_all, wg, wx)
    _sweep.record({"test": "vjp_generic", "D": D, "hidden": hidden, "stack": name, "path": path,
                   "seed": c["seed"], "grad_err": worst_all})


@pytest.mark.parametrize("D,hidden,name", CASES, ids=IDS)
def test_loss_and_grads_against_float64_autograd(D, hidden, name):
    c = _case(D, hidden, name)
    path = _expected_path(D, hidden, name)
    fg, f = c["fg"], c["f64"]
    stack = fg._native_stack()
    assert stack.vjp_kernel_name() == path
    names = [k for k, _ in _params(fg)]
    worst_all = 0.0
    for B in BS:
        xg, yg = c["x"][:B].to(DEV), c["y"][:B].to(DEV)
        for kind in (0, 1):
            f.zero_grad()
            x = c["x"][:B].double().requires_grad_(True)
            zs, ld = f(x)
            rows = _sweep.loss_rows64(zs[-1], ld.reshape(-1), c["y"][:B], kind, 0.5)
            (rows[0].sum() / B).backward()
            ref_g = [p.grad.numpy().copy() for _, p in _params(f)]
            rows = rows.detach().numpy()
            n0 = engine.stats["loss_vjp"]
            terms, grads, dx = stack.loss_and_grads(xg, yg, kind=kind, det=0.5,
                                                    grad_scale=1.0 / B, need_dx=True)
            assert engine.stats["loss_vjp"] == n0 + 1
            t2, g2, dx2 = stack.loss_and_grads(xg, yg, kind=kind, det=0.5, grad_scale=1.0 / B,
                                               need_dx=True)
            assert torch.equal(terms, t2) and torch.equal(grads, g2) and torch.equal(dx, dx2), \
                "two calls differ"
            got_t = terms.double().cpu().numpy()
            bound = 1e-5 * np.abs(rows).sum(axis=1)
            terr = np.abs(got_t - rows.sum(axis=1))
            got_g = [g.cpu().numpy() for g in stack.split(grads)]
            wg, where = _worst(got_g, ref_g, names)
            wx = _sweep.grad_err(dx.cpu().numpy(), x.grad.numpy())
            print("%s %s B=%d kind=%d seed=%d: terms err %s bound %s grads %.2e (%s) dx %.2e"
                  % (_sweep.shape_id(D, hidden), name, B, kind, c["seed"], terr, bound, wg, where,
                     wx))
            assert np.all(terr <= bound), (B, kind, got_t, rows.sum(axis=1), bound)
            assert wg <= GRAD_TOL, (B, kind, wg, where)
            assert wx <= GRAD_TOL, (B, kind, wx)
            worst_all = max(worst_all, wg, wx)
    _sweep.record({"test": "vjp_loss", "D": D, "hidden": hidden, "stack": name, "path": path,
                   "seed": c["seed"], "grad_err": worst_all})
