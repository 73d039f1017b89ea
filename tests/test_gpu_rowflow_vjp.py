"""Every reverse-mode instantiation of the planar and radial families on the
GPU against float64, and sentinel guards around their workspace and outputs.

launch_bwd splits k_<family>_bwd<lpr, cpl> three ways -- tape and per-lane
accumulators in registers (rega), tape in registers with record_add (regt),
tape in the workspace (tape) -- and the wave records sit in LDS or, past
kLdsWords, in the workspace (gacc).  tests/_rowsweep.CASES holds every
geometry under each variant it can take, gacc on and off, the kAccD boundary,
the deepest stack, the capped gacc grid and the finish kernel's chunked adds.
Every case first asserts its launch plan (cnf_<family>_launch_plan).

Per case: loss_and_grads (cal and ce, grad_scale = 1 / B, dx), the generic
objective through autograd with random upstream weights on every zs[l] (and on
the log-det for planar: gz_all, gld), and the final-only objective through
transform (gz).  Parameter gradients and dx: 1e-4 under test_gpu_vjp._grad_err
against tests/_planar_ref.py / _radial_ref.py; loss terms 1e-5 relative.
_rowsweep.prepare admits a case only where the fp32 CPU path itself is within
a quarter of those bars.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

import _rowsweep as S
from _golden import rel_err
from cnf_hip import _lib, engine, rowstack
from cnf_hip.stack import _ptr, _stream
from test_gpu_rowflow_forward import _loss_err, on_device

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _flat_grads(flow):
    return torch.cat([q.grad.reshape(-1) for q in flow.parameters()]).cpu().numpy()


@pytest.mark.parametrize("cid", S.IDS)
def test_gradients(cid):
    case = S.BY_ID[cid]
    p = S.prepare(case)
    fam, B = case.family, case.B
    flow, stack, x, y = on_device(p)
    assert stack.launch_plan(B) == case.plan()
    planar = fam == "planar"
    ref = p.ref
    e = {}

    # the fused loss + reverse mode
    for kind, k, det in (("cal", _lib.LOSS_CAL, 1.0), ("ce", _lib.LOSS_CE, S.DET)):
        kw = {"det": det} if planar else {}
        n0 = engine.stats[fam + "_loss_vjp"]
        out = stack.loss_and_grads(x, y, kind=k, grad_scale=1.0 / B, need_dx=True, **kw)
        terms, grads, dx = [t.clone() for t in out]
        again = stack.loss_and_grads(x, y, kind=k, grad_scale=1.0 / B, need_dx=True, **kw)
        assert engine.stats[fam + "_loss_vjp"] == n0 + 2
        assert all(torch.equal(a, b) for a, b in zip((terms, grads, dx), again)), (cid, kind)
        e["loss_" + kind] = _loss_err(terms, ref["terms_" + kind], B)
        e["g_" + kind] = S.grad_err(grads.cpu().numpy(), ref["g_" + kind])
        e["dx_" + kind] = S.grad_err(dx.cpu().numpy(), ref["dx_" + kind])

    # upstream gradients on every layer's output (and the log-det): gz_all, gld
    gz_all = torch.from_numpy(p.gz_all).to(DEV)
    flow.zero_grad()
    n0 = engine.stats[fam + "_vjp"]
    xg = x.clone().requires_grad_(True)
    zs, ld = flow(xg)
    obj = (torch.stack(zs) * gz_all).sum()
    if planar:
        obj = obj + (ld.reshape(-1) * torch.from_numpy(p.gld).to(DEV)).sum()
    obj.backward()
    assert engine.stats[fam + "_vjp"] == n0 + 1, "the native reverse mode did not run"
    e["g_all"] = S.grad_err(_flat_grads(flow), ref["g_all"])
    e["dx_all"] = S.grad_err(xg.grad.cpu().numpy(), ref["dx_all"])

    # the final output's gradient alone, through transform: gz
    flow.zero_grad()
    xg = x.clone().requires_grad_(True)
    z, _ = flow.transform(xg)
    (z * gz_all[-1]).sum().backward()
    assert engine.stats[fam + "_vjp"] == n0 + 2
    e["g_fin"] = S.grad_err(_flat_grads(flow), ref["g_fin"])
    e["dx_fin"] = S.grad_err(xg.grad.cpu().numpy(), ref["dx_fin"])
    flow.zero_grad()

    row = S.record(case, attempt=p.attempt, floor_grad=p.floor_grad,
                   **{"bwd_" + k: v for k, v in e.items()})
    print("rowflow_sweep", json.dumps(row))
    for k, v in e.items():
        assert v <= (S.OUT_BAR if k.startswith("loss_") else S.GRAD_BAR), (cid, k, v)


# ---- bounds ----------------------------------------------------------------------------
SENT = -12345.678
PAD = 4096      # floats of sentinel on each side


class Guarded:
    """n floats cut from the middle of a sentinel-filled buffer."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), SENT, dtype=torch.float32, device=DEV)
        self.t = self.buf[PAD:PAD + n]

    def intact(self):
        return bool((self.buf[:PAD] == SENT).all()) and bool((self.buf[PAD + self.n:] == SENT).all())


@pytest.mark.parametrize("cid", S.BOUNDS)
def test_workspace_and_outputs_stay_inside_their_buffers(cid):
    """The C entry points with a workspace of exactly workspace_bytes and every
    output cut from the middle of a sentinel-filled buffer: forward with z,
    (log-det,) z_all; loss_vjp with dx; predict.  The one-lane-per-row kernels
    store whole blocks through an LDS tile (nrows * D contiguous floats), the
    reverse mode writes records, tape and dx: nothing may land outside."""
    case = S.BY_ID[cid]
    p = S.prepare(case)
    fam, D, L, B = case.family, case.D, case.L, case.B
    flow, stack, x, y = on_device(p)
    assert stack.launch_plan(B) == case.plan()
    planar = fam == "planar"
    lib = _lib.lib()
    nws = rowstack.workspace_bytes(fam, D, L, B)
    assert nws % 4 == 0 and nws == 4 * S.workspace_floats(fam, D, L, B)
    i32, i64, f32, sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
    ptrs = (ctypes.c_void_p * (3 * L))(*[q.data_ptr() for q in stack.param_tensors()])
    head = (i32(D), i32(L), ptrs, _ptr(x))
    lp = torch.from_numpy(p.lp).float().to(DEV)
    dev = torch.device(DEV)
    g = {k: Guarded(n) for k, n in (("ws", nws // 4), ("z", B * D), ("ld", B),
                                    ("z_all", L * B * D), ("terms", 3),
                                    ("grads", stack.param_count()), ("dx", B * D),
                                    ("probs", B * D), ("pld", B))}
    tail = (i64(B), _ptr(g["ws"].t), sz(nws), _stream(dev))
    call = lambda entry, *args: getattr(lib, "cnf_%s_%s" % (fam, entry))(*head, *args, *tail)
    if planar:
        assert call("forward", _ptr(g["z"].t), _ptr(g["ld"].t), _ptr(g["z_all"].t)) == 0
        assert call("loss_vjp", _ptr(y), i32(_lib.LOSS_CAL), f32(1.0), f32(1.0 / B),
                    _ptr(g["terms"].t), _ptr(g["grads"].t), _ptr(g["dx"].t)) == 0
        assert call("predict", _ptr(lp), _ptr(g["probs"].t), _ptr(g["pld"].t)) == 0
    else:
        assert call("forward", _ptr(g["z"].t), _ptr(g["z_all"].t)) == 0
        assert call("loss_vjp", _ptr(y), i32(_lib.LOSS_CAL), f32(1.0 / B), _ptr(g["terms"].t),
                    _ptr(g["grads"].t), _ptr(g["dx"].t)) == 0
        assert call("predict", _ptr(lp), _ptr(g["probs"].t)) == 0
    torch.cuda.synchronize()
    for k, buf in g.items():
        assert buf.intact(), "%s: a write outside %s" % (cid, k)
    # the calls ran: every output holds the reference's values, none a sentinel
    ref = p.ref
    num = lambda k, *shape: g[k].t.view(*shape).cpu().numpy()
    assert rel_err(num("z_all", L, B, D), ref["zs"]) <= S.OUT_BAR
    assert rel_err(num("z", B, D), ref["zs"][-1]) <= S.OUT_BAR
    assert rel_err(num("probs", B, D), ref["probs"]) <= S.OUT_BAR
    assert S.grad_err(num("grads", -1), ref["g_cal"]) <= S.GRAD_BAR
    assert S.grad_err(num("dx", B, D), ref["dx_cal"]) <= S.GRAD_BAR
    assert _loss_err(g["terms"].t, ref["terms_cal"], B) <= S.OUT_BAR
    if planar:
        assert rel_err(num("ld", B), ref["ld"]) <= S.OUT_BAR
        assert not bool((g["pld"].t == SENT).any())
