"""Every row-geometry kernel of the mixed family on the GPU against float64
(tests/_mixed_sweep.py): forward, zs and the per-row log-det, both fused losses
with gradients and dx, the reverse mode with gz only and with gz_all + gld,
predict, score, and a second call bitwise equal -- for all geometries of
_rowsweep.WIDTHS at depths 3 and 11, at a ragged multi-block batch and at one
row, and for the shapes on each side of every switch of the reverse mode.  No
row and no case is exempt.

Bars: _rowsweep's OUT_BAR (outputs, log-dets, loss terms) and GRAD_BAR
(gradients, dx); probabilities under probs_err with max(1e-5, twice the fp32
CPU path's own error); the score record is exact against
calibration_record(predict(...)).  Each case first asserts the launch-plan
fields it is about (literals in _mixed_sweep) against cnf_mixed_launch_plan.
"""
import numpy as np
import pytest
import torch

import _mixed_ref as M
import _mixed_sweep as MS
import _rowsweep as S
from _golden import rel_err
from cnf_hip import _lib, mixed
from cnf_hip.metrics import calibration_record
from cnf_hip.mixed import MixedStack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("case", MS.CASES, ids=MS.IDS)
def test_case(case):
    p = MS.prepare(case)
    D, L, B = case.D, case.L, case.B
    plan = case.plan()
    assert mixed.launch_plan(D, case.kinds, B) == plan
    flow = M.build_flow(p.ps, DEV)
    stack = MixedStack(list(flow.layers))
    assert stack.kinds == case.kinds
    x, y, ref = _dev(p.x), _dev(p.y), p.ref
    out, grad = {}, {}

    # forward
    _, ld, zs = stack.run(x, want_all=True)
    z, ld1, _ = stack.run(x)
    out["zs"], out["ld"] = rel_err(zs.cpu().numpy(), ref["zs"]), rel_err(ld.cpu().numpy(), ref["ld"])
    assert ld.shape == (B,) and torch.equal(z, zs[-1]) and torch.equal(ld, ld1)

    # fused losses
    for kind, k, det in (("cal", _lib.LOSS_CAL, 1.0), ("ce", _lib.LOSS_CE, MS.DET)):
        terms, g, dx = stack.loss_and_grads(x, y, kind=k, det=det, grad_scale=1.0 / B,
                                            need_dx=True)
        t2, _, _ = stack.forward_loss(x, y, kind=k, det=det)
        tr = ref["terms_" + kind] / B
        out["terms_" + kind] = max(rel_err(terms.cpu().numpy() / B, tr),
                                   rel_err(t2.cpu().numpy() / B, tr))
        grad["g_" + kind] = S.grad_err(g.cpu().numpy(), ref["g_" + kind])
        grad["dx_" + kind] = S.grad_err(dx.cpu().numpy(), ref["dx_" + kind])
        again = stack.loss_and_grads(x, y, kind=k, det=det, grad_scale=1.0 / B, need_dx=True)
        assert all(torch.equal(a, b) for a, b in zip(again, (terms, g, dx)))
        assert torch.equal(stack.forward_loss(x, y, kind=k, det=det)[0], t2)

    # reverse mode
    gza, gld = _dev(p.gz_all), _dev(p.gld)
    dxa, ga = stack.vjp(x, gza, gld, True, True)
    dxf, gf = stack.vjp(x, gza[-1], None, False, True)
    grad["g_all"], grad["dx_all"] = (S.grad_err(ga.cpu().numpy(), ref["g_all"]),
                                     S.grad_err(dxa.cpu().numpy(), ref["dx_all"]))
    grad["g_fin"], grad["dx_fin"] = (S.grad_err(gf.cpu().numpy(), ref["g_fin"]),
                                     S.grad_err(dxf.cpu().numpy(), ref["dx_fin"]))
    dxa2, ga2 = stack.vjp(x, gza, gld, True, True)
    assert torch.equal(ga, ga2) and torch.equal(dxa, dxa2)

    # predict / score
    lp = _dev(p.lp.astype(np.float32))
    probs = stack.predict(x, lp)
    pd = S.probs_err(probs.cpu().numpy(), ref["probs"])
    assert torch.equal(probs, stack.predict(x, lp))
    if D >= 2:
        for bins in (1, MS.BINS):
            assert torch.equal(stack.score(x, lp, y, bins), calibration_record(probs, y, bins))
        yb = y.clone()
        yb[0] = D
        rec = stack.score(x, lp, yb, MS.BINS)
        assert int(rec[1]) == 1 and torch.equal(rec, calibration_record(probs, yb, MS.BINS))

    MS.record(case, attempt=p.attempt, floor_out=p.floor_out, floor_grad=p.floor_grad,
              out=max(out.values()), grad=max(grad.values()), probs_d=pd, probs_bar=p.probs_bar)
    print("%s [%s gacc=%d]: out %s grad %s probs*D %.2e (bar %.2e)"
          % (case.id, MS.variant_name(plan), plan["gacc"],
             " ".join("%s=%.1e" % kv for kv in out.items()),
             " ".join("%s=%.1e" % kv for kv in grad.items()), pd, p.probs_bar))
    assert max(out.values()) <= S.OUT_BAR, out
    assert max(grad.values()) <= S.GRAD_BAR, grad
    assert pd <= p.probs_bar
