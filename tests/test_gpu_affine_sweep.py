"""Every row-geometry kernel of the affine family on the GPU against float64
(tests/_affine_sweep.py): forward, zs and the [1] log-det, inverse, xs and its
log-det, both fused losses with gradients and dx, the reverse mode with gz
only and with gz_all + gld, predict, score, and a second call bitwise equal --
for all geometries of _rowsweep.WIDTHS at depths 3 and 11, at a ragged
multi-block batch and at one row, and for the family's boundary shapes.  No
row and no case is exempt.

Bars: _rowsweep's OUT_BAR (outputs, log-dets, probabilities, loss terms) and
GRAD_BAR (gradients, dx); the score record is exact against
calibration_record(predict(...)).  Each case first asserts the launch-plan
fields it is about (literals in _affine_sweep) against cnf_affine_launch_plan.
"""
import numpy as np
import pytest
import torch

import _affine_ref as A
import _affine_sweep as AS
import _rowsweep as S
from _golden import rel_err
from cnf_hip import _lib, rowstack
from cnf_hip.affine import AffineStack
from cnf_hip.metrics import calibration_record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("case", AS.CASES, ids=AS.IDS)
def test_case(case):
    p = AS.prepare(case)
    D, L, B = case.D, case.L, case.B
    plan = case.plan()
    assert rowstack.launch_plan("affine", D, L, B) == plan
    flow = A.build_flow(p.d, DEV)
    stack = AffineStack(list(flow.layers))
    x, y, ref = _dev(p.x), _dev(p.y), p.ref
    out, grad = {}, {}

    # forward / inverse
    _, ld, zs = stack.run(x, want_all=True)
    z, ld1, _ = stack.run(x)
    out["zs"], out["ld"] = rel_err(zs.cpu().numpy(), ref["zs"]), rel_err(ld.cpu().numpy(), ref["ld"])
    assert ld.shape == (1,) and torch.equal(z, zs[-1]) and torch.equal(ld, ld1)
    zin = _dev(ref["zs"][-1].astype(np.float32))
    _, ild, xs = stack.run(zin, inverse=True, want_all=True)
    xf, ild1, _ = stack.run(zin, inverse=True)
    out["xs"] = rel_err(xs.cpu().numpy(), ref["xs"])
    out["ild"] = rel_err(ild.cpu().numpy(), ref["ild"])
    assert ild.shape == (1,) and torch.equal(xf, xs[-1]) and torch.equal(ild, ild1)
    xb, _, _ = stack.run(z, inverse=True)
    out["rt"] = rel_err(xb.cpu().numpy(), ref["rt"])

    # fused losses
    for kind, k, det in (("cal", _lib.LOSS_CAL, 1.0), ("ce", _lib.LOSS_CE, AS.DET)):
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
    out["probs"] = rel_err(probs.cpu().numpy(), ref["probs"])
    pd = S.probs_err(probs.cpu().numpy(), ref["probs"])
    assert torch.equal(probs, stack.predict(x, lp))
    if D >= 2:
        for bins in (1, AS.BINS):
            assert torch.equal(stack.score(x, lp, y, bins), calibration_record(probs, y, bins))
        yb = y.clone()
        yb[0] = D
        rec = stack.score(x, lp, yb, AS.BINS)
        assert int(rec[1]) == 1 and torch.equal(rec, calibration_record(probs, yb, AS.BINS))

    print("%s [%s gacc=%d]: out %s grad %s probs*D %.2e (bar %.2e)"
          % (case.id, S.variant_name(plan), plan["gacc"],
             " ".join("%s=%.1e" % kv for kv in out.items()),
             " ".join("%s=%.1e" % kv for kv in grad.items()), pd, p.probs_bar))
    assert max(out.values()) <= S.OUT_BAR, out
    assert max(grad.values()) <= S.GRAD_BAR, grad
    assert pd <= p.probs_bar
