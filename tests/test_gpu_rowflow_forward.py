"""Every planar and radial row geometry on the GPU against float64: forward
(every layer's output, log-det), transform, forward_loss, predict and score.

CNF_ROWFLOW_DISPATCH instantiates k_<family>_fwd, _predict and _score for 22
geometries <lpr, cpl>; tests/_rowsweep.CASES runs each of them, at both ends
of every multi-lane geometry, in both families, at more than one block with a
ragged last one and at one row, plus the boundary shapes (deepest stack, each
side of the LDS-record limit, one row past the grid cap at 16 and 64 lanes per
row).  Every case first asserts the launch plan it expects
(cnf_<family>_launch_plan), so a dispatch change cannot turn it into a test of
another kernel.

Bars: outputs, log-det and probabilities 1e-5 under _golden.rel_err, loss terms
1e-5 relative, against tests/_planar_ref.py, _planar_predict_ref.py and
_radial_ref.py.  The probabilities are held a second time in units of the
uniform one (_rowsweep.probs_err, at max(1e-5, twice the fp32 CPU path's own
error)), without which the comparison cannot see one wrong column of a wide
row.  No other per-case floors: _rowsweep.prepare admits a case only where
the fp32 CPU path itself is within a quarter of the bar.  score must leave, word
for word, the record of calibration_record(predict(x), y).
"""
import json

import numpy as np
import pytest
import torch

import _rowsweep as S
from _golden import rel_err
from cnf_hip import _lib, engine
from cnf_hip.metrics import calibration_record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def on_device(p):
    flow = S.build_flow(p, DEV)
    stack = flow._planar_stack() if p.case.family == "planar" else flow._radial_stack()
    return flow, stack, torch.from_numpy(p.x).to(DEV), torch.from_numpy(p.y).to(DEV)


def _loss_err(terms, ref, B):
    got = terms.cpu().numpy().astype(np.float64) / B
    ref = np.asarray(ref, dtype=np.float64) / B
    return float(np.max(np.abs(got - ref) / (np.abs(ref) + 1.0)))


@pytest.mark.parametrize("cid", S.IDS)
def test_forward_loss_predict_score(cid):
    case = S.BY_ID[cid]
    p = S.prepare(case)
    fam, D, L, B = case.family, case.D, case.L, case.B
    flow, stack, x, y = on_device(p)
    assert stack.launch_plan(B) == case.plan()
    planar = fam == "planar"
    ref = p.ref

    # flow(x): every layer's output and the log-det; transform: the final one
    n0 = engine.stats[fam + "_forward"]
    with torch.no_grad():
        zs, ld = flow(x)
        z, ld2 = flow.transform(x)
        z_again, _ = flow.transform(x)
    assert engine.stats[fam + "_forward"] == n0 + 3, "native path did not run"
    assert len(zs) == L
    e = {"zs": rel_err(torch.stack(zs).cpu().numpy(), ref["zs"])}
    if planar:
        e["ld"] = rel_err(ld.reshape(-1).cpu().numpy(), ref["ld"])
        assert torch.equal(ld, ld2)
    else:
        assert float(ld) == 0.0 and float(ld2) == 0.0
    assert torch.equal(z, zs[-1]) and torch.equal(z, z_again)

    # forward_loss, both kinds
    lp = torch.from_numpy(p.lp).float().to(DEV)
    for kind, k, det in (("cal", _lib.LOSS_CAL, 1.0), ("ce", _lib.LOSS_CE, S.DET)):
        if planar:
            terms, zl, ldl = stack.forward_loss(x, y, kind=k, det=det, want_outputs=True)
            assert rel_err(ldl.cpu().numpy(), ref["ld"]) <= S.OUT_BAR
        else:
            terms, zl = stack.forward_loss(x, y, kind=k, want_outputs=True)
        assert rel_err(zl.cpu().numpy(), ref["zs"][-1]) <= S.OUT_BAR
        e["loss_" + kind] = _loss_err(terms, ref["terms_" + kind], B)

    # predict, and score against the two-launch record
    probs = stack.predict(x, lp)
    assert torch.equal(probs, stack.predict(x, lp))
    e["probs"] = rel_err(probs.cpu().numpy(), ref["probs"])
    e["probs_d"] = S.probs_err(probs.cpu().numpy(), ref["probs"])      # D * p: same bar
    if D >= 2:                                  # cnf_metrics' envelope: 2 <= dim
        n0 = engine.stats[fam + "_score"]
        rec = stack.score(x, lp, y, S.BINS)
        assert engine.stats[fam + "_score"] == n0 + 1
        want = calibration_record(probs, y, S.BINS)
        assert torch.equal(rec, want), (cid, rec.tolist(), want.tolist())
        assert int(rec[0]) == B and int(rec[1]) == 0

    row = S.record(case, attempt=p.attempt, floor_out=p.floor_out, floor_probs_d=p.floor_probs_d,
                   **{"fwd_" + k: v for k, v in e.items()})
    print("rowflow_sweep", json.dumps(row))
    for k, v in e.items():
        assert v <= (p.probs_bar if k == "probs_d" else S.OUT_BAR), (cid, k, v)
