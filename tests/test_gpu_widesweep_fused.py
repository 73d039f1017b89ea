"""Every row of k_wide16's table (cnf_wide16.hip kW16Table) x nets {2, 1} at
L = 1 and L = 3 (random_flip), forward family and fused training sweeps, against
float64.

Forward family (k_wide16<..., MODE, NETS>: transform, inverse_transform,
predict) at B in {1, 131, 517} -- 131 is one 128-row block plus a wave with
three rows and three waves with none -- against the float64 numpy oracle;
predict against _sweep.predict64, absolute and in units of the uniform
probability (D * p).

Training (k_wtrain16_fwd / _bwd, k_wseed, k_wdw16g) at B in {1, 131}: the
generic objectives through k_wseed (every layer's gz_all, and final-only) and
loss_and_grads for cal and ce with need_dx (the seed rides the forward sweep's
epilogue), against float64 CPU autograd; one L = 2 case per row x nets at
B = 261, where k_wdw16g sums two row-block records, and the table's row without
hidden units at 65,541 rows (plan16's batch caps).  Gradient batches stay
small on purpose: with 100-wide hidden layers the ReLU-kink guard expects
about 7 pre-activations within KINK_MIN of zero per seed at 517 rows, and the
seed search would fail.

Each case first asserts kernel_name() == "mfma-wide", vjp_kernel_name() ==
"wide-fused" and its launch plan: the table row, nets, k_wdw16g and its
(G tiles, H tiles) classes.  Bars as tests/test_gpu_widesweep_layerwise.py;
outputs and log-det rel_err <= 1e-5, the inverse max(1e-5, 2 x the fp32 numpy
oracle's own error), predict 1e-5 absolute and max(1e-5, 2 x the fp32 CPU
path's own error) in D * p.  One case per table row also runs through the C
entry points with an exact workspace and fenced outputs."""
import numpy as np
import pytest
import torch

import _widesweep as W
from _golden import rel_err
from cnf_hip import engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STACKS = [c for c in W.FUSED if c.batches == (1, 131)]


def _np(t):
    return t.detach().cpu().numpy()


def _stack(case, flow):
    fg = W.to_device(flow, DEV)
    stack = fg._native_stack()
    assert stack.kernel_name() == "mfma-wide" and stack.vjp_kernel_name() == "wide-fused"
    plan = W.assert_plan(case, stack, case.batches[-1])
    assert plan["row"] == W.W16_TABLE.index((case.D, case.hidden))
    assert plan["nets"] == (2 if case.scale else 1) and plan["wdwg"]
    assert plan["classes"] == W.case_plan(case)["classes"] != set()
    return fg, stack


@pytest.mark.parametrize("case", STACKS, ids=[c.id for c in STACKS])
def test_forward_inverse_predict_against_float64(case):
    p = W.prepare_forward(case)
    fg, stack = _stack(case, p.flow)
    xg, zg = p.x.to(DEV), torch.from_numpy(p.zin).to(DEV)
    lp = torch.log(p.prior).to(DEV)
    worst = dict(fwd_err=0.0, inv_err=0.0, inv_fp32_oracle_err=0.0, predict_err=0.0,
                 predict_dp_err=0.0, predict_dp_fp32_cpu_err=0.0)
    for B in W.FUSED_FORWARD_BATCHES:
        n0 = engine.stats["forward"] + engine.stats["inverse"] + engine.stats["predict"]
        with torch.no_grad():
            z, ld = fg.transform(xg[:B])
            xr, ild = fg.inverse_transform(zg[:B])
            probs = stack.predict(xg[:B], lp)
        assert engine.stats["forward"] + engine.stats["inverse"] + engine.stats["predict"] \
            == n0 + 3, "native path did not run"
        ef = max(rel_err(_np(z), p.z64[:B]), rel_err(_np(ld).reshape(-1), p.ld64[:B]))
        floor = max(rel_err(p.x32[:B], p.x64[:B]), rel_err(p.ild32[:B], p.ild64[:B]))
        ei = max(rel_err(_np(xr), p.x64[:B]), rel_err(_np(ild).reshape(-1), p.ild64[:B]))
        ep = float(np.max(np.abs(_np(probs).astype(np.float64) - p.p64[:B])))
        edp, fdp = W.probs_err(_np(probs), p.p64[:B]), W.probs_err(p.p32[:B], p.p64[:B])
        print("%s B=%d seed=%d: fwd %.2e inv %.2e (fp32 oracle %.2e) predict %.2e, D*p %.2e "
              "(fp32 cpu %.2e)" % (case.id, B, p.seed, ef, ei, floor, ep, edp, fdp))
        assert ef <= W.OUT_BAR, (B, ef)
        assert ei <= max(W.OUT_BAR, 2 * floor), (B, ei, floor)
        assert ep <= W.OUT_BAR, (B, ep)
        assert edp <= max(W.OUT_BAR, 2 * fdp), (B, edp, fdp)
        for k, v in (("fwd_err", ef), ("inv_err", ei), ("inv_fp32_oracle_err", floor),
                     ("predict_err", ep), ("predict_dp_err", edp),
                     ("predict_dp_fp32_cpu_err", fdp)):
            worst[k] = max(worst[k], v)
    W.record(case, forward_seed=p.seed, **worst)


@pytest.mark.parametrize("case", W.FUSED, ids=[c.id for c in W.FUSED])
def test_training_sweeps_against_float64(case):
    p = W.prepare_grad(case)
    fg, stack = _stack(case, p.flow)
    worst, worst_terms = 0.0, 0.0
    for B in case.batches:
        W.assert_plan(case, stack, B)
        refs = W.grad_refs(p, B)
        x, y = p.x[:B].to(DEV), p.y[:B].to(DEV)
        w, wl = p.w[:, :B].to(DEV), p.wl[:B].to(DEV)
        for name in ("all", "fin"):
            fg.zero_grad()
            xg = x.clone().requires_grad_(True)
            n0 = engine.stats["vjp"] + engine.stats["torch_ops"]
            W.objective(fg, name, xg, y, w, wl, False).backward()
            assert engine.stats["vjp"] + engine.stats["torch_ops"] > n0, "native path did not run"
            e = W.worst_grad(([_np(q.grad) for q in W.params(fg)], _np(xg.grad)), refs[name])
            print("%s B=%d %s seed=%d: grad err %.2e" % (case.id, B, name, p.seed, e))
            assert e <= W.GRAD_BAR, (B, name, e)
            worst = max(worst, e)
        for name in ("cal", "ce"):
            kind = 0 if name == "cal" else 1
            rows = W.loss_rows(p, B, name)
            terms, grads, dx = stack.loss_and_grads(x, y, kind=kind, det=1.0 if kind == 0 else W.DET,
                                                    grad_scale=1.0 / B, need_dx=True)
            terr = np.abs(terms.double().cpu().numpy() - rows.sum(axis=1))
            bound = W.OUT_BAR * np.abs(rows).sum(axis=1)
            e = W.worst_grad(([_np(t) for t in stack.split(grads)], _np(dx)), refs[name])
            print("%s B=%d %s: terms err %s bound %s grad err %.2e" % (case.id, B, name, terr,
                                                                       bound, e))
            assert np.all(terr <= bound), (B, name, terr, bound)
            assert e <= W.GRAD_BAR, (B, name, e)
            worst = max(worst, e)
            worst_terms = max(worst_terms, W.terms_ratio(terr, bound))
    W.record(case, seed=p.seed, fp32_cpu_grad_err=p.floor, grad_err=worst,
             terms_err_over_bound=worst_terms, fp32_cpu_terms_err_over_bound=p.terms_floor,
             plan=dict(case.expect),
             classes=sorted(W.case_plan(case)["classes"]))


FENCED = [c.id for c in W.FUSED if c.L == 3 and c.scale]


@pytest.mark.parametrize("cid", FENCED)
def test_exact_workspace_and_fenced_outputs(cid):
    """One case per table row: cnf_vjp and cnf_loss_vjp with a workspace of
    exactly cnf_vjp_workspace_bytes and outputs between sentinels."""
    case = W.BY_ID[cid]
    p = W.prepare_grad(case)
    _, stack = _stack(case, p.flow)
    B = case.batches[-1]
    refs = W.grad_refs(p, B)
    e = max(W.check_fenced(stack, case, p, B, "cnf_vjp", refs["all"]),
            W.check_fenced(stack, case, p, B, "cnf_loss_vjp", refs["cal"]))
    W.record(case, fenced_grad_err=e)
