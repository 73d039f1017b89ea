"""Every dispatch class of the layer-at-a-time reverse mode (cnf_wvjp.hip:
wvjp_run, wvjp_inv_run) against float64 CPU autograd.

The cases (tests/_widesweep.LAYERWISE) are the smallest shapes that reach each
class: both sides of every pick_nj threshold (k_wfwd_update / k_wbwd_update
<kNJ>), strict_nan and the inverse's reverse mode at D > 128, L = 1 (keep_acts
off: the backward sweep recomputes the activations), every k_wgemm
instantiation with 1..7 column blocks and 1..4 reduction chunks, k_wdw16 with
grid z > 1 and with two row blocks, and the batch caps of the row kernels.
tests/test_widesweep_sync_cpu.py shows that list complete.  Each case first
asserts kernel_name() == "mfma-tile", vjp_kernel_name() == "layerwise" and its
launch plan (cnf_vjp_launch_plan), so a dispatch change cannot turn it into a
test of another kernel.

Objectives per case and batch: every layer's output and the log-det weighted
("all"), the final output and the log-det ("fin", Flow.transform), and
loss_and_grads for the cal and ce losses with need_dx; the inverse cases the
first two on Flow.backward / inverse_transform.  Bars: loss terms 1e-5 x the
sum of the per-row magnitudes, every gradient _sweep.grad_err <= 1e-4.  The
inputs are admitted on the CPU from the references alone
(_widesweep.prepare_grad).

The batch-cap case has no hidden layer: the ReLU-kink guard cannot admit a
stack with hidden units at 65,541 rows (the number of pre-activations within
KINK_MIN of zero grows with rows x units), and without hidden units there is
no kink to guard.

A final group runs one case per kNJ and one inverse case through the C entry
points with a workspace of exactly cnf_vjp_workspace_bytes and every output
cut from a sentinel-filled buffer: the sentinels on both sides survive, and a
repeated call agrees bitwise."""
import ctypes

import numpy as np
import pytest
import torch

import _sweep
import _widesweep as W
from cnf_hip import _lib, engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [c.id for c in W.LAYERWISE]


def _np(t):
    return t.detach().cpu().numpy()


def _stack(case, p):
    fg = W.to_device(p.flow, DEV, case.strict)
    stack = fg._native_stack()
    assert stack.kernel_name() == "mfma-tile" and stack.strict_nan == case.strict
    assert stack.vjp_kernel_name() == "layerwise"
    return fg, stack


@pytest.mark.parametrize("case", W.LAYERWISE, ids=IDS)
def test_reverse_mode_against_float64(case):
    p = W.prepare_grad(case)
    fg, stack = _stack(case, p)
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
            W.objective(fg, name, xg, y, w, wl, case.inverse).backward()
            assert engine.stats["vjp"] + engine.stats["torch_ops"] > n0, "native path did not run"
            got = ([_np(q.grad) for q in W.params(fg)], _np(xg.grad))
            e = W.worst_grad(got, refs[name])
            print("%s B=%d %s seed=%d: grad err %.2e" % (case.id, B, name, p.seed, e))
            assert e <= W.GRAD_BAR, (B, name, e)
            worst = max(worst, e)
        if case.inverse:
            continue
        for name in ("cal", "ce"):
            kind = 0 if name == "cal" else 1
            rows = W.loss_rows(p, B, name)
            n0 = engine.stats["loss_vjp"]
            terms, grads, dx = stack.loss_and_grads(x, y, kind=kind, det=1.0 if kind == 0 else W.DET,
                                                    grad_scale=1.0 / B, need_dx=True)
            assert engine.stats["loss_vjp"] == n0 + 1
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
             plan=dict(case.expect))


def test_past_the_lds_bound_is_none():
    """(256, [281]) with two nets: one column past the last width wvjp_ok
    admits; no reverse mode, and the workspace query says so."""
    D, hidden = W.PAST_LDS
    flow = _sweep.make_flow(D, 2, hidden, W.SIGMA, _sweep.SEED0)
    stack = flow.to(DEV)._native_stack()
    assert stack.kernel_name() == "mfma-tile" and stack.vjp_kernel_name() == "none"
    assert stack.vjp_launch_plan(69) == {"path": "none"} and not stack.has_native_vjp()
    n = ctypes.c_size_t()
    assert _lib.lib().cnf_vjp_workspace_bytes(ctypes.byref(stack.desc), ctypes.c_int64(69),
                                              ctypes.byref(n)) == -3   # CNF_ERR_UNSUPPORTED


# ---- exact workspace, sentinels, repeatability ----------------------------------------
FENCED = [c.id for c in W.LAYERWISE if c.group == "width" and not c.strict and c.L == 2
          and c.D in (64, 128, 192, 256)]


@pytest.mark.parametrize("cid", FENCED)
def test_exact_workspace_and_fenced_outputs(cid):
    """One case per kNJ (1..4) and the inverse at D = 256."""
    case = W.BY_ID[cid]
    p = W.prepare_grad(case)
    _, stack = _stack(case, p)
    B = case.batches[-1]
    W.assert_plan(case, stack, B)
    refs = W.grad_refs(p, B)
    if case.inverse:
        e = W.check_fenced(stack, case, p, B, "cnf_vjp_inverse", refs["all"])
    else:
        e = max(W.check_fenced(stack, case, p, B, "cnf_vjp", refs["all"]),
                W.check_fenced(stack, case, p, B, "cnf_loss_vjp", refs["cal"]))
    W.record(case, fenced_grad_err=e)
