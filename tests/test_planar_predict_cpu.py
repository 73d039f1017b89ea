"""The planar calibrator path without a GPU: argument validation of
cnf_planar_predict and cnf_adam_step_tensors (every status is returned before
any device work), the float64 restatement of predict (tests/
_planar_predict_ref.py) against the reference's float64 record
(tests/golden/planar_predict), and the package's host calibrator against the
reference's own TorchFlowCalibrator run (tests/golden/planar_cal)."""
import ctypes

import numpy as np
import pytest
import torch

import _planar_predict_ref as PR
import _planar_ref as R
from cnf_hip import _lib
from cnf_hip.planar import workspace_bytes

P = ctypes.c_void_p
I32, I64, DB = ctypes.c_int32, ctypes.c_int64, ctypes.c_double


def _args(L=2, bad=None):
    arr = (P * (3 * L))(*[4096 + 64 * i for i in range(3 * L)])
    if bad is not None:
        arr[bad[0]] = bad[1]
    return arr


def test_predict_argument_validation_without_gpu():
    lib = _lib.lib()
    D, L, B = 3, 2, 8
    ws = workspace_bytes(D, L, B)
    pr = lambda params, x, lp, probs, ld, b, w, wb, d=D, l=L: lib.cnf_planar_predict(
        I32(d), I32(l), params, P(x), P(lp), P(probs), P(ld), I64(b), P(w), ctypes.c_size_t(wb),
        P(0))
    assert pr(_args(), 16, 16, 16, 0, -1, 16, ws) == -4
    assert pr(_args(), 16, 16, 16, 0, (1 << 31) + 1, 16, ws) == -4
    assert pr(None, 16, 16, 16, 0, B, 16, ws) == -1
    assert pr(_args(bad=(4, 0)), 16, 16, 16, 0, B, 16, ws) == -1      # a NULL parameter
    assert pr(_args(bad=(4, 4098)), 16, 16, 16, 0, B, 16, ws) == -6   # a misaligned one
    assert pr(_args(), 0, 16, 16, 0, B, 16, ws) == -1                 # x
    assert pr(_args(), 16, 0, 16, 0, B, 16, ws) == -1                 # log_priors
    assert pr(_args(), 16, 16, 0, 0, B, 16, ws) == -1                 # probs
    assert pr(_args(), 16, 16, 16, 0, B, 0, ws) == -1                 # workspace
    assert pr(_args(), 16, 16, 16, 0, B, 16, ws - 4) == -1            # too small
    assert pr(_args(), 18, 16, 16, 0, B, 16, ws) == -6
    assert pr(_args(), 16, 18, 16, 0, B, 16, ws) == -6
    assert pr(_args(), 16, 16, 18, 0, B, 16, ws) == -6
    assert pr(_args(), 16, 16, 16, 18, B, 16, ws) == -6
    assert pr(_args(), 16, 16, 16, 0, B, 18, ws) == -6
    assert pr(_args(), 16, 16, 16, 0, B, 16, ws, d=257) == -3
    assert pr(_args(), 16, 16, 16, 0, B, 16, ws, d=0) == -2
    assert pr(_args(L=65), 16, 16, 16, 0, B, 16, ws, l=65) == -3
    assert pr(_args(), 16, 16, 16, 0, B, 16, ws, l=0) == -2
    assert pr(_args(), 0, 0, 0, 0, 0, 0, 0) == 0                      # B == 0: a no-op


def test_adam_tensors_argument_validation_without_gpu():
    lib = _lib.lib()

    def call(n, numel, params, grads=16, m=16, v=16, step=1, sched=0):
        ne = None if numel is None else (I64 * max(len(numel), 1))(*numel)
        pa = None if params is None else (P * max(len(params), 1))(*params)
        return lib.cnf_adam_step_tensors(I32(n), ne, pa, P(grads), P(m), P(v), I64(step),
                                         DB(1e-3), P(sched), DB(0.9), DB(0.999), DB(1e-8),
                                         DB(0.0), P(0), P(0))
    ok = ([3, 3, 1], [4096, 4160, 4224])
    assert call(-1, *ok) == -2
    assert call(3, ok[0], [4096, 0, 4224]) == -1          # a NULL tensor
    assert call(3, [3, -3, 1], ok[1]) == -2               # numel < 0
    assert call(3, *ok, step=0) == -2                     # step < 1 without sched
    assert call(3, None, ok[1]) == -1
    assert call(3, ok[0], None) == -1
    assert call(3, *ok, grads=0) == -1
    assert call(3, *ok, m=0) == -1
    assert call(3, *ok, v=0) == -1
    assert call(0, [], []) == 0                           # nothing to do
    assert call(0, None, None) == 0
    # past the 128-tensor chunk boundary the checks still precede every launch
    n = 200
    many = [4096 + 64 * i for i in range(n)]
    many[199] = 0
    assert call(n, [3] * n, many) == -1
    assert call(n, [3] * 199 + [-1], [4096 + 64 * i for i in range(n)]) == -2


def test_stack_adam_takes_any_stack():
    """StackAdam's host side (hyper-parameters, state round trip, schedule
    scalars) for a PlanarStack, which has no cnf_desc."""
    from cnf_hip.adam import StackAdam, supports
    from cnf_hip.planar import PlanarStack
    from flows.flows import Flow, PlanarLayer
    torch.manual_seed(3)
    flow = Flow([PlanarLayer(3) for _ in range(2)])
    stack = PlanarStack(list(flow.layers))
    assert not hasattr(stack, "desc")
    opt = torch.optim.Adam(flow.parameters(), lr=2e-3, betas=(0.8, 0.99), eps=1e-7)
    assert supports(opt) and not supports(torch.optim.AdamW(flow.parameters()))
    for p in flow.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    opt.step()
    sa = StackAdam.like(stack, opt)
    assert (sa.lr, sa.betas, sa.eps, sa.t) == (2e-3, (0.8, 0.99), 1e-7, 2)
    assert sa._m.numel() == stack.param_count() == 14
    assert sa.sched_values(3) == (2e-3 / (1 - 0.8 ** 3), (1 - 0.99 ** 3) ** 0.5)
    want = [opt.state[p]["exp_avg"].clone() for p in stack.param_tensors()]
    opt2 = torch.optim.Adam(flow.parameters())
    sa.store_into(opt2)
    for p, w in zip(stack.param_tensors(), want):
        assert float(opt2.state[p]["step"]) == 2.0
        assert torch.equal(opt2.state[p]["exp_avg"], w)


@pytest.mark.parametrize("name", sorted(PR.FIXTURES))
def test_restatement_matches_float64_reference(name):
    d = PR.load(name)
    probs, ld = PR.predict(R.params_of(d), d["x"], d["log_priors"])
    assert (np.isnan(probs) == np.isnan(d["probs64"])).all()
    assert (np.isnan(ld) == np.isnan(d["ld64"])).all()
    ok = ~np.isnan(d["probs64"])
    assert not ok.any() or float(np.max(np.abs(probs[ok] - d["probs64"][ok]))) <= 1e-12
    okl = ~np.isnan(d["ld64"])
    assert not okl.any() or float(np.max(np.abs(ld[okl] - d["ld64"][okl])
                                         / (np.abs(d["ld64"][okl]) + 1))) <= 1e-12
    if name in ("nan", "inf"):
        assert np.isnan(d["probs64"]).all() and np.isnan(d["probs"]).all()
    else:
        assert ok.all() and float(d["qmin"]) >= 0.05
        assert np.abs(d["probs64"].sum(axis=1) - 1).max() <= 1e-12


@pytest.mark.parametrize("name", ["full", "mb128"])
def test_host_calibrator_matches_reference_run(name):
    """The package's TorchFlowCalibrator on the CPU (the reference's own torch
    loop), seeded as the generator seeds the reference: parameters, history
    and predictions within 1e-6 relative.  Measured on the build machine: 0
    for every quantity, both batch sizes."""
    from calibrators import TorchFlowCalibrator
    from flows._factory import PlanarFlow
    d = PR.load_cal(name)
    L, D = d["W"].shape
    torch.manual_seed(int(d["seed"]))
    f0 = PlanarFlow(D, layers=L)
    assert all(np.array_equal(ly.w.detach().numpy(), d["W0"][l])
               and np.array_equal(ly.u.detach().numpy(), d["U0"][l])
               and np.array_equal(ly.b.detach().numpy(), d["Bv0"][l:l + 1])
               for l, ly in enumerate(f0.layers)), "initial parameters differ"
    torch.manual_seed(int(d["seed"]))
    cal = TorchFlowCalibrator(PlanarFlow, d["logits"], np.eye(D)[d["labels"]], layers=L,
                              epochs=int(d["epochs"]), batch_size=int(d["batch_size"]),
                              dev=torch.device("cpu"))
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b) / (np.abs(b) + 1)))
    errs = {"W": rel(np.stack([ly.w.detach().numpy() for ly in cal.flow.layers]), d["W"]),
            "U": rel(np.stack([ly.u.detach().numpy() for ly in cal.flow.layers]), d["U"]),
            "Bv": rel(np.concatenate([ly.b.detach().numpy() for ly in cal.flow.layers]), d["Bv"]),
            "pred": rel(cal.predict(d["held"]), d["pred"])}
    for k in ("loss", "ce", "log_det"):
        errs[k] = rel([float(v) for v in cal.history[k]], d[k].astype(np.float64))
    print("%s: %s" % (name, errs))
    assert len(cal.history["loss"]) == int(d["epochs"])
    assert max(errs.values()) <= 1e-6
