"""TorchFlowCalibrator around a mixed planar / radial / affine flow on the GPU:
the native fit (one cnf_mixed_loss_vjp + one cnf_adam_step_tensors per batch,
HIP-graph epochs included), predict, evaluate and the one-launch score, against
the reference's own CPU run (tests/golden/mixed_cal, order PRPRA).

Bars: those of tests/test_gpu_radial_cal.py / test_gpu_affine_cal.py --
parameters within steps * lr * 2e-2 of the reference's, history within 1e-5 +
that * the L1 norm of the reference's loss gradient.  The fixtures' seed is one
at which the reference's fp32 and float64 fits agree within a quarter of the
parameter bar.
"""
import numpy as np
import pytest
import torch

import _metrics_ref as MR
import _mixed_ref as M
from _golden import rel_err
from cnf_hip import engine
from flows import flows as FL
from flows.normalizing_flows_torch import MixedFlow

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _fit(d, epochs=None, batch_size=None, **kw):
    from calibrators import TorchFlowCalibrator
    D = d["logits"].shape[1]
    torch.manual_seed(int(d["seed"]))
    return TorchFlowCalibrator(MixedFlow, d["logits"], np.eye(D)[d["labels"]],
                               layers=str(d["order"]),
                               epochs=int(d["epochs"]) if epochs is None else epochs,
                               batch_size=int(d["batch_size"]) if batch_size is None else batch_size,
                               dev=torch.device(DEV), **kw)


def _params(cal):
    return torch.cat([p.detach().reshape(-1).cpu() for p in cal.flow.parameters()]).numpy()


def _set_params(flow, flat):
    off = 0
    with torch.no_grad():
        for p in flow.parameters():
            n = p.numel()
            p.copy_(torch.from_numpy(np.asarray(flat[off:off + n], dtype=np.float32)).reshape(p.shape))
            off += n


def _hist(cal):
    return {k: np.array([float(v) for v in cal.history[k]]) for k in ("loss", "ce", "log_det")}


def _delta(fn):
    """(fn(), the launch counters that moved); "torch_ops" counts the route a
    launch took (the torch.library operators), not a launch."""
    before = dict(engine.stats)
    out = fn()
    return out, {k: engine.stats[k] - before.get(k, 0) for k in engine.stats
                 if engine.stats[k] != before.get(k, 0) and k != "torch_ops"}


@pytest.mark.parametrize("name", ["full", "mb128"])
def test_calibrator_fit_matches_reference_run(name, monkeypatch):
    """Native fit (eager epoch + one graph of 4 epochs) against the reference's
    own CPU run."""
    d = M.load_cal(name)
    N, bs, epochs = d["logits"].shape[0], int(d["batch_size"]), int(d["epochs"])
    steps = epochs * -(-N // bs)
    assert np.array_equal(_params(_fit(d, epochs=0)), d["P0"])     # the reference's init draw

    def no_torch_step(self, *a, **k):
        raise AssertionError("torch.optim.Adam.step ran on the native path")
    monkeypatch.setattr(torch.optim.Adam, "step", no_torch_step)
    (cal), n = _delta(lambda: _fit(d))
    # launches issued (the captured ones count once, at capture)
    assert n.get("adam") == steps, "one Adam launch per training batch"
    assert n.get("mixed_loss_vjp") == steps
    assert not any(k.startswith(("planar_", "radial_", "affine_")) for k in n), n
    for p in cal.flow.parameters():
        assert float(cal.optimizer.state[p]["step"]) == steps
    pbar = steps * 1e-3 * 2e-2
    pdiff = float(np.max(np.abs(_params(cal) - d["P"])))
    # L1 norm of the reference's loss gradient at its final parameters (CPU)
    flow = MixedFlow(3, layers=str(d["order"]))
    _set_params(flow, d["P"])
    x = torch.as_tensor(d["logits"] - d["logits"].mean(axis=1, keepdims=True), dtype=torch.float)
    y = torch.as_tensor(d["labels"])
    z, ld = flow(x)
    ce = torch.log(torch.softmax(z, dim=1).gather(1, y.view(-1, 1)) + 1e-7)
    (-torch.mean(ce.squeeze() + ld)).backward()
    g1 = float(sum(p.grad.abs().sum() for p in flow.parameters()))
    hbar = 1e-5 + pbar * g1
    h = _hist(cal)
    hdiff = {k: float(np.max(np.abs(h[k] - d[k]) / (np.abs(d[k].astype(np.float64)) + 1)))
             for k in h}
    print("%s: params %.2e (bar %.2e) history %s (bar %.2e)" % (name, pdiff, pbar, hdiff, hbar))
    assert len(h["loss"]) == epochs and np.isfinite(h["loss"]).all()
    assert h["log_det"].all() and d["log_det"].all()
    assert cal.history["loss"][0].device.type == "cuda"      # no host sync per epoch
    assert pdiff <= pbar
    assert max(hdiff.values()) <= hbar


@pytest.mark.parametrize("name", ["full", "mb128"])
def test_graph_replay_equals_eager_epochs(name):
    """53 epochs: one eager, one replay of 50, two eager tail epochs -- against
    53 eager epochs, bitwise."""
    d = M.load_cal(name)
    a = _fit(d, epochs=53)
    b = _fit(d, epochs=53, cnf_graph=False)
    assert np.array_equal(_params(a), _params(b))
    ha, hb = _hist(a), _hist(b)
    assert all(np.array_equal(ha[k], hb[k]) for k in ha) and len(ha["loss"]) == 53
    steps = 53 * -(-300 // int(d["batch_size"]))
    for cal in (a, b):
        for p in cal.flow.parameters():
            assert float(cal.optimizer.state[p]["step"]) == steps


def test_calibrator_predict_evaluate_and_score_on_device():
    import calibrators as C
    d = M.load_cal("mb128")
    cal = _fit(d)
    held = d["held"]
    got, n = _delta(lambda: cal.predict(held))
    assert n == {"mixed_predict": 1} and got.dtype == np.float64
    # the host path through predict_post, softmaxes in NumPy
    host, n = _delta(lambda: C.Calibrator.predict(cal, held))
    assert "mixed_predict" not in n and rel_err(got, host) <= 1e-5
    # the reference's recorded predict of its own fit
    perr = float(np.max(np.abs(got - d["pred"])))
    print("predict vs the reference's record: %.2e" % perr)
    assert perr <= 1e-5
    y = np.random.RandomState(71).randint(0, 3, size=held.shape[0])
    ref = MR.score(got, y, 15)
    sums, n = _delta(lambda: cal.evaluate_sums(held, y))
    assert n == {"mixed_predict": 1, "metrics": 1}
    MR.check_record_counts(sums.record, ref, 15)
    hv = C.Calibrator.evaluate(cal, held, y)
    for logits in (held, torch.as_tensor(held, dtype=torch.float32).to(DEV)):
        sc, n = _delta(lambda: cal.score(logits, y))
        assert n == {"mixed_score": 1}                  # one launch, no predict, no cnf_metrics
        assert sc == cal.evaluate(held, y)
        assert sc["n"] == hv["n"] == held.shape[0]
        assert abs(sc["ece"] - hv["ece"]) <= 1e-6
        assert abs(sc["accuracy"] - hv["accuracy"]) <= 1e-12
        rows = np.arange(ref["n"])
        p32 = got.astype(np.float32)
        d32 = abs(float(np.mean(-np.log(p32[rows, y] + np.float32(1e-7)).astype(np.float64)))
                  - hv["nll"])
        assert abs(sc["nll"] - hv["nll"]) <= 4 * d32 + 2.0 ** -32


def test_predict_matches_the_reference_at_its_parameters():
    """The recorded `pred` is the reference's predict at ITS final parameters:
    a calibrator holding exactly those parameters reproduces it at 1e-5."""
    d = M.load_cal("full")
    cal = _fit(d, epochs=0)
    _set_params(cal.flow, d["P"])
    got, n = _delta(lambda: cal.predict(d["held"]))
    assert n == {"mixed_predict": 1}
    assert np.max(np.abs(got - d["pred"])) <= 1e-5


def test_switch_off_takes_no_mixed_launch(monkeypatch):
    monkeypatch.setattr(FL, "MIXED_NATIVE", False)
    d = M.load_cal("full")
    held = d["held"]
    (cal, probs), n = _delta(lambda: (lambda c: (c, c.predict(held)))(_fit(d, epochs=2)))
    _, n2 = _delta(lambda: cal.score(held, np.zeros(held.shape[0], dtype=np.int64)))
    assert not any(k.startswith("mixed_") or k == "adam" for k in list(n) + list(n2))
    assert np.isfinite(probs).all() and len(cal.history["loss"]) == 2
    h = _hist(cal)
    assert rel_err(h["log_det"], d["log_det"][:2]) <= 1e-5 and rel_err(h["loss"], d["loss"][:2]) <= 1e-5
