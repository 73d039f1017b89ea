"""The planar calibrator path on the GPU: the fused predict
(cnf_planar_predict) against the reference's float64 record
(tests/golden/planar_predict) and the float64 restatement
tests/_planar_predict_ref.py, the one-launch Adam over a tensor list
(cnf_adam_step_tensors) against torch.optim.Adam, and TorchFlowCalibrator's
native planar fit (HIP-graph epochs included), predict and evaluate against
the reference's own run (tests/golden/planar_cal).

Bars.  Probabilities and log-det: max(1e-5, 2 * floor) under _golden.rel_err,
floor = the reference's own fp32-vs-float64 error recorded with the fixture
(_planar_ref.bar).  Adam: the bar of tests/test_gpu_adam.py.  Calibrator fit:
the bars tests/test_gpu_planar.py derives (parameters steps * lr * 2e-2,
history 1e-5 + that * the L1 norm of the loss gradient).
"""
import numpy as np
import pytest
import torch

import _metrics_ref as MR
import _planar_predict_ref as PR
import _planar_ref as R
from _golden import rel_err
from cnf_hip import engine
from cnf_hip.adam import StackAdam
from conftest import RECORDS
from flows import flows as FL
from flows._factory import PlanarFlow

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FINITE = ["one", "d3", "d10", "d17", "d100"]
_cache = {}


def fx(name):
    """(fixture arrays, PlanarStack on the device, x and log-priors on the
    device), loaded once."""
    if name not in _cache:
        d = PR.load(name)
        flow = R.build_flow(d, DEV)
        _cache[name] = (d, flow._planar_stack(), torch.from_numpy(d["x"]).to(DEV),
                        torch.as_tensor(d["log_priors"], dtype=torch.float32, device=DEV), flow)
    return _cache[name][:4]


# ---- the fused predict -------------------------------------------------------------

@pytest.mark.parametrize("name", FINITE)
def test_predict_matches_float64_record(name):
    d, stack, x, lp = fx(name)
    n0 = engine.stats["planar_predict"]
    probs, ld = stack.predict(x, lp, want_logdet=True)
    assert engine.stats["planar_predict"] == n0 + 1
    p, l = probs.cpu().numpy(), ld.cpu().numpy()
    ep, el = rel_err(p, d["probs64"]), rel_err(l, d["ld64"])
    pb, lb = R.bar(d["floor_probs"]), R.bar(d["floor_ld"])
    print("%s: probs %.2e (bar %.2e) ld %.2e (bar %.2e)" % (name, ep, pb, el, lb))
    RECORDS.setdefault("planar_predict_parity", []).append(
        {"fixture": name, "probs": ep, "probs_bar": pb, "ld": el, "ld_bar": lb})
    assert ep <= pb and el <= lb
    assert np.abs(p.astype(np.float64).sum(axis=1) - 1).max() <= 1e-6
    assert torch.equal(stack.predict(x, lp), probs)          # without the log-det


@pytest.mark.parametrize("name", ["nan", "inf"])
def test_nan_positions_coincide(name):
    d, stack, x, lp = fx(name)
    probs, ld = stack.predict(x, lp, want_logdet=True)
    p = probs.cpu().numpy()
    assert (np.isnan(p) == np.isnan(d["probs64"])).all()
    assert (np.isnan(p) == np.isnan(d["probs"])).all()
    assert np.isnan(p).all()                                  # what the reference recorded
    assert rel_err(ld.cpu().numpy(), d["ld64"]) <= R.bar(d["floor_ld"])


@pytest.mark.parametrize("name,B", [(n, b) for n in ("d3", "d10") for b in (255, 256, 257)]
                         + [("d17", b) for b in (15, 16, 17)]
                         + [("d100", b) for b in (3, 4, 5)])
def test_batch_edges(name, B):
    """Each side of a block's row count: 256 rows (one lane per row), 16 rows
    (16 lanes per row), 4 rows (64 lanes per row)."""
    d, stack, x, lp = fx(name)
    probs, ld = stack.predict(x[:B], lp, want_logdet=True)
    assert probs.shape == (B, x.shape[1]) and ld.shape == (B,)
    assert rel_err(probs.cpu().numpy(), d["probs64"][:B]) <= R.bar(d["floor_probs"])
    assert rel_err(ld.cpu().numpy(), d["ld64"][:B]) <= R.bar(d["floor_ld"])


def _random_params(rs, D, L):
    params = [((rs.standard_normal(D) * 0.5).astype(np.float32),
               (rs.standard_normal(D) * 0.5).astype(np.float32),
               (rs.standard_normal(1) * 0.5).astype(np.float32)) for _ in range(L)]
    d = {"W": np.stack([p[0] for p in params]), "U": np.stack([p[1] for p in params]),
         "Bv": np.concatenate([p[2] for p in params])}
    return params, R.build_flow(d, DEV)


def test_one_row_past_the_grid_cap():
    """256 rows per pass x 1024 blocks + 1: block 0 takes a second pass of one
    row.  The sampled rows are well conditioned (min |1 + h'c| = 0.45 in
    float64), so the project's 1e-5 holds for the log-det."""
    B, D, L = 1024 * 256 + 1, 3, 2
    rs = np.random.RandomState(51)
    params, flow = _random_params(rs, D, L)
    xh = rs.standard_normal((B, D)).astype(np.float32)
    lph = np.log(np.array([0.2, 0.3, 0.5]))
    probs, ld = flow._planar_stack().predict(torch.from_numpy(xh).to(DEV), lph, want_logdet=True)
    idx = np.concatenate([[0], np.sort(rs.choice(B - 2, 2048, replace=False)) + 1, [B - 1]])
    pr, lr = PR.predict(params, xh[idx], lph)
    assert rel_err(probs[idx].cpu().numpy(), pr) <= 1e-5
    assert rel_err(ld[idx].cpu().numpy(), lr) <= 1e-5
    assert bool(torch.isfinite(probs).all())


@pytest.mark.parametrize("name", ["d3", "d10", "d17"])
def test_views(name):
    """x[1:] starts D floats into the buffer (4-byte aligned only for odd D); an
    odd number of floats B * D; a column slice of a wider buffer, which is not
    contiguous."""
    d, stack, x, lp = fx(name)
    B, D = x.shape
    ref = stack.predict(x, lp)
    assert torch.equal(stack.predict(x[1:], lp), ref[1:])
    wide = torch.zeros(B, D + 3, device=DEV)
    wide[:, 1:D + 1] = x
    view = wide[:, 1:D + 1]
    assert not view.is_contiguous()
    assert torch.equal(stack.predict(view, lp), ref)
    if D % 2:
        Bo = B if B % 2 else B - 1
        assert (Bo * D) % 2 == 1
        assert torch.equal(stack.predict(x[:Bo], lp), ref[:Bo])


@pytest.mark.parametrize("name", FINITE)
def test_predict_equals_the_composition(name):
    """Device torch ops around PlanarStack.run: what predict fuses."""
    d, stack, x, lp = fx(name)
    xc = x - x.mean(dim=1, keepdim=True)
    z, ld, _ = stack.run(xc)
    comp = torch.softmax(torch.log(torch.softmax(z, dim=1) + 1e-7) - lp, dim=1)
    probs, ld2 = stack.predict(x, lp, want_logdet=True)
    assert rel_err(probs.cpu().numpy(), comp.cpu().numpy()) <= R.bar(d["floor_probs"])
    assert rel_err(ld2.cpu().numpy(), ld.cpu().numpy()) <= R.bar(d["floor_ld"])


def test_stats_and_repeatability():
    for name in ("d10", "d17", "d100"):
        d, stack, x, lp = fx(name)
        n0 = engine.stats["planar_predict"]
        a = stack.predict(x, lp, want_logdet=True)
        assert engine.stats["planar_predict"] == n0 + 1
        b = stack.predict(x, lp, want_logdet=True)
        assert engine.stats["planar_predict"] == n0 + 2
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_wrong_prior_count():
    d, stack, x, lp = fx("d3")
    n0 = engine.stats["planar_predict"]
    with pytest.raises(ValueError, match="log_priors must have 3 entries"):
        stack.predict(x, np.zeros(4))
    assert engine.stats["planar_predict"] == n0


def test_million_rows_once():
    """2^20 x 10, L = 10: one call held to the restatement on 2,048 sampled
    rows (min |1 + h'c| = 0.54 over them in float64), and a second call
    bitwise equal."""
    B, D, L = 1 << 20, 10, 10
    rs = np.random.RandomState(61)
    params, flow = _random_params(rs, D, L)
    g = torch.Generator(device="cpu").manual_seed(62)
    xc = torch.randn(B, D, generator=g)
    lph = np.log(np.arange(1, D + 1) / (D * (D + 1) / 2.0))
    x = xc.to(DEV)
    stack = flow._planar_stack()
    probs, ld = stack.predict(x, lph, want_logdet=True)
    idx = np.arange(2048) * 509 + 23
    pr, lr = PR.predict(params, xc.numpy()[idx], lph)
    assert rel_err(probs[idx].cpu().numpy(), pr) <= 1e-5
    assert rel_err(ld[idx].cpu().numpy(), lr) <= 1e-5
    p2, l2 = stack.predict(x, lph, want_logdet=True)
    assert torch.equal(probs, p2) and torch.equal(ld, l2)


# ---- cnf_adam_step_tensors ---------------------------------------------------------

class _ListStack:
    """The least StackAdam asks of a stack: param_tensors() and param_count()."""

    def __init__(self, tensors):
        self.ts = list(tensors)

    def param_tensors(self):
        return self.ts

    def param_count(self):
        return sum(t.numel() for t in self.ts)


def _tensor_list(n, seed):
    g = torch.Generator().manual_seed(seed)
    sizes = [1 + (7 * i) % 13 for i in range(n)]
    if n >= 3:
        sizes[1] = 1500                       # more than one block of 256
    return [torch.randn(s, generator=g).to(DEV) for s in sizes]


@pytest.mark.parametrize("n,wd", [(3, 0.0), (200, 0.0), (200, 0.01)])
def test_adam_tensors_matches_torch_adam(n, wd):
    """5 steps on the same gradients; 200 tensors cross the 128-tensor chunk."""
    lr = 3e-3
    pa = _tensor_list(n, 1)
    pb = [torch.nn.Parameter(t.clone()) for t in pa]
    ta = torch.optim.Adam(pb, lr=lr, weight_decay=wd)
    na = StackAdam(_ListStack(pa), lr=lr, weight_decay=wd)
    g = torch.Generator().manual_seed(2)
    n0 = engine.stats.get("adam", 0)
    for _ in range(5):
        flat = torch.randn(na.stack.param_count(), generator=g).to(DEV)
        na.step(flat)
        off = 0
        for p in pb:
            p.grad = flat[off:off + p.numel()].clone()
            off += p.numel()
        ta.step()
    assert engine.stats["adam"] == n0 + 5 and na.t == 5
    for i, (p, q) in enumerate(zip(pa, pb)):
        assert ((p - q).abs() / (q.abs() + 5 * lr)).max().item() <= 1e-4, i


def test_adam_tensors_sched_and_skip():
    """The sched form equals the scalar form bitwise; a set skip flag leaves
    parameters and moments untouched."""
    pa, pb = _tensor_list(200, 3), _tensor_list(200, 3)
    a, b = StackAdam(_ListStack(pa), lr=2e-3), StackAdam(_ListStack(pb), lr=2e-3)
    g = torch.Generator().manual_seed(4)
    for t in range(1, 4):
        flat = torch.randn(a.stack.param_count(), generator=g).to(DEV)
        a.step(flat)
        b.step_sched(flat, torch.tensor(b.sched_values(t), dtype=torch.float32, device=DEV))
    assert all(torch.equal(p, q) for p, q in zip(pa, pb))
    assert torch.equal(a._m, b._m) and torch.equal(a._v, b._v)
    keep = [p.clone() for p in pa], a._m.clone(), a._v.clone()
    flag = torch.ones(1, dtype=torch.int32, device=DEV)
    a.step(torch.randn(a.stack.param_count(), generator=g).to(DEV), skip=flag)
    assert all(torch.equal(p, q) for p, q in zip(pa, keep[0]))
    assert torch.equal(a._m, keep[1]) and torch.equal(a._v, keep[2])
    flag.zero_()
    a.step(torch.randn(a.stack.param_count(), generator=g).to(DEV), skip=flag)
    assert not torch.equal(pa[1], keep[0][1])


def test_adam_tensors_equals_desc_entry_point():
    """A coupling stack's tensors through cnf_adam_step_tensors and through
    cnf_adam_step (its descriptor): bitwise-equal parameters and moments."""
    from flows.flows import Flow, NvpCouplingLayer

    def flow():
        torch.manual_seed(5)
        return Flow([NvpCouplingLayer(10, [5, 5]) for _ in range(12)]).to(DEV)   # 144 tensors
    fa, fb = flow(), flow()
    sa, sb = fa._native_stack(), fb._native_stack()
    assert len(sa.param_tensors()) > 128
    a, b = StackAdam(sa, lr=3e-3), StackAdam(_ListStack(sb.param_tensors()), lr=3e-3)
    g = torch.Generator().manual_seed(6)
    for _ in range(3):
        flat = (torch.randn(sa.param_count(), generator=g) * 0.1).to(DEV)
        a.step(flat)
        b.step(flat)
    assert all(torch.equal(p, q) for p, q in zip(sa.param_tensors(), sb.param_tensors()))
    assert torch.equal(a._m, b._m) and torch.equal(a._v, b._v)


# ---- the calibrator ------------------------------------------------------------------

def _fit(d, epochs=None, batch_size=None, **kw):
    from calibrators import TorchFlowCalibrator
    L, D = d["W"].shape
    torch.manual_seed(int(d["seed"]))
    cal = TorchFlowCalibrator(PlanarFlow, d["logits"], np.eye(D)[d["labels"]], layers=L,
                              epochs=int(d["epochs"]) if epochs is None else epochs,
                              batch_size=int(d["batch_size"]) if batch_size is None else batch_size,
                              dev=torch.device(DEV), **kw)
    return cal


def _params(cal):
    return torch.cat([p.detach().reshape(-1).cpu() for p in cal.flow.parameters()]).numpy()


def _hist(cal):
    return {k: np.array([float(v) for v in cal.history[k]]) for k in ("loss", "ce", "log_det")}


def _fixture_params(d):
    return np.concatenate([np.concatenate([d["W"][l], d["U"][l], d["Bv"][l:l + 1]])
                           for l in range(d["W"].shape[0])])


@pytest.mark.parametrize("name", ["full", "mb128"])
def test_calibrator_fit_matches_reference_run(name, monkeypatch):
    """Native fit (eager epoch + one graph of 4 epochs) against the reference's
    own CPU run; bound as derived in tests/test_gpu_planar.py."""
    d = PR.load_cal(name)
    N, bs, epochs = d["logits"].shape[0], int(d["batch_size"]), int(d["epochs"])
    steps = epochs * -(-N // bs)

    def no_torch_step(self, *a, **k):
        raise AssertionError("torch.optim.Adam.step ran on the native path")
    monkeypatch.setattr(torch.optim.Adam, "step", no_torch_step)
    n_adam, n_vjp = engine.stats.get("adam", 0), engine.stats["planar_loss_vjp"]
    cal = _fit(d)
    # launches issued (the captured ones count once, at capture)
    assert engine.stats["adam"] == n_adam + steps, "one Adam launch per training batch"
    assert engine.stats["planar_loss_vjp"] == n_vjp + steps
    for p in cal.flow.parameters():
        assert float(cal.optimizer.state[p]["step"]) == steps
    pbar = steps * 1e-3 * 2e-2
    pdiff = float(np.max(np.abs(_params(cal) - _fixture_params(d))))
    # L1 norm of the reference's loss gradient at its final parameters (CPU)
    flow = R.build_flow(d)
    x = torch.as_tensor(d["logits"] - d["logits"].mean(axis=1, keepdims=True), dtype=torch.float)
    y = torch.as_tensor(d["labels"])
    zs, ld = flow(x)
    ce = torch.log(torch.softmax(zs[-1], dim=1).gather(1, y.view(-1, 1)) + 1e-7)
    (-torch.mean(ce.squeeze() + ld)).backward()
    g1 = float(sum(p.grad.abs().sum() for p in flow.parameters()))
    hbar = 1e-5 + pbar * g1
    h = _hist(cal)
    hdiff = {k: float(np.max(np.abs(h[k] - d[k]) / (np.abs(d[k].astype(np.float64)) + 1)))
             for k in h}
    print("%s: params %.2e (bar %.2e) history %s (bar %.2e)" % (name, pdiff, pbar, hdiff, hbar))
    RECORDS.setdefault("planar_calibrator_native", []).append(
        {"fixture": name, "steps": steps, "param_diff": pdiff, "param_bar": pbar,
         "history_diff": hdiff, "history_bar": hbar})
    assert len(h["loss"]) == epochs and np.isfinite(h["loss"]).all()
    assert pdiff <= pbar
    assert max(hdiff.values()) <= hbar


@pytest.mark.parametrize("name", ["full", "mb128"])
def test_graph_replay_equals_eager_epochs(name):
    """53 epochs: one eager, one replay of 50, two eager tail epochs -- against
    53 eager epochs, bitwise."""
    d = PR.load_cal(name)
    a = _fit(d, epochs=53)
    b = _fit(d, epochs=53, cnf_graph=False)
    assert np.array_equal(_params(a), _params(b))
    ha, hb = _hist(a), _hist(b)
    assert all(np.array_equal(ha[k], hb[k]) for k in ha) and len(ha["loss"]) == 53
    steps = 53 * -(-300 // int(d["batch_size"]))
    for cal in (a, b):
        for p in cal.flow.parameters():
            assert float(cal.optimizer.state[p]["step"]) == steps


def test_second_fit_continues():
    """fit(3 epochs) then fit(2 epochs) against 5 uninterrupted epochs: the
    step count and moments carry over through the torch optimizer's state."""
    d = PR.load_cal("mb128")
    bs = int(d["batch_size"])
    cal = _fit(d, epochs=3)
    h2 = cal.fit(cal.logits, cal.target, epochs=2, batch_size=bs)
    steps = 5 * -(-300 // bs)
    for p in cal.flow.parameters():
        assert float(cal.optimizer.state[p]["step"]) == steps
    one = _fit(d, epochs=5)
    pbar = steps * 1e-3 * 2e-2
    assert float(np.max(np.abs(_params(cal) - _params(one)))) <= pbar
    assert len(h2["loss"]) == 2


def test_unsupported_optimizer_keeps_the_torch_step():
    """AdamW: cnf_hip.adam.supports is false, so the per-batch loop with
    torch's own step runs (no native Adam launch)."""
    from calibrators import TorchFlowCalibrator
    d = PR.load_cal("full")
    torch.manual_seed(7)
    cal = TorchFlowCalibrator(PlanarFlow, d["logits"], np.eye(3)[d["labels"]], layers=4, epochs=0,
                              dev=torch.device(DEV))
    cal.optimizer = torch.optim.AdamW(cal.flow.parameters())
    n_adam, n_vjp = engine.stats.get("adam", 0), engine.stats["planar_loss_vjp"]
    h = cal.fit(cal.logits, cal.target, epochs=2, batch_size=300)
    assert engine.stats.get("adam", 0) == n_adam and engine.stats["planar_loss_vjp"] == n_vjp + 2
    assert len(h["loss"]) == 2 and np.isfinite([float(v) for v in h["loss"]]).all()


def test_calibrator_predict_and_evaluate_on_device():
    import calibrators as C
    d = PR.load_cal("mb128")
    cal = _fit(d)
    held = d["held"]
    n0 = engine.stats["planar_predict"]
    got = cal.predict(held)
    assert engine.stats["planar_predict"] == n0 + 1 and got.dtype == np.float64
    host = C.Calibrator.predict(cal, held)              # through predict_post, softmaxes in NumPy
    assert engine.stats["planar_predict"] == n0 + 1
    assert rel_err(got, host) <= 1e-5
    # evaluate: the record of the device probabilities, as the coupling test holds it
    y = np.random.RandomState(71).randint(0, 3, size=held.shape[0])
    ref = MR.score(got, y, 15)
    m0 = engine.stats["metrics"]
    sums = cal.evaluate_sums(held, y)
    assert engine.stats["metrics"] == m0 + 1 and engine.stats["planar_predict"] == n0 + 2
    MR.check_record_counts(sums.record, ref, 15)
    ev = cal.evaluate(held, y)
    hv = C.Calibrator.evaluate(cal, held, y)
    assert ev["n"] == hv["n"] == held.shape[0]
    assert abs(ev["ece"] - hv["ece"]) <= 1e-6
    assert abs(ev["ece"] - ref["ece"]) <= 1e-9
    assert abs(ev["accuracy"] - hv["accuracy"]) <= 1e-12
    rows = np.arange(ref["n"])
    p32 = got.astype(np.float32)
    d32 = abs(float(np.mean(-np.log(p32[rows, y] + np.float32(1e-7)).astype(np.float64)))
              - hv["nll"])
    assert abs(ev["nll"] - hv["nll"]) <= 4 * d32 + 2.0 ** -32
    # every call above but the first host one went through the fused predict
    assert engine.stats["planar_predict"] == n0 + 4
    curves = cal.detection_curves(held, y)
    assert engine.stats["planar_predict"] == n0 + 5 and curves is not None


def test_switch_off_takes_no_new_launch(monkeypatch):
    monkeypatch.setattr(FL, "PLANAR_NATIVE", False)
    d = PR.load_cal("full")
    n_p, n_a = engine.stats["planar_predict"], engine.stats.get("adam", 0)
    n_v = engine.stats["planar_loss_vjp"]
    cal = _fit(d, epochs=2)
    probs = cal.predict(d["held"])
    cal.evaluate(d["held"], np.zeros(d["held"].shape[0], dtype=np.int64))
    assert engine.stats["planar_predict"] == n_p and engine.stats.get("adam", 0) == n_a
    assert engine.stats["planar_loss_vjp"] == n_v
    assert np.isfinite(probs).all()
