"""cnf_pav_predict on the device (include/cnf.h; cnf_hip/pav.py;
calibrators.PAVCalibrator) through ctypes and through the torch operator:
the calibrator (host fit, device predict) against the reference's recorded
predictions (tests/golden/pav), predict from an uploaded model on the LDS and
the global-memory path against the restatement (tests/_pav_ref.py), wide rows
past one pass of the grid, repeatability, graph replay, a side stream and bad
labels.  Measured maxima are printed and recorded (conftest.RECORDS ->
pav_errors.jsonl)."""
import numpy as np
import pytest
import torch

import _pav_ref as R
from cnf_hip import _lib, engine, pav

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# fp32 output rounding 2^-24 plus the <= 1e-7 ramp bound of gen_golden_pav.py
# (a device score differs from NumPy's by a few float64 ulps), with a factor
# two in hand.  Measured maximum: 3.0e-8 on every fixture and model (DESIGN.md,
# "Isotonic calibration").
ATOL = 2.0 ** -22


@pytest.fixture(params=["ctypes", "torch_op"])
def path(request):
    old = engine.USE_TORCH_OPS
    engine.USE_TORCH_OPS = request.param == "torch_op"
    yield request.param
    engine.USE_TORCH_OPS = old


@pytest.fixture(scope="module")
def fx():
    return {n: R.load(n) for n in R.FIXTURES}


def _record(row):
    import conftest
    conftest.RECORDS.setdefault("pav_errors", []).append(row)
    print("pav_errors", row)


# ---- 1. end to end -----------------------------------------------------------------
def _fit_cal(f, target="labels", as_tensor=True):
    import calibrators as C
    D = f["x"].shape[1]
    t = f["y"] if target == "labels" else np.eye(D)[f["y"]]
    t = torch.from_numpy(t).to(DEV) if as_tensor else t
    return C.PAVCalibrator(torch.from_numpy(f["x"]).to(DEV), t)


@pytest.mark.parametrize("name", R.FIXTURES)
def test_end_to_end_against_the_reference(fx, path, name):
    f = fx[name]
    cal = _fit_cal(f)
    assert [len(px) for px, _ in cal.models] == f["n_thr"].tolist()
    for (px, py), (rx, ry) in zip(cal.models, f["thr"]):
        assert np.max(np.abs(px - rx)) <= 4e-16 and np.max(np.abs(py - ry)) <= 4e-16
    n0 = engine.stats["pav_predict"]
    got = cal.predict(torch.from_numpy(f["held"]).to(DEV))
    assert engine.stats["pav_predict"] == n0 + 1
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == f["held"].shape
    got = got.cpu().numpy().astype(np.float64)
    want = f["pred"]
    assert (np.isnan(got) == np.isnan(want)).all()
    ok = ~np.isnan(want)
    err = float(np.max(np.abs(got[ok] - want[ok]), initial=0.0))
    _record({"test": "end_to_end", "path": path, "fixture": name, "max_abs_err": err,
             "nan": int((~ok).sum())})
    assert err <= ATOL
    if name in R.MODERATE:
        assert ok.all()


@pytest.mark.parametrize("name", ["ties", "degen"])
def test_targets_in_every_form_give_one_model(fx, name):
    f = fx[name]
    held = torch.from_numpy(f["held"]).to(DEV)
    base = _fit_cal(f).predict(held)
    for target, as_tensor in (("labels", False), ("onehot", True), ("onehot", False)):
        other = _fit_cal(f, target, as_tensor).predict(held)
        assert torch.equal(base.view(torch.int32), other.view(torch.int32)), (target, as_tensor)


@pytest.mark.parametrize("name", R.MODERATE)
def test_evaluate_against_the_recorded_probabilities(fx, name):
    """evaluate of a ROCm tensor (predict, then cnf_metrics on the device)
    against utils.metrics on the reference's recorded float64 probabilities,
    at the bars of tests/test_gpu_metrics.py."""
    from utils import metrics as M
    f = fx[name]
    cal = _fit_cal(f)
    n = f["held"].shape[0]
    yh = np.random.RandomState(5).randint(0, f["x"].shape[1], size=n)
    got = cal.evaluate(torch.from_numpy(f["held"]).to(DEV), yh)
    p = f["pred"]
    host = {"nll": M.neg_log_likelihood(p, yh), "ece": M.expected_calibration_error(p, yh),
            "accuracy": M.accuracy(p, yh)}
    p32 = p.astype(np.float32)
    d32 = abs(float(np.mean(-np.log(p32[np.arange(n), yh] + np.float32(1e-7)).astype(np.float64)))
              - host["nll"])
    _record({"test": "evaluate", "fixture": name, "nll_err": abs(got["nll"] - host["nll"]),
             "nll_bar": 4 * d32 + 2.0 ** -32, "ece_err": abs(got["ece"] - host["ece"])})
    assert got["n"] == n
    assert abs(got["accuracy"] - host["accuracy"]) <= 1e-12
    assert abs(got["ece"] - host["ece"]) <= 1e-6
    assert abs(got["nll"] - host["nll"]) <= 4 * d32 + 2.0 ** -32


# ---- 2. predict from an uploaded model ----------------------------------------------
def _synthetic_model(counts, seed):
    """Per class `counts[c]` points: x strictly increasing inside [0.05, 0.6]
    (so scores fall outside on both sides), y non-decreasing in [0, 1] with
    flat stretches."""
    rs = np.random.RandomState(seed)
    points = []
    for n in counts:
        steps = rs.randint(1, 1 << 10, size=n).astype(np.float64)
        px = 0.05 + 0.55 * np.cumsum(steps) / (steps.sum() + 1.0)
        py = np.sort(np.round(rs.random_sample(n), 2))
        points.append((px, py))
    return points


@pytest.mark.parametrize("case", ["golden", "lds", "global"])
def test_predict_from_an_uploaded_model(fx, path, case):
    """golden: the recorded thresholds of `ties`; lds: a class with one point
    next to wider ones, D * cap <= 2048; global: the same with tables past the
    LDS budget (a fit of 65,537 noisy monotone rows leaves some n^(1/3) blocks,
    far below it, so the tables are built directly).  B = 1,077: a ragged last
    block; scores on both sides of [X_min, X_max]."""
    if case == "golden":
        f = fx["ties"]
        points, x, lp = f["thr"], f["held"], f["log_priors"]
    else:
        points = _synthetic_model((1, 40, 7) if case == "lds" else (1, 1500, 700), 41)
        x = (1.5 * np.random.RandomState(42).standard_normal((1077, 3))).astype(np.float32)
        lp = np.log(np.array([0.2, 0.5, 0.3]))
    model = pav.PavModel.from_host(points, torch.device(DEV))
    entries = model.thr_x.shape[0] * model.thr_x.shape[1]
    assert (entries > _lib.PAV_LDS_ENTRIES) == (case == "global")
    sc = R.scores(x)
    if case != "golden":
        assert (sc[:, 1] < points[1][0][0]).any() and (sc[:, 1] > points[1][0][-1]).any()
    want = R.predict(points, x, lp)
    got = pav.predict(torch.from_numpy(x).to(DEV), model, lp).cpu().numpy().astype(np.float64)
    err = float(np.max(np.abs(got - want)))
    _record({"test": "predict_model", "path": path, "case": case, "max_abs_err": err})
    assert err <= ATOL


def test_predict_wide_rows_grid_stride(path):
    """D = 100 and 256 (16 and 64 lanes per row); B = 4,099 rows of D = 100 is
    past one pass of the grid (1,024 blocks of 4 rows)."""
    for D, B in ((100, 4099), (256, 130), (17, 300), (10, 257)):
        points = _synthetic_model([1 + (7 * c) % 23 for c in range(D)], D)
        x = np.random.RandomState(D).standard_normal((B, D)).astype(np.float32)
        for px, _ in points:   # scores of D classes are ~1/D: bring the tables there
            px *= 4.0 / D
        lp = np.log(np.full(D, 1.0 / D))
        want = R.predict(points, x, lp)
        model = pav.PavModel.from_host(points, torch.device(DEV))
        got = pav.predict(torch.from_numpy(x).to(DEV), model, lp).cpu().numpy().astype(np.float64)
        assert np.max(np.abs(got - want)) <= ATOL, (D, B)


# ---- 3. other properties ---------------------------------------------------------------
def test_repeatable_graph_replay_and_side_stream(fx):
    f = fx["ties"]
    held = torch.from_numpy(f["held"]).to(DEV)
    model = pav.PavModel.from_host(f["thr"], torch.device(DEV))
    lp = torch.from_numpy(f["log_priors"]).to(DEV)
    p1, p2 = pav.predict(held, model, lp), pav.predict(held, model, lp)
    assert torch.equal(p1.view(torch.int32), p2.view(torch.int32))
    s = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        ps = pav.predict(held, model, lp)   # a side stream
        s.synchronize()
        assert torch.equal(ps.view(torch.int32), p1.view(torch.int32))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            rep = pav.predict(held, model, lp)
        rep.zero_()
        g.replay()
        s.synchronize()
    assert torch.equal(rep.view(torch.int32), p1.view(torch.int32))


def test_bad_labels_are_refused(fx):
    import calibrators as C
    f = fx["mod"]
    xd = torch.from_numpy(f["x"]).to(DEV)
    for bad in (-1, 4):
        y = f["y"].copy()
        y[17] = bad
        with pytest.raises(ValueError):
            C.PAVCalibrator(xd, torch.from_numpy(y).to(DEV))


def test_host_fitted_model_serves_host_and_device_inputs(fx):
    import calibrators as C
    f = fx["mod"]
    cal = C.PAVCalibrator(f["x"].astype(np.float64), f["y"])
    host = cal.predict(f["held"].astype(np.float64))
    assert isinstance(host, np.ndarray) and np.max(np.abs(host - f["pred"])) <= 1e-15
    n0 = engine.stats["pav_predict"]
    got = cal.predict(torch.from_numpy(f["held"]).to(DEV))
    assert engine.stats["pav_predict"] == n0 + 1
    assert got.is_cuda and np.max(np.abs(got.cpu().numpy() - f["pred"])) <= ATOL
