"""cnf_metrics on the device (include/cnf.h; cnf_hip/metrics.py): the integer
calibration record of every scoring fixture, through ctypes and through
torch.ops.cnf.metrics, against the float64 restatement of the reference's
utils/metrics.py (tests/_metrics_ref.py); shapes that break the tilings, ties,
accumulation, graph replay, invalid rows, and the calibrator's evaluate."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _metrics_ref as R
from _golden import GOLDEN
from cnf_hip import _lib, engine
from cnf_hip.metrics import CalibrationSums, calibration_record, record_words

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ctypes_record(p, y, bins, rec=None):
    """One cnf_metrics call through the C ABI on the current stream."""
    if rec is None:
        rec = torch.zeros(record_words(bins), dtype=torch.int64, device=p.device)
    st = _lib.lib().cnf_metrics(engine._ptr(p), engine._ptr(y), ctypes.c_int32(p.shape[1]),
                                ctypes.c_int32(bins), ctypes.c_int64(p.shape[0]),
                                engine._ptr(rec), ctypes.c_void_p(0), ctypes.c_size_t(0),
                                engine._stream(p.device))
    _lib.check("cnf_metrics", st)
    return rec


def _op_record(p, y, bins, rec=None):
    if rec is None:
        rec = torch.zeros(record_words(bins), dtype=torch.int64, device=p.device)
    _lib.torch_ops().metrics(p, y, bins, rec)
    return rec


PATHS = {"ctypes": _ctypes_record, "torch_op": _op_record}


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in R.FIXTURES:
        f = R.load(name)
        out[name] = (f, R.score(f["probs"], f["y"], int(f["bins"])),
                     torch.from_numpy(f["probs"]).to(DEV), torch.from_numpy(f["y"]).to(DEV))
    return out


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", R.FIXTURES)
def test_fixture_records(cases, name, path):
    """Counts and conf_fx exact, ECE within 1e-9 (2^-33 per row of fixed point
    plus float64 rounding).  NLL: the device's distance from the float64
    value is held to 4x the distance of an fp32 NumPy restatement (np.log on
    fp32 is correctly rounded, the device log need not be) plus 2^-32; both
    distances are recorded (conftest RECORDS -> metrics_errors.jsonl)."""
    import conftest
    f, ref, p, y = cases[name]
    bins = int(f["bins"])
    rec = PATHS[path](p, y, bins).cpu().numpy()
    R.check_record_counts(rec, ref, bins)
    s = CalibrationSums(rec, bins)
    assert abs(s.ece() - ref["ece"]) <= 1e-9
    assert abs(s.ece() - float(f["ece"])) <= 1e-6   # the reference's own number
    assert s.accuracy() == ref["acc"]
    rows = np.arange(ref["n"])
    t32 = -np.log(f["probs"][rows, f["y"]] + np.float32(1e-7))
    assert t32.dtype == np.float32
    d32 = abs(float(np.mean(t32.astype(np.float64))) - ref["nll"])
    ddev = abs(s.nll() - ref["nll"])
    conftest.RECORDS.setdefault("metrics_errors", []).append(
        {"fixture": name, "path": path, "nll_fp64": ref["nll"], "fp32_numpy_dist": d32,
         "device_dist": ddev, "ece_dist": abs(s.ece() - ref["ece"])})
    print("metrics_errors %s %s fp32=%.3e device=%.3e" % (name, path, d32, ddev))
    assert ddev <= 4 * d32 + 2.0 ** -32, (name, path, ddev, d32)


def _compare(p_np, y_np, bins, p_dev=None):
    ref = R.score(p_np, y_np, bins)
    p = torch.from_numpy(p_np).to(DEV) if p_dev is None else p_dev
    rec = calibration_record(p, torch.from_numpy(y_np).to(DEV), bins).cpu().numpy()
    R.check_record_counts(rec, ref, bins)
    assert abs(CalibrationSums(rec, bins).ece() - ref["ece"]) <= 1e-9
    assert abs(CalibrationSums(rec, bins).nll() - ref["nll"]) <= 1e-9
    return rec


@pytest.mark.parametrize("B", [1, 63, 64, 65, 4099, 70001])
def test_batch_sizes(B):
    """One row, around one pass of a block (64 rows at 4 lanes per row), more
    rows than one pass of the whole grid (512 blocks x 64 rows = 32,768)."""
    _compare(*R.softmax_rows(B, 10, 100 + B), 15)


@pytest.mark.parametrize("D", [2, 3, 16, 17, 33, 100, 256])
def test_widths(D):
    """Both sides of every lanes-per-row threshold (16 | 17, 64 | 100), widths
    below the group size and the widest row."""
    n0 = engine.stats["metrics"]
    _compare(*R.softmax_rows(129, D, 200 + D), 15)
    assert engine.stats["metrics"] == n0 + 1


def test_row_view_takes_contiguous_copy():
    """A non-contiguous, 4-byte-aligned view of the rows scores as its copy."""
    p_np, y_np = R.softmax_rows(129, 10, 31)
    wide = torch.zeros(129, 13, device=DEV)
    wide[:, 1:11] = torch.from_numpy(p_np).to(DEV)
    view = wide[:, 1:11]
    assert not view.is_contiguous() and view.data_ptr() % 16 == 4
    _compare(p_np, y_np, 15, p_dev=view)


def test_ties_across_lane_groups():
    """D=100 (64 lanes per row): the maximum duplicated in columns 3 and 67
    sits in two lanes' (value, index) pairs; the first index wins."""
    p_np, y_np = R.softmax_rows(64, 100, 41)
    p_np[:, 3] = p_np[:, 67] = p_np.max(axis=1) * np.float32(1.5)
    y_np[:32], y_np[32:] = 3, 67
    rec = _compare(p_np, y_np, 15)
    assert rec[3] == 32


def test_accumulation_and_repeatability(cases):
    f, ref, p, y = cases["m1"]
    one = calibration_record(p, y, 15)
    h = p.shape[0] // 2
    two = calibration_record(p[:h], y[:h], 15)
    assert calibration_record(p[h:], y[h:], 15, record=two) is two
    assert torch.equal(one, two)
    assert torch.equal(one, calibration_record(p, y, 15))
    assert torch.equal(one, _ctypes_record(p, y, 15))


def test_graph_replay_accumulates(cases):
    f, ref, p, y = cases["m1"]
    eager = calibration_record(p, y, 15)
    rec = torch.zeros_like(eager)
    calibration_record(p, y, 15, record=rec)  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        calibration_record(p, y, 15, record=rec)
    rec.zero_()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(rec, 3 * eager)


def test_invalid_rows_land_in_n_invalid_only():
    p_np, y_np = R.softmax_rows(200, 10, 51)
    keep = np.ones(200, dtype=bool)
    keep[[5, 77, 130, 199]] = False
    clean = calibration_record(torch.from_numpy(p_np[keep]).to(DEV),
                               torch.from_numpy(y_np[keep]).to(DEV), 15)
    y_np[5], y_np[77] = -1, 10
    p_np[130, 4] = np.nan
    p_np[199, 9] = np.inf
    rec = calibration_record(torch.from_numpy(p_np).to(DEV), torch.from_numpy(y_np).to(DEV), 15)
    want = clean.clone()
    want[1] = 4
    assert torch.equal(rec, want)
    assert np.isnan(CalibrationSums(rec, 15).nll()) and CalibrationSums(rec, 15).n == 196


def test_dropin_metrics_take_the_native_path(cases):
    from utils import metrics as M
    f, ref, p, y = cases["m3"]
    n0 = engine.stats["metrics"]
    ece = M.expected_calibration_error(p, y, bins=10)
    acc = M.accuracy(p, y)
    nll = M.neg_log_likelihood(p, y)
    assert engine.stats["metrics"] == n0 + 3
    assert isinstance(ece, float) and abs(ece - ref["ece"]) <= 1e-9
    assert acc == ref["acc"] and abs(nll - ref["nll"]) <= 1e-9


def test_calibrator_evaluate_on_device():
    """g7's data, a short fit on cuda:0: evaluate_sums' count words equal the
    restatement applied to cal.predict(x_test); evaluate agrees with the host
    path Calibrator.evaluate (predict's D2H copy, then utils.metrics)."""
    import calibrators as C
    from flows.realNVP_torch import RealNvpFlow
    f = np.load(os.path.join(GOLDEN, "g7_calibrator_d3.npz"))
    meta = json.loads(str(f["meta"]))
    torch.manual_seed(meta["seed"])
    np.random.seed(meta["seed"])
    cal = C.TorchFlowCalibrator(RealNvpFlow, f["x"].astype(np.float64), f["y"], layers=5,
                                hidden_size=[3, 3], epochs=3, dev=torch.device(DEV))
    x_test = f["x_test"].astype(np.float64)
    y_test = np.random.RandomState(78).randint(0, 3, size=x_test.shape[0])  # gen_golden.py:49-52
    ref = R.score(cal.predict(x_test), y_test, 15)
    n0 = engine.stats["metrics"]
    sums = cal.evaluate_sums(x_test, y_test)
    assert engine.stats["metrics"] == n0 + 1
    R.check_record_counts(sums.record, ref, 15)
    got = cal.evaluate(x_test, y_test)
    host = C.Calibrator.evaluate(cal, x_test, y_test)
    assert got["n"] == host["n"] == x_test.shape[0]
    assert abs(got["ece"] - host["ece"]) <= 1e-6        # the reference's fp32 hit mean
    assert abs(got["ece"] - ref["ece"]) <= 1e-9
    assert abs(got["accuracy"] - host["accuracy"]) <= 1e-12
    rows = np.arange(ref["n"])
    p32 = cal.predict(x_test).astype(np.float32)
    d32 = abs(float(np.mean(-np.log(p32[rows, y_test] + np.float32(1e-7)).astype(np.float64)))
              - host["nll"])
    assert abs(got["nll"] - host["nll"]) <= 4 * d32 + 2.0 ** -32


def test_calibrator_evaluate_with_predict_fallback():
    """A stack cnf_predict does not serve (hidden [10, 10] at D=10 runs on
    k_valu; its predict is cnf_forward plus device torch ops) still scores on
    the device: same count words as the restatement on cal.predict."""
    import calibrators as C
    from flows.realNVP_torch import RealNvpFlow
    rs = np.random.RandomState(9)
    y = rs.randint(0, 10, size=300)
    x = rs.standard_normal((300, 10))
    x[np.arange(300), y] += 2.0
    torch.manual_seed(1)
    np.random.seed(1)
    cal = C.TorchFlowCalibrator(RealNvpFlow, x, y, layers=2, hidden_size=[10, 10], epochs=1,
                                dev=torch.device(DEV))
    ref = R.score(cal.predict(x), y, 15)
    n0, p0 = engine.stats["metrics"], engine.stats["predict"]
    sums = cal.evaluate_sums(x, y)
    assert engine.stats["metrics"] == n0 + 1
    assert engine.stats["predict"] == p0, "expected the torch fallback of predict"
    R.check_record_counts(sums.record, ref, 15)
    assert abs(sums.ece() - ref["ece"]) <= 1e-9
