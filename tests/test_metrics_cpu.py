"""Scoring without a GPU: the float64 restatement (tests/_metrics_ref.py)
against the reference's own numbers (tests/golden/metrics/m*.npz), the
drop-in utils.metrics host functions, the CPU-tensor calibration record, the
record math and the argument validation of the three C entry points."""
import ctypes

import numpy as np
import pytest
import torch

import _metrics_ref as R
from cnf_hip import _lib
from cnf_hip.metrics import CalibrationSums, calibration_record, record_words

FX = R.FX


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in R.FIXTURES:
        f = R.load(name)
        out[name] = (f, R.score(f["probs"], f["y"], int(f["bins"])))
    return out


@pytest.mark.parametrize("name", R.FIXTURES)
def test_restatement_matches_reference(cases, name):
    """nll and acc to 1e-12; ece to 1e-6: the reference averages the 0/1 hits
    of a bin in fp32 (metrics.py:54, 67), the restatement in float64.  Measured
    gaps on the fixtures: m1 5.0e-9, m2 5.9e-9, m3 7.2e-9, m4 5.5e-9."""
    f, ref = cases[name]
    assert f["probs"].dtype == np.float32 and f["y"].dtype == np.int64
    assert abs(ref["nll"] - float(f["nll"])) <= 1e-12
    assert abs(ref["acc"] - float(f["acc"])) <= 1e-12
    assert abs(ref["ece"] - float(f["ece"])) <= 1e-6


def test_m1_holds_every_edge_and_its_neighbours():
    """The fixture really exercises the edge rule: for every i/15 a confidence
    equal to fp32(edge) and to both fp32 neighbours (<= 1), and argmax ties."""
    f = R.load("m1")
    conf = f["probs"].max(axis=1)
    for i in range(1, 16):
        e = np.float32(i * (1. / 15))
        for c in (np.nextafter(e, np.float32(0)), e, np.nextafter(e, np.float32(2))):
            if c <= 1:
                assert (conf == c).any(), (i, c)
        if i < 15:
            # every inner edge rounds UP in fp32: a confidence of fp32(edge)
            # belongs to the next bin
            assert float(e) > i * (1. / 15)
    assert ((f["probs"] == f["probs"][:, :1]).all(axis=1)).sum() >= 2


@pytest.mark.parametrize("name", R.FIXTURES)
def test_dropin_host_metrics_match_reference(cases, name):
    from utils import metrics as M
    f, _ = cases[name]
    p64 = f["probs"].astype(np.float64)
    y, bins = f["y"], int(f["bins"])
    onehot = np.eye(p64.shape[1])[y]
    for target in (y, onehot):
        ece = M.expected_calibration_error(p64, target, bins=bins)
        assert isinstance(ece, float) and abs(ece - float(f["ece"])) <= 1e-6
    nll = M.neg_log_likelihood(p64, onehot)
    acc = M.accuracy(p64, onehot)
    assert isinstance(nll, float) and abs(nll - float(f["nll"])) <= 1e-12
    assert isinstance(acc, float) and abs(acc - float(f["acc"])) <= 1e-12
    if int(y.max()) + 1 == p64.shape[1]:  # label vectors: one-hot width = max + 1
        assert abs(M.neg_log_likelihood(p64, y) - float(f["nll"])) <= 1e-12
        assert abs(M.accuracy(p64, y) - float(f["acc"])) <= 1e-12


def test_dropin_binary_branch_and_helpers():
    """1-D binary scores: confidence |(1 - round(p)) - p|, prediction round(p)
    (metrics.py:50-52); onehot_encode; empirical_cross_entropy."""
    from utils import metrics as M
    from utils.ops import onehot_encode
    p = np.array([0.9, 0.2, 0.6, 0.4, 0.97, 0.03])
    t = np.array([1, 0, 0, 0, 1, 1])
    conf = np.where(p >= 0.5, p, 1 - p)
    hits = (np.around(p) == t).astype(np.float64)
    want = 0.
    for i in range(15):
        sel = (i / 15 < conf) & (conf <= (i + 1) / 15)
        if sel.any():
            want += abs(hits[sel].mean() - conf[sel].mean()) * sel.sum()
    assert abs(M.expected_calibration_error(p, t) - want / 6) <= 1e-6
    two = np.stack([1 - p, p], axis=1)
    assert abs(M.neg_log_likelihood(p, t) - M.neg_log_likelihood(two, t)) <= 1e-15
    oh = onehot_encode([2, 0, 1])
    assert oh.dtype == np.int32 and oh.tolist() == [[0, 0, 1], [1, 0, 0], [0, 1, 0]]
    lr = np.array([4.0, 0.5, 2.0, 0.25])
    tt = np.array([1, 0, 1, 0])
    want = 0.5 / 2 * np.sum(tt * np.log2(1 + 1 / lr)) + 0.5 / 2 * np.sum((1 - tt) * np.log2(1 + lr))
    assert abs(M.empirical_cross_entropy(lr, tt, 0.5) - want) <= 1e-15


@pytest.mark.parametrize("name", R.FIXTURES)
def test_cpu_tensor_record(cases, name):
    """The torch restatement fills the record the kernel fills: counts and
    conf_fx = sum rint(conf * 2^32) exactly; ece within 1e-9 (at most 2^-33
    per row from the fixed point, divided by n, plus float64 rounding)."""
    f, ref = cases[name]
    bins = int(f["bins"])
    rec = calibration_record(torch.from_numpy(f["probs"]), torch.from_numpy(f["y"]), bins)
    assert rec.dtype == torch.int64 and rec.device.type == "cpu"
    R.check_record_counts(rec.numpy(), ref, bins)
    want_nll_fx = int(np.rint(ref["nll_terms"] * FX).astype(np.int64).sum())
    assert abs(int(rec[2]) - want_nll_fx) <= ref["n"]  # log rounding: <= 1 unit per row
    s = CalibrationSums(rec, bins)
    assert s.n == ref["n"] and s.n_invalid == 0
    assert abs(s.ece() - ref["ece"]) <= 1e-9
    assert abs(s.nll() - ref["nll"]) <= 1e-9
    assert s.accuracy() == ref["acc"]
    cnt, conf, acc = s.reliability()
    np.testing.assert_array_equal(cnt, ref["count"])
    full = ref["count"] > 0
    np.testing.assert_allclose(conf[full], ref["conf_sum"][full] / ref["count"][full], atol=1e-9)
    np.testing.assert_array_equal(acc[full], ref["correct"][full] / ref["count"][full])
    assert np.isnan(conf[~full]).all() and np.isnan(acc[~full]).all()


def test_cpu_record_accumulates_and_splits(cases):
    f, _ = cases["m1"]
    p, y = torch.from_numpy(f["probs"]), torch.from_numpy(f["y"])
    one = calibration_record(p, y, 15)
    rec = calibration_record(p[:1000], y[:1000], 15)
    assert calibration_record(p[1000:], y[1000:], 15, record=rec) is rec
    assert torch.equal(rec, one)
    # float64 input (what predict returns) gives the same record as its fp32 source
    assert torch.equal(calibration_record(p.double(), y, 15), one)


def test_cpu_record_invalid_rows(cases):
    f, _ = cases["m3"]
    p = torch.from_numpy(f["probs"][:8].copy())
    y = torch.from_numpy(f["y"][:8].copy())
    clean = calibration_record(p[3:], y[3:], 10)
    y[0], y[1] = -1, 3
    p[2, 1] = float("nan")
    rec = calibration_record(p, y, 10)
    assert int(rec[1]) == 3
    want = clean.clone()
    want[1] = 3
    assert torch.equal(rec, want)
    assert np.isnan(CalibrationSums(rec, 10).nll())
    assert CalibrationSums(rec, 10).n == 5


def test_record_math_on_a_hand_written_record():
    bins = 3
    rec = np.zeros(record_words(bins), dtype=np.int64)
    rec[0], rec[1], rec[2], rec[3] = 10, 0, int(5.0 * FX), 7
    rec[4:7] = [0, 4, 6]
    rec[7:10] = [0, int(2.0 * FX), int(5.25 * FX)]   # mean conf 0.5 and 0.875
    rec[10:13] = [0, 1, 6]
    s = CalibrationSums(rec, bins)
    assert s.n == 10 and s.nll() == 0.5 and s.accuracy() == 0.7
    assert s.ece() == (abs(1 - 2.0) + abs(6 - 5.25)) / 10
    cnt, conf, acc = s.reliability()
    assert cnt.tolist() == [0, 4, 6] and np.isnan(conf[0]) and np.isnan(acc[0])
    assert conf[1:].tolist() == [0.5, 0.875] and acc[1:].tolist() == [0.25, 1.0]
    assert s.as_dict() == {"nll": 0.5, "ece": 0.175, "accuracy": 0.7, "n": 10}
    assert CalibrationSums(torch.from_numpy(rec)).bins == 3  # bins from the length
    rec[1] = 1
    assert np.isnan(CalibrationSums(rec, bins).nll())
    with pytest.raises(ValueError):
        CalibrationSums(rec, 4)
    with pytest.raises(ValueError):
        record_words(65)


def test_metrics_argument_validation_without_gpu():
    """The three entry points reject bad arguments before any launch."""
    lib = _lib.lib()
    P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    words = I64(-1)
    assert lib.cnf_metrics_record_words(I32(15), ctypes.byref(words)) == 0 and words.value == 49
    assert lib.cnf_metrics_record_words(I32(64), ctypes.byref(words)) == 0 and words.value == 196
    assert lib.cnf_metrics_record_words(I32(0), ctypes.byref(words)) == -2
    assert lib.cnf_metrics_record_words(I32(65), ctypes.byref(words)) == -2
    assert lib.cnf_metrics_record_words(I32(15), None) == -1
    n = ctypes.c_size_t(7)
    assert lib.cnf_metrics_workspace_bytes(I32(10), I32(15), I64(1 << 20), ctypes.byref(n)) == 0
    assert n.value == 0
    assert lib.cnf_metrics_workspace_bytes(I32(1), I32(15), I64(8), ctypes.byref(n)) == -2
    assert lib.cnf_metrics_workspace_bytes(I32(257), I32(15), I64(8), ctypes.byref(n)) == -3
    assert lib.cnf_metrics_workspace_bytes(I32(10), I32(65), I64(8), ctypes.byref(n)) == -2
    assert lib.cnf_metrics_workspace_bytes(I32(10), I32(15), I64(-1), ctypes.byref(n)) == -4
    assert lib.cnf_metrics_workspace_bytes(I32(10), I32(15), I64((1 << 26) + 1),
                                           ctypes.byref(n)) == -4
    assert lib.cnf_metrics_workspace_bytes(I32(10), I32(15), I64(8), None) == -1

    probs = (ctypes.c_float * 32)()
    y = (ctypes.c_int64 * 4)()
    rec = (ctypes.c_int64 * 49)()
    pp, py, pr = (ctypes.addressof(a) for a in (probs, y, rec))

    def call(p=pp, lab=py, dim=10, bins=15, B=2, r=pr):
        return lib.cnf_metrics(P(p), P(lab), I32(dim), I32(bins), I64(B), P(r), P(0),
                               ctypes.c_size_t(0), P(0))
    assert call(B=-1) == -4
    assert call(B=(1 << 26) + 1) == -4
    assert call(dim=1) == -2 and call(dim=257) == -3
    assert call(bins=0) == -2 and call(bins=65) == -2
    assert call(p=0) == -1 and call(lab=0) == -1 and call(r=0) == -1
    assert call(p=pp + 2) == -6 and call(lab=py + 4) == -6 and call(r=pr + 4) == -6
    assert call(p=0, lab=0, B=0) == 0       # B == 0 is a no-op
    assert not any(rec)


def test_torch_operator_registers():
    ops = _lib.torch_ops()
    assert ops is not None, "libcnf_torch.so was not built"
    sch = str(torch.ops.cnf.metrics.default._schema)
    assert "Tensor(a!) record" in sch and "int bins" in sch


def test_calibrator_evaluate_host_path():
    """Calibrator.evaluate = predict, then utils.metrics; the flow calibrator's
    evaluate on a CPU device goes through the record and agrees."""
    import calibrators as C
    from flows.realNVP_torch import RealNvpFlow
    rs = np.random.RandomState(5)
    y = rs.randint(0, 3, size=200)
    x = rs.standard_normal((200, 3))
    x[np.arange(200), y] += 2.0
    ref = R.score(C.DummyCalibrator(x, y).predict(x), y, 15)
    got = C.DummyCalibrator(x, y).evaluate(x, y)
    assert got["n"] == 200 and abs(got["nll"] - ref["nll"]) <= 1e-12
    assert abs(got["ece"] - ref["ece"]) <= 1e-6 and abs(got["accuracy"] - ref["acc"]) <= 1e-12
    torch.manual_seed(0)
    np.random.seed(0)
    cal = C.TorchFlowCalibrator(RealNvpFlow, x, y, layers=2, hidden_size=[3, 3], epochs=2,
                                dev=torch.device("cpu"))
    ref = R.score(cal.predict(x), y, 10)
    sums = cal.evaluate_sums(x, np.eye(3)[y], bins=10)
    R.check_record_counts(sums.record, ref, 10)
    got = cal.evaluate(x, y, bins=10)
    assert got["n"] == 200 and abs(got["ece"] - ref["ece"]) <= 1e-9
    assert abs(got["nll"] - ref["nll"]) <= 1e-9 and got["accuracy"] == ref["acc"]
