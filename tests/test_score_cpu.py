"""The fused score entry point without a GPU (cnf_planar_score; include/cnf.h):
header, binding and library agree on the symbol, every argument error is
returned before any HIP call, and Calibrator.score / score_sums on host arrays
give evaluate()'s numbers."""
import ctypes

import numpy as np
import pytest
import torch

import _metrics_ref as MR
import _pav_ref as PV
import _scaling_ref as SR
import calibrators as C
from cnf_hip import _lib
from test_abi import header_functions

P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
OK, NULL, DESC, UNSUPPORTED, BATCH, ALIGN = 0, -1, -2, -3, -4, -6
A = 64  # an aligned, never dereferenced address


def test_symbols_agree():
    lib = _lib.lib()
    name = "cnf_planar_score"
    assert name in header_functions() and name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.cnf_abi_version() == 2


def _planar(dim=10, bins=15, B=8, y=A, record=A, x=A, L=2):
    params = (P * (3 * L))(*[A] * (3 * L))
    return _lib.lib().cnf_planar_score(I32(dim), I32(L), params, P(x), P(A), P(y), I32(bins),
                                       P(record), I64(B), P(A), ctypes.c_size_t(1 << 40), P(0))


@pytest.mark.parametrize("kw,status", [
    ({"record": 0}, NULL),
    ({"bins": 0}, DESC),
    ({"bins": 65}, DESC),
    ({"B": (1 << 26) + 1}, BATCH),
    ({"B": -1}, BATCH),
    ({"y": A + 4}, ALIGN),
    ({"record": A + 4}, ALIGN),
    ({"y": 0}, NULL),
    ({"x": 0}, NULL),
    ({"x": A + 2}, ALIGN),
    ({"dim": 1}, DESC),
    ({"dim": 257}, UNSUPPORTED),
    ({}, None),
])
def test_argument_errors_before_any_device_call(kw, status):
    """One defect per call; the pointers are never dereferenced on the host,
    so a status other than the documented one would be a HIP call (CNF_ERR_HIP
    on a machine without a GPU) or a crash."""
    if status is None:   # nothing wrong: the only case that would launch
        kw, status = {"B": 0}, OK
    assert _planar(**kw) == status


def test_empty_batch_needs_no_data_pointers():
    assert _planar(B=0, x=0, y=0) == OK
    assert _planar(B=0, record=0) == NULL


def test_planar_shape_rules_of_the_sibling():
    assert _planar(L=0) == DESC and _planar(L=65) == UNSUPPORTED


# ---- Calibrator.score on host arrays ---------------------------------------------
def _cases():
    s1 = SR.load("s1")
    x, y = s1["x"].astype(np.float64), s1["y"]
    held, yh = s1["held"].astype(np.float64), s1["y_held"]
    yield "dummy", C.DummyCalibrator(x, y), held, yh
    yield "temp", C.TempScalingCalibrator(x, y), held, yh
    pm = PV.load("mod")
    yp = np.random.RandomState(5).randint(0, 4, size=pm["held"].shape[0])
    yield "pav", C.PAVCalibrator(pm["x"].astype(np.float64), pm["y"]), \
        pm["held"].astype(np.float64), yp


@pytest.mark.parametrize("name,cal,held,y", list(_cases()), ids=lambda v: v if isinstance(v, str)
                         else "")
def test_host_score_equals_evaluate(name, cal, held, y):
    want = cal.evaluate(held, y)
    assert cal.score(held, y) == want
    assert cal.score(held, np.eye(held.shape[1])[y], bins=15) == want
    assert cal.score(torch.from_numpy(held), y) == want          # a CPU tensor
    # score_sums: the integer record of the same float64 probabilities; every
    # term is rounded to 2^-32 once (|error| <= 2^-33 per row, so per mean)
    sums = cal.score_sums(held, y)
    got = sums.as_dict()
    assert got["n"] == want["n"] == held.shape[0] and sums.n_invalid == 0
    assert got["accuracy"] == want["accuracy"]
    # (+ 1e-12: float64 sums of <= 512 terms in another order, 512 * 2^-53 * sum|t|)
    assert abs(got["nll"] - want["nll"]) <= 2.0 ** -33 + 1e-12
    # ece: evaluate() averages a bin's 0/1 hits in fp32, as the reference does
    # (the 1e-6 bar of tests/test_metrics_cpu.py); the float64 restatement of
    # the same formula is met to the fixed point
    assert abs(got["ece"] - want["ece"]) <= 1e-6
    ref = MR.score(cal.predict(held), y, 15)
    assert abs(got["ece"] - ref["ece"]) <= 2.0 ** -33 + 1e-12
    MR.check_record_counts(sums.record, ref, 15)
    # accumulation: a second call into the same record doubles it
    rec = torch.zeros(4 + 3 * 15, dtype=torch.int64)
    cal.score_sums(held, y, record=rec)
    cal.score_sums(held, y, record=rec)
    assert np.array_equal(rec.numpy(), 2 * sums.record)
    assert cal.score(held, y, bins=7) == cal.evaluate(held, y, bins=7)
