"""The isotonic calibrator without a GPU: the float64 restatement
(tests/_pav_ref.py) and the host path of calibrators.PAVCalibrator against the
reference's recorded thresholds and predictions (tests/golden/pav/*.npz,
written by gen_golden_pav.py), the restatement against a fresh sklearn fit
where sklearn imports (with a sweep of the chunk count of the chunked PAV),
the binding tables, and the argument validation of cnf_pav_predict."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import _pav_ref as R
from cnf_hip import _lib

THR_TOL = 4e-16
PRED_TOL = 1e-15
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAV = ("cnf_pav_predict",)


@pytest.fixture(scope="module")
def fx():
    return {n: R.load(n) for n in R.FIXTURES}


def _close(got, want, tol):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert (np.isnan(got) == np.isnan(want)).all()
    ok = ~np.isnan(want) & (got != want)  # equal infinities agree
    assert np.max(np.abs(got[ok] - want[ok]), initial=0.0) <= tol


def _same_model(points, f):
    assert [len(px) for px, _ in points] == f["n_thr"].tolist()
    for (px, py), (rx, ry) in zip(points, f["thr"]):
        _close(px, rx, THR_TOL)
        _close(py, ry, THR_TOL)


@pytest.mark.parametrize("name", R.FIXTURES)
def test_restatement_reproduces_the_goldens(fx, name):
    f = fx[name]
    D = f["x"].shape[1]
    points = R.fit(R.scores(f["x"]), f["y"])
    _same_model(points, f)
    _close(R.log_priors(f["y"], D), f["log_priors"], 0.0)
    _close(R.predict(points, f["held"], f["log_priors"]), f["pred"], PRED_TOL)
    _close(R.predict(f["thr"], f["held"], f["log_priors"]), f["pred"], PRED_TOL)


def test_fixtures_are_what_their_names_say(fx):
    assert (fx["ties"]["x"][700:] == fx["ties"]["x"][:300]).all()
    assert fx["ties"]["min_gap"] >= 1e-8 and fx["mod"]["min_gap"] >= 1e-8
    sat = R.scores(fx["sat"]["x"])
    assert (sat < 1e-15).sum() > 100 and ((sat < 1) & (1 - sat < 1e-15)).sum() > 0
    assert not (fx["degen"]["y"] == 2).any() and np.isneginf(fx["degen"]["log_priors"][2])
    assert fx["degen"]["thr"][2][1].tolist() == [0.0, 0.0] and np.isnan(fx["degen"]["pred"]).all()
    assert fx["one"]["x"].shape == (1, 3) and fx["one"]["n_thr"].tolist() == [1, 1, 1]
    for n in R.FIXTURES:  # exactly centred rows: both sides fit on identical values
        assert (np.mean(fx[n]["x"].astype(np.float64), axis=1) == 0).all()


def _random_case(seed, B, D, scale):
    rs = np.random.RandomState(seed)
    x = (scale * rs.standard_normal((B, D))).astype(np.float32)
    y = rs.randint(0, D, size=B)
    held = (scale * rs.standard_normal((300, D))).astype(np.float32)
    return x, y, held


@pytest.mark.parametrize("seed,B,D,scale", [(1, 4096, 10, 2.0), (2, 1500, 3, 2.0), (3, 5, 3, 1.0),
                                            (4, 700, 4, 80.0), (5, 2, 2, 1.0)])
def test_restatement_against_sklearn(seed, B, D, scale):
    """A fresh sklearn fit per class; the chunked PAV gives the same blocks
    for every chunk count; the package's host fit agrees too."""
    iso = pytest.importorskip("sklearn.isotonic")
    from cnf_hip import pav
    x, y, held = _random_case(seed, B, D, scale)
    if seed == 2:
        x[1200:] = x[:300]  # exact ties
    sc, hs = R.scores(x), R.scores(held)
    base = R.fit(sc, y)
    host = pav.host_fit(sc, np.eye(D)[y])
    for c in range(D):
        m = iso.IsotonicRegression(y_min=0, y_max=1, out_of_bounds="clip")
        m.fit(sc[:, c], (y == c).astype(np.float64))
        assert len(base[c][0]) == len(m.X_thresholds_)
        _close(base[c][0], m.X_thresholds_, THR_TOL)
        _close(base[c][1], m.y_thresholds_, THR_TOL)
        _close(R.predict_class(base[c][0], base[c][1], hs[:, c]), m.predict(hs[:, c]), PRED_TOL)
        assert (host[c][0] == base[c][0]).all() and (host[c][1] == base[c][1]).all()
        _close(pav.host_predict_class(host[c][0], host[c][1], hs[:, c]), m.predict(hs[:, c]),
               PRED_TOL)
    for chunks in (2, 3, 7, 64, 1000):
        got = R.fit(sc, y, chunks=chunks)
        for c in range(D):
            assert (got[c][0] == base[c][0]).all() and (got[c][1] == base[c][1]).all()


def test_grouping_walk_needs_more_than_one_step():
    """Scores packed inside 1e-15 of each other near 0 and near 1: the run is
    one group only when it is shorter than 1e-15; the package's run-wise walk
    (binary search per step) opens the groups the plain walk opens."""
    from cnf_hip import pav
    lo = np.arange(40) * 3e-16                       # 0 .. 1.17e-14: several steps
    hi = 1.0 - np.arange(30)[::-1] * 2.0 ** -53      # within 3.3e-15 of 1
    mid = np.array([0.25, 0.25, 0.25 + 5e-16, 0.5])
    x = np.concatenate([lo, mid, hi])
    want = R.group_starts(x)
    assert (pav.group_starts(x) == want).all()
    assert 4 < (want < 40).sum() < 40 and (want >= 44).sum() > 1
    rs = np.random.RandomState(0)
    bit = rs.randint(0, 2, size=x.shape[0])
    a, b = R.fit_class(x, bit), pav.host_fit_class(x, bit)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


# degen and one were recorded with one-hot targets; labels that do not reach
# every class mean the same here (the one-hot rows are D wide either way)
@pytest.mark.parametrize("target", ["labels", "onehot"])
@pytest.mark.parametrize("name", R.FIXTURES)
def test_host_calibrator_reproduces_the_recorded_predict(fx, name, target):
    import calibrators as C
    f = fx[name]
    D = f["x"].shape[1]
    t = f["y"] if target == "labels" else np.eye(D)[f["y"]]
    cal = C.PAVCalibrator(f["x"].astype(np.float64), t)
    _same_model(cal.models, f)
    got = cal.predict(f["held"].astype(np.float64))
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    _close(got, f["pred"], PRED_TOL)
    _close(cal(f["held"].astype(np.float64)), f["pred"], PRED_TOL)


def test_host_calibrator_surface(fx):
    import calibrators as C
    assert issubclass(C.PAVCalibrator, C.Calibrator)
    assert list(inspect.signature(C.PAVCalibrator.__init__).parameters) == ["self", "logits",
                                                                           "target"]
    f = fx["mod"]
    soft = 0.9 * np.eye(4)[f["y"]] + 0.025  # soft targets: real-valued PAV on the host
    p = C.PAVCalibrator(f["x"].astype(np.float64), soft).predict(f["held"].astype(np.float64))
    assert np.isfinite(p).all() and np.max(np.abs(p.sum(axis=1) - 1)) <= 1e-12
    for px, py in C.PAVCalibrator(f["x"].astype(np.float64), soft).models:
        assert (np.diff(px) > 0).all() and (np.diff(py) >= 0).all()
        assert py.min() >= 0.025 - 1e-12 and py.max() <= 0.925 + 1e-12
    cal = C.PAVCalibrator(f["x"].astype(np.float64), f["y"])
    ev = cal.evaluate(f["held"].astype(np.float64), np.zeros(256, dtype=np.int64))
    assert set(ev) == {"nll", "ece", "accuracy", "n"} and ev["n"] == 256


def test_header_exports_and_signatures_agree():
    src = open(os.path.join(ROOT, "include", "cnf.h")).read()
    declared = set(re.findall(r"^int (cnf_pav_\w+)\(", src, re.M))
    assert declared == set(PAV)
    assert set(PAV) <= set(_lib.EXPORTS)
    lib = _lib.lib()
    for name in PAV:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes
        # one ctypes argument per declared parameter
        decl = re.search(r"^int %s\((.*?)\);" % name, src, re.M | re.S).group(1)
        assert len(fn.argtypes) == len(decl.split(",")), name
    assert _lib.ABI_VERSION == 2 and lib.cnf_abi_version() == 2


def test_argument_validation_without_gpu():
    """cnf_pav_predict refuses bad arguments before any launch."""
    lib = _lib.lib()
    P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    x = (ctypes.c_float * 64)()
    d = (ctypes.c_double * 256)(*([7.0] * 256))
    y = (ctypes.c_int64 * 8)()
    nt = (ctypes.c_int32 * 16)(*([7] * 16))
    ws = (ctypes.c_double * 1)()
    probs = (ctypes.c_float * 64)(*([7.0] * 64))
    px, pd, py, pn, pw, pp = (ctypes.addressof(v) for v in (x, d, y, nt, ws, probs))

    def pr(x=px, dim=3, B=2, tx=pd, ty=pd + 512, n=pn, cap=4, lp=pd + 1024, out=pp):
        return lib.cnf_pav_predict(P(x), I32(dim), I64(B), P(tx), P(ty), P(n), I32(cap), P(lp),
                                   P(out), P(0))
    assert pr(dim=1) == -2 and pr(dim=257) == -3
    assert pr(B=-1) == -4 and pr(B=(1 << 26) + 1) == -4
    assert pr(cap=0) == -2
    assert pr(x=0) == -1 and pr(tx=0) == -1 and pr(ty=0) == -1 and pr(n=0) == -1
    assert pr(lp=0) == -1 and pr(out=0) == -1
    assert pr(x=px + 2) == -6 and pr(tx=pd + 4) == -6 and pr(ty=pd + 516) == -6
    assert pr(n=pn + 2) == -6 and pr(lp=pd + 1028) == -6 and pr(out=pp + 2) == -6
    assert pr(x=0, out=0, B=0) == 0
    # nothing was written by any refused or empty call
    assert all(v == 7.0 for v in d) and all(v == 7 for v in nt) and all(v == 7.0 for v in probs)


def test_torch_operators_register():
    import torch
    assert _lib.torch_ops() is not None, "libcnf_torch.so was not built"
    sch = str(torch.ops.cnf.pav_predict.default._schema)
    assert "Tensor n_thr" in sch and "Tensor log_priors" in sch


def test_engine_counters_exist():
    from cnf_hip import engine, pav  # noqa: F401
    assert engine.stats["pav_predict"] >= 0
