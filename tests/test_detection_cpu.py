"""The detection view without a GPU: utils.ops.detection_log_likelihood_ratios
and utils.metrics.empirical_cross_entropy_curve on host arrays, the torch
restatements of cnf_hip/detection.py on CPU tensors and EceCurveSums, all
against the reference's recorded outputs (tests/golden/detection/*.npz, written
by gen_golden_detection.py).  Bounds: tests/_detection_ref.py."""
import numpy as np
import pytest
import torch

import _detection_ref as R
from cnf_hip import _lib, detection
from utils import metrics as M
from utils import ops


@pytest.fixture(scope="module")
def fx():
    return {n: R.load(n) for n in R.FIXTURES}


@pytest.mark.parametrize("name", R.FIXTURES)
def test_numpy_llr_reproduces_the_reference(fx, name):
    f = fx[name]
    got = ops.detection_log_likelihood_ratios(f["x"].astype(np.float64), f["priors"])
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    got = got[:, :f["llr"].shape[1]]
    assert np.max(np.abs(got - f["llr"])) <= 1e-15
    # a CPU tensor is copied to the host
    again = ops.detection_log_likelihood_ratios(torch.from_numpy(f["x"]).double(), f["priors"])
    assert isinstance(again, np.ndarray) and (again[:, :got.shape[1]] == got).all()


@pytest.mark.parametrize("name", R.FIXTURES)
def test_torch_llr_restatement(fx, name):
    f = fx[name]
    D = f["x"].shape[1]
    got = detection.log_likelihood_ratios(torch.from_numpy(f["x"]), f["priors"])
    assert got.dtype == torch.float64 and got.device.type == "cpu"
    got = got.numpy()[:, :f["llr"].shape[1]]
    R.close(got, f["llr"], R.llr_tol(f["llr"], D))


def _sums(f):
    if "t" in f:  # d7, the binary form: positive iff y == 0
        return detection.ece_curve_sums(torch.from_numpy(f["llr"][:, 0]),
                                        torch.from_numpy(1 - f["t"]), f["axis"], n_labels=2)
    return detection.ece_curve_sums(torch.from_numpy(f["llr"]), torch.from_numpy(f["y"]),
                                    f["axis"])


@pytest.mark.parametrize("name", R.FIXTURES)
def test_torch_curve_restatement(fx, name):
    f = fx[name]
    s = _sums(f)
    assert isinstance(s, detection.EceCurveSums) and s.n_invalid == 0
    assert s.n == f["x"].shape[0] and s.cols == f["curves"].shape[0]
    R.close(s.curves(), f["curves"], R.curve_tol(f["curves"]))
    for c in range(s.cols):
        assert (np.isnan(s.curve(c)) == np.isnan(f["curves"][c])).all()
    R.close(s.flat(), f["flat"], R.curve_tol(f["flat"]))
    assert (s.log10_odds == f["axis"]).all()
    odds = np.array([10 ** v for v in f["axis"]])
    assert (s.priors == odds / (1 + odds)).all()


@pytest.mark.parametrize("name", R.MULTI)
def test_host_curve_reproduces_the_reference(fx, name):
    f = fx[name]
    ratios = np.exp(f["llr"])
    with np.errstate(invalid="ignore", divide="ignore"):
        axis, flat = M.empirical_cross_entropy_curve(ratios, f["y"])
        assert (axis == f["axis"]).all() and flat.shape == (100,)
        R.close(flat, f["flat"], R.curve_tol(f["flat"]))
        onehot = np.eye(ratios.shape[1])[f["y"]]
        _, again = M.empirical_cross_entropy_curve(ratios, onehot, range=[-2.5, 2.5], bins=100)
        assert (again == flat).all()
        # one class against its own 0/1 target, and ECE_plot_multi's matrix
        _, c0 = M.empirical_cross_entropy_curve(ratios[:, 0], (f["y"] == 0).astype(np.float64))
        R.close(c0, f["curves"][0], R.curve_tol(f["curves"][0]))
        _, multi = M.empirical_cross_entropy_curve([ratios, ratios[:, ::-1].copy()], f["y"])
    assert multi.shape == (100, 2)
    R.close(multi[:, 0], f["flat"], R.curve_tol(f["flat"]))
    _, one = M.empirical_cross_entropy_curve([ratios[:, 0]], (f["y"] == 0).astype(np.float64),
                                             bins=7)
    assert one.shape == (7, 1)


def test_ece_curve_sums_views(fx):
    f = fx["d2"]
    s = _sums(f)
    assert s.curves().shape == (10, 100) and s.flat().shape == (100,)
    assert (s.curves()[3] == s.curve(3)).all()
    # the LR = 1 line is the reference's ECE of unit ratios: a function of the prior
    t0 = (f["y"] == 0).astype(np.float64)
    want = np.array([M.empirical_cross_entropy(np.ones(t0.shape), t0, p) for p in s.priors])
    R.close(s.reference(), want, R.curve_tol(want))
    # a class that never occurs is 0 / 0 = NaN, the others are not
    s6 = _sums(fx["d6"])
    assert np.isnan(s6.curve(2)).all() and np.isfinite(s6.curve(0)).all()
    assert np.isfinite(s6.flat()).all() and s6.n_pos.tolist()[2] == 0
    # a label outside [0, n_labels): counted, and every curve is NaN
    y = f["y"].copy()
    y[5], y[9] = 10, -1
    bad = detection.ece_curve_sums(torch.from_numpy(f["llr"]), torch.from_numpy(y), f["axis"])
    assert bad.n_invalid == 2 and bad.n == 1029
    assert np.isnan(bad.curves()).all() and np.isnan(bad.flat()).all()
    # ... while the sums themselves hold the valid rows only
    keep = np.ones(1031, dtype=bool)
    keep[[5, 9]] = False
    good = detection.ece_curve_sums(torch.from_numpy(f["llr"][keep]),
                                    torch.from_numpy(f["y"][keep]), f["axis"])
    R.close(bad.sums, good.sums, 1e-13 * (1 + np.abs(good.sums)))
    assert (bad.counts[:11] == good.counts[:11]).all()


def test_torch_sums_edge_elements():
    """+-inf ratios give the terms log2(1 + 1 / post) and log2(1 + post) take
    there (0 or inf); a NaN reaches only its column's sums."""
    l, y, axis = R.edge_case()
    s = detection.ece_curve_sums(torch.from_numpy(l), torch.from_numpy(y), axis)
    R.check_edge_sums(s.sums)
    assert s.counts.tolist() == [2, 2, 2, 6, 0]


def test_empirical_cross_entropy_on_host_is_unchanged():
    lr = np.array([4.0, 0.5, 2.0, 0.25])
    tt = np.array([1, 0, 1, 0])
    want = 0.5 / 2 * np.sum(tt * np.log2(1 + 1 / lr)) + 0.5 / 2 * np.sum((1 - tt) * np.log2(1 + lr))
    assert abs(M.empirical_cross_entropy(lr, tt, 0.5) - want) <= 1e-15
    assert M.empirical_cross_entropy(torch.from_numpy(lr), torch.from_numpy(tt), 0.5) == \
        M.empirical_cross_entropy(lr, tt, 0.5)


def test_host_calibrator_detection_curves(fx):
    """Calibrator.detection_curves on the host: predict, log(p + 1e-7), the
    ratios under uniform priors, the curves -- against the same steps through
    the drop-in functions."""
    import calibrators as C
    f = fx["d2"]
    x = f["x"].astype(np.float64)
    cal = C.DummyCalibrator(x, f["y"])
    s = cal.detection_curves(x, f["y"], bins=20)
    assert s.curves().shape == (10, 20) and s.n == 1031 and s.n_invalid == 0
    llr = ops.detection_log_likelihood_ratios(np.log(cal.predict(x) + 1e-7), np.full(10, 0.1))
    _, want = M.empirical_cross_entropy_curve(np.exp(llr), f["y"], bins=20)
    R.close(s.flat(), want, R.curve_tol(want))
    _, w3 = M.empirical_cross_entropy_curve(np.exp(llr[:, 3]), (f["y"] == 3).astype(np.float64),
                                            bins=20)
    R.close(s.curve(3), w3, R.curve_tol(w3))
    assert (cal.detection_curves(x, np.eye(10)[f["y"]], bins=20).sums == s.sums).all()


def test_surface_and_refusals(fx):
    """The package surface; a ROCm tensor is refused by cnf_hip.detection (no
    device kernel serves it yet) rather than scored by eager device ops; the
    C ABI is unchanged."""
    assert callable(ops.detection_log_likelihood_ratios)
    assert callable(M.empirical_cross_entropy_curve)
    assert _lib.ABI_VERSION == 2 and not any("detect" in n or "ece" in n for n in _lib.EXPORTS)
    f = fx["d5"]
    with pytest.raises(ValueError):
        detection.log_likelihood_ratios(torch.from_numpy(f["x"]), f["priors"][:1])
    with pytest.raises(ValueError):
        detection.ece_curve_sums(torch.from_numpy(f["llr"]), torch.from_numpy(f["y"]),
                                 np.linspace(-1, 1, 129))
    with pytest.raises(ValueError):
        detection.ece_curve_sums(torch.from_numpy(f["llr"]), torch.from_numpy(f["y"][:-1]),
                                 f["axis"])
    with pytest.raises(ValueError):
        detection.ece_curve_sums(torch.from_numpy(f["llr"]), torch.from_numpy(f["y"]), f["axis"],
                                 n_labels=1)
