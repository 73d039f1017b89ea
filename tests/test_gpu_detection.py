"""The detection view with ROCm tensors in hand: it runs on the host
(DESIGN.md section 7e), so the drop-in functions and Calibrator.detection_curves
copy device values there, and cnf_hip.detection refuses a device tensor rather
than score it with eager device ops."""
import numpy as np
import pytest
import torch

import _detection_ref as R
from cnf_hip import detection
from utils import metrics as M
from utils import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_drop_in_functions_copy_device_tensors_to_the_host():
    f = R.load("d2")
    x = torch.from_numpy(f["x"]).to(DEV)
    got = ops.detection_log_likelihood_ratios(x, f["priors"])
    assert isinstance(got, np.ndarray) and np.max(np.abs(got - f["llr"])) <= 1e-15
    ratios = torch.exp(torch.from_numpy(f["llr"])).to(DEV)
    axis, flat = M.empirical_cross_entropy_curve(ratios, torch.from_numpy(f["y"]).to(DEV))
    assert (axis == f["axis"]).all()
    R.close(flat, f["flat"], R.curve_tol(f["flat"]))
    with pytest.raises(NotImplementedError):
        detection.log_likelihood_ratios(x, f["priors"])
    with pytest.raises(NotImplementedError):
        detection.ece_curve_sums(torch.from_numpy(f["llr"]).to(DEV), torch.from_numpy(f["y"]),
                                 f["axis"])


def test_scaling_calibrator_detection_curves_from_device_predict():
    """predict of ROCm logits is a ROCm fp32 tensor; detection_curves scores
    exactly those probabilities, widened, on the host."""
    import calibrators as C
    rs = np.random.RandomState(10)
    y = rs.randint(0, 10, size=500)
    x = (2 * rs.standard_normal((500, 10))).astype(np.float32)
    x[np.arange(500), y] += 3.0
    xd = torch.from_numpy(x).to(DEV)
    cal = C.TempScalingCalibrator(xd, y)
    priors = rs.dirichlet(np.full(10, 5.0))
    s = cal.detection_curves(xd, y, priors=priors)
    probs = cal.predict(xd)
    assert probs.is_cuda and probs.dtype == torch.float32
    p64 = probs.cpu().numpy().astype(np.float64)
    llr = ops.detection_log_likelihood_ratios(np.log(p64 + 1e-7), priors)
    _, want = M.empirical_cross_entropy_curve(np.exp(llr), y)
    assert s.n == 500 and s.n_invalid == 0 and s.curves().shape == (10, 100)
    R.close(s.flat(), want, R.curve_tol(want))
