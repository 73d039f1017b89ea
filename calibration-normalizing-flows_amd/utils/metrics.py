"""Drop-in mirror of the reference's utils/metrics.py, so that
`from utils.metrics import neg_log_likelihood, expected_calibration_error,
accuracy` (run_experiment3D.py:13) works unchanged.

NumPy inputs are scored on the host in float64 with the reference's
arithmetic (including its 1-D binary ECE branch), on NumPy 1 and 2 alike.  A
2-D torch tensor on a ROCm device is scored where it lives: one native launch
fills the integer calibration record (cnf_hip.metrics.calibration_record) and
only its 4 + 3 * bins words are copied back.  Every function returns a Python
float.
"""
import numpy as np

from .ops import onehot_encode


def _device_sums(probs, target, bins=15):
    """CalibrationSums of a 2-D ROCm tensor, or None for host inputs."""
    try:
        import torch
    except ImportError:
        return None
    if not (torch.is_tensor(probs) and probs.is_cuda and probs.dim() == 2):
        return None
    from cnf_hip.metrics import CalibrationSums, calibration_record
    target = torch.as_tensor(target).to(probs.device)
    if target.shape == probs.shape:  # one-hot targets
        target = torch.argmax(target, dim=1)
    return CalibrationSums(calibration_record(probs.to(torch.float32), target, bins), bins)


def _host(a):
    """A NumPy view of a host array or CPU tensor."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def neg_log_likelihood(probs, target):
    """mean_i(-sum_j target_ij * log(probs_ij + 1e-7)) (metrics.py:6-15)."""
    sums = _device_sums(probs, target)
    if sums is not None:
        return sums.nll()
    probs, target = _host(probs), _host(target)
    if probs.ndim < 2 or probs.shape[1] == 1:
        # binary scores: columns (1 - p, p); the reference's np.stack call
        # passes the second column as `axis` and cannot run
        probs = np.stack((1. - probs.ravel(), probs.ravel()), axis=1)
    if target.shape != probs.shape:
        target = onehot_encode(target)
    return float(np.mean(-np.sum(target * np.log(probs + 1e-7), axis=1)))


def empirical_cross_entropy(like_ratios, target, prior):
    """Empirical cross entropy of likelihood ratios at a prior (Ramos et al.,
    Entropy 2018, 20, 208; metrics.py:18-32)."""
    like_ratios, target = _host(like_ratios), _host(target)
    post_ratios = like_ratios * (prior / (1. - prior))
    n_pos = np.sum(target)
    pos = prior / n_pos * np.sum(target * np.log2(1 + 1. / post_ratios))
    neg = (1 - prior) / (target.size - n_pos) * np.sum((1 - target) * np.log2(1 + post_ratios))
    return float(pos + neg)


def empirical_cross_entropy_curve(like_ratios, target, range=(-2.5, 2.5), bins=100):
    """(logprior_axis, ece): the numbers ECE_plot computes before it draws
    (visualization.py:459-471): the axis np.linspace(range, num=bins) of prior
    log10-odds and the empirical cross entropy at each point.  2-D ratios are
    flattened and scored together against the one-hot target, as ECE_plot
    does.  A list of ratio arrays gives ECE_plot_multi's [bins, len(list)]
    matrix (visualization.py:530-541).  The reference's loop in float64 NumPy
    on the host; tensors (ROCm ones included) are copied there."""
    many = isinstance(like_ratios, (list, tuple))
    axis = np.linspace(range[0], range[1], num=bins)
    out = []
    for lr in (like_ratios if many else [like_ratios]):
        lr, t = _host(lr), _host(target)
        if lr.ndim == 2:
            if t.shape != lr.shape:
                # width of the ratios, so a class the batch never draws keeps its column
                t = (t.astype(np.int64).reshape(-1, 1) == np.arange(lr.shape[1])).astype(np.int32)
            lr, t = lr.ravel(), t.ravel()
        ece = np.zeros(axis.shape)
        for i, logprior in enumerate(axis):
            odds = 10 ** logprior
            ece[i] = empirical_cross_entropy(lr, t, odds / (1. + odds))
        out.append(ece)
    return axis, (np.stack(out, axis=1) if many else out[0])


def expected_calibration_error(probs, target, bins=15):
    """ECE of Guo et al. (arXiv:1706.04599) with equal-width confidence bins
    (low, high] (metrics.py:35-73)."""
    sums = _device_sums(probs, target, bins)
    if sums is not None:
        return sums.ece()
    probs, target = _host(probs), _host(target)
    if probs.ndim > 1:
        preds = np.argmax(probs, axis=1)
        if target.shape == probs.shape:
            target = np.argmax(target, axis=1)
        conf = probs[np.arange(probs.shape[0]), preds]
    else:
        preds = np.around(probs)
        conf = np.abs((1 - preds) - probs)
    hits = np.equal(preds, target).astype(np.float32)
    width = 1. / bins
    total = 0.
    for i in range(bins):
        sel = (i * width < conf) & (conf <= (i + 1) * width)
        n = int(np.count_nonzero(sel))
        if n:
            total += abs(np.mean(hits[sel]) - np.mean(conf[sel])) * n
    return float(total / target.size)


def accuracy(probs, target):
    """Fraction of rows whose argmax is the label (metrics.py:76-80)."""
    sums = _device_sums(probs, target)
    if sums is not None:
        return sums.accuracy()
    probs, target = _host(probs), _host(target)
    if target.shape != probs.shape:
        target = onehot_encode(target)
    return float(np.mean(np.argmax(probs, axis=1) == np.argmax(target, axis=1)))
