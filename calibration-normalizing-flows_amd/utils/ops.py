"""utils/ops.py of the reference: the helpers the metrics and the scaling
calibrators need (onehot_encode, optim_temperature)."""
import numpy as np


def onehot_encode(target):
    """One-hot rows (int32 [n, max(target) + 1]) of a label vector
    (utils/ops.py:42-51)."""
    labels = np.asarray(target).astype(np.int32).reshape(-1)
    out = np.zeros((labels.shape[0], int(labels.max()) + 1), dtype=np.int32)
    out[np.arange(labels.shape[0]), labels] = 1
    return out


def detection_log_likelihood_ratios(logits, priors):
    """One-vs-rest log-likelihood ratios [B, D] of the logits under the class
    priors (utils/ops.py:54-66):
    -log(sum_{i != cls} priors[i] / (1 - priors[cls]) * exp(x_i - x_cls)).
    The reference's double loop in float64 NumPy on the host, same summation
    order; a tensor (a ROCm one included: there is no device kernel for the
    ratios yet) is copied to the host.  Returns a float64 array."""
    if hasattr(logits, "detach"):
        logits = logits.detach().cpu().numpy()
    if hasattr(priors, "detach"):
        priors = priors.detach().cpu().numpy()
    logits = np.asarray(logits, dtype=np.float64)
    priors = np.asarray(priors, dtype=np.float64)
    D = logits.shape[1]
    acc = np.zeros(logits.shape)
    for c in range(D):  # ascending i, skipping c: the reference's order of additions
        for i in range(D):
            if i != c:
                acc[:, c] += priors[i] / (1 - priors[c]) * np.exp(logits[:, i] - logits[:, c])
    with np.errstate(divide="ignore"):
        return -np.log(acc)


# ---- scaling calibrators (calibrators.py:57-205, utils/ops.py:69-115) ----
SCALE_SCALAR, SCALE_DIAG, SCALE_FULL = 0, 1, 2   # CNF_SCALE_* of include/cnf.h


def scaling_sums_host(logits, target, kind, a, b=None, want_grad=True):
    """The raw sums of cnf_scaling_loss_grad in float64 NumPy, for hard or soft
    `target` rows [B, D]:  [sum_r -sum_j target*log(p + 1e-7) | sum_r g_rj | ga]
    with p = softmax(t), g = p - target, t = a*x + b (scalar kind), w*x + b
    (diagonal), x@W + b (full; ga[i*D + j] = sum_r x_ri g_rj)."""
    from scipy.special import softmax
    x = np.asarray(logits, dtype=np.float64)
    D = x.shape[1]
    a = np.asarray(a, dtype=np.float64)
    bias = 0. if b is None else np.asarray(b, dtype=np.float64).reshape(D)
    if kind == SCALE_SCALAR:
        t = a.reshape(()) * x + bias
    elif kind == SCALE_DIAG:
        t = a.reshape(D) * x + bias
    else:
        t = x @ a.reshape(D, D) + bias
    p = softmax(t, axis=1)
    loss = np.sum(-np.sum(target * np.log(p + 1e-7), axis=1))
    if not want_grad:
        return np.array([loss])
    g = p - target
    if kind == SCALE_SCALAR:
        ga = np.array([np.sum(np.sum(g * x, axis=1))])  # row sums first, as the reference
    elif kind == SCALE_DIAG:
        ga = np.sum(g * x, axis=0)
    else:
        ga = (x.T @ g).ravel()
    return np.concatenate([[loss], np.sum(g, axis=0), ga])


def _is_device(a):
    return hasattr(a, "is_cuda") and a.is_cuda


def hard_labels(target, shape):
    """int64 labels [B] of `target` (labels, or one-hot rows of `shape`) as a
    host array, or None when the rows are soft (not exactly one-hot)."""
    if hasattr(target, "detach"):
        target = target.detach().cpu().numpy()
    target = np.asarray(target)
    if target.shape != tuple(shape):
        return target.astype(np.int64).reshape(-1)
    if not (((target == 0) | (target == 1)).all() and (target.sum(axis=1) == 1).all()):
        return None
    return np.argmax(target, axis=1).astype(np.int64)


def scaling_sums_fn(logits, target, kind):
    """(sums(a, b, want_grad), B, D) of a problem under the host / device
    convention of utils.metrics: a ROCm fp32 tensor `logits` with hard labels
    evaluates on the device (cnf_hip.scaling.ScalingObjective); arrays, CPU
    tensors and soft targets in float64 on the host."""
    if _is_device(logits):
        import torch
        labels = hard_labels(target, logits.shape)
        if labels is not None and logits.dtype == torch.float32:
            D = logits.shape[1]
            if labels.size and (labels.min() < 0 or labels.max() >= D):
                raise ValueError("labels must lie in [0, %d)" % D)
            from cnf_hip.scaling import ScalingObjective
            obj = ScalingObjective(logits, torch.from_numpy(labels), kind)
            return obj.sums, obj.B, obj.D
    if hasattr(logits, "detach"):
        logits = logits.detach().cpu().numpy()
    if hasattr(target, "detach"):
        target = target.detach().cpu().numpy()
    x = np.asarray(logits, dtype=np.float64)
    target = np.asarray(target)
    if target.shape != x.shape:
        # width of the logits, so a class the batch never draws keeps its column
        onehot = np.zeros(x.shape)
        onehot[np.arange(x.shape[0]), target.astype(np.int64).reshape(-1)] = 1
        target = onehot

    def sums(a, b=None, want_grad=True):
        return scaling_sums_host(x, target, kind, a, b, want_grad)
    return sums, x.shape[0], x.shape[1]


def temperature_fun_jac(sums, B, D):
    """The reference's objective and gradient in T (utils/ops.py:81-90) from
    the sums at a = 1/T: the objective carries the 1e-7, the gradient
    -mean(sum((p - t) * x)) / T^2 does not."""
    def fun(T):
        T = float(np.asarray(T).reshape(-1)[0])
        return sums([1. / T], None, True)[0] / B

    def jac(T):
        T = float(np.asarray(T).reshape(-1)[0])
        return np.array([-(sums([1. / T], None, True)[1 + D] / B) / T ** 2])
    return fun, jac


def _optim_temperature(logits, target, method='newton', min_diff=1e-6, step=0.01):
    """(T, OptimizeResult or None) of optim_temperature."""
    from scipy.optimize import minimize
    sums, B, D = scaling_sums_fn(logits, target, SCALE_SCALAR)
    fun, jac = temperature_fun_jac(sums, B, D)
    T = 1.0
    if method.lower() == 'newton':
        res = minimize(fun, x0=T, method='Newton-CG', jac=jac)
        return res.x[0], res
    while True:  # the reference's fixed-step descent (utils/ops.py:100-113)
        grad = float(jac(T)[0])
        if abs(grad) < min_diff:
            break
        T -= grad * step
    return T, None


def optim_temperature(logits, target, method='newton', min_diff=1e-6, step=0.01):
    """The temperature minimising the NLL of softmax(logits / T)
    (utils/ops.py:69-115): SciPy's Newton-CG from T = 1 ('newton'), or the
    reference's fixed-step gradient descent (any other `method`).  NumPy
    inputs run in float64 on the host; a ROCm fp32 tensor `logits` (labels or
    one-hot rows as a tensor or array) keeps the data on the device, each
    evaluation one cnf_scaling_loss_grad call."""
    return _optim_temperature(logits, target, method, min_diff, step)[0]
