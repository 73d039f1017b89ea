"""Drop-in mirror of the reference's calibrators.py for the flow calibrator.

`Calibrator` (base: logit centring, one-hot targets, prior correction) and
`TorchFlowCalibrator` keep the reference's constructor, `fit` schedule, history
format and `predict` path (calibrators.py:13-44, 239-353).  When the flow built
by the factory is a stack of NvpCouplingLayers on a ROCm device, each training
step is ONE fused native launch (forward + calibrator loss + reverse mode,
cnf_loss_vjp) followed by the optimizer step, and the per-epoch evaluation is
ONE fused forward + loss launch (cnf_forward_loss); history entries stay
device tensors, as in the reference, so no step synchronises the host.
A flow made of PlanarLayers (flows._factory.PlanarFlow) runs the same schedule
on its own kernels: cnf_planar_loss_vjp into a persistent flat gradient and one
native Adam launch (cnf_adam_step_tensors) per batch, cnf_planar_forward_loss
per evaluation batch, and -- after one eager epoch -- chunks of epochs replayed
as one captured HIP graph.  An optimizer the native Adam does not reproduce
(cnf_hip.adam.supports) keeps torch's own step after each
cnf_planar_loss_vjp.  `predict` / `evaluate` / `detection_curves` of a planar
calibrator on a ROCm device are one cnf_planar_predict launch on a resident
replica, and `evaluate` copies only the 4 + 3 * bins record words to the host.
CNF_PLANAR_NATIVE=0 keeps a planar flow on torch ops throughout.
A flow made of RadialLayers (flows._factory.RadialFlow) takes the same route
on the cnf_radial_* kernels -- cnf_radial_loss_vjp, cnf_radial_forward_loss,
cnf_radial_predict, cnf_radial_score (and a flow made of AffineConstantLayers,
flows._factory.AffineConstantFlow, on the cnf_affine_* ones, its log-det one
number per batch); a radial flow's `history['log_det']` is zeros, the
layer's log-det being the reference's constant 0 -- and CNF_RADIAL_NATIVE=0
keeps it on torch ops.
Any other flow (or a CPU device) runs the reference's own torch loop.

The scaling baselines -- TempScalingCalibrator, MLRCalibrator,
VectorScalingCalibrator, MatrixScalingCalibrator (calibrators.py:57-205) --
keep the reference's constructor `(logits, target)`, attributes and SciPy
calls.  NumPy inputs fit in float64 on the host; a ROCm fp32 tensor `logits`
(labels or one-hot rows as a tensor or array) stays on the device, where every
objective / gradient evaluation is one cnf_scaling_loss_grad call
(cnf_hip/scaling.py), and `predict` of a ROCm tensor is one
cnf_scaling_predict launch that returns a ROCm fp32 tensor.

PAVCalibrator (calibrators.py:208-236) keeps the reference's constructor
`(logits, target)`: one isotonic regression per class on the class's softmax
score.  NumPy inputs fit and predict in float64 on the host with the package's
own NumPy isotonic fit (cnf_hip/pav.py: sklearn 1.7's steps restated, so no
sklearn and no `np.float`); tensors are copied to the host for the fit.
`predict` of a ROCm tensor is one cnf_pav_predict launch from the uploaded
per-class tables and returns a ROCm fp32 tensor.  (The fit itself is not on
the device yet: DESIGN.md section 7d.)

`Calibrator.score` / `score_sums` is the one scoring interface of every
calibrator.  A planar, radial or affine TorchFlowCalibrator scores in ONE fused
launch that never stores the probabilities (cnf_planar_score, cnf_radial_score,
cnf_affine_score).  DummyCalibrator (whose predict
now also runs on the device), the four scaling calibrators, PAVCalibrator and
a coupling flow score a ROCm tensor with their fused predict plus one
cnf_metrics launch; host inputs go through predict() and the record of
cnf_hip.metrics.  `evaluate` / `evaluate_sums` are unchanged.

`Calibrator.detection_curves` scores predict() in the detection view (one-vs-rest
log-likelihood ratios, empirical cross-entropy curves; cnf_hip/detection.py) in
float64 on the host.

Out of scope here: TempScaler.
"""
import numpy as np
import torch
from scipy.special import softmax
from torch import nn
from torch.utils.data import DataLoader, TensorDataset


def _onehot(target, n_classes=None):
    """utils/ops.py:42-51 (onehot_encode)."""
    target = np.asarray(target).astype(int).reshape(-1)
    n = int(target.max()) + 1 if n_classes is None else n_classes
    out = np.zeros((target.shape[0], n))
    out[np.arange(target.shape[0]), target] = 1
    return out


def _detection_curves(probs, target, priors, lims, bins):
    """EceCurveSums of a probability matrix, in float64 on the host (a tensor,
    e.g. a scaling calibrator's ROCm fp32 predict, is copied there)."""
    from cnf_hip import detection
    from utils import ops
    if torch.is_tensor(probs):
        probs = probs.detach().cpu().numpy()
    probs = np.asarray(probs, dtype=np.float64)
    D = int(probs.shape[1])
    if torch.is_tensor(target):
        target = target.detach().cpu().numpy()
    target = np.asarray(target)
    y = np.argmax(target, axis=1) if target.ndim == 2 else target.reshape(-1)
    priors = np.full(D, 1. / D) if priors is None else np.asarray(priors, dtype=np.float64)
    llr = ops.detection_log_likelihood_ratios(np.log(probs + 1e-7), priors)
    return detection.ece_curve_sums(torch.from_numpy(llr), torch.as_tensor(y.astype(np.int64)),
                                    detection.prior_axis(lims, bins))


def _on_device(a):
    return torch.is_tensor(a) and a.is_cuda


def _score_labels(target, device):
    """int64 labels [B] on `device` of `target` (labels, or one-hot rows whose
    argmax is the label), as they are: a label outside [0, D) is the record's
    business (n_invalid)."""
    if torch.is_tensor(target):
        y = target.detach()
        y = torch.argmax(y, dim=1) if y.dim() == 2 else y.reshape(-1)
    else:
        y = np.asarray(target)
        y = np.argmax(y, axis=1) if y.ndim == 2 else y.reshape(-1)
        y = torch.as_tensor(y.astype(np.int64))
    return y.to(device=device, dtype=torch.int64)


class Calibrator:
    """Abstract calibrator (calibrators.py:13-44)."""

    def __init__(self, logits, target):
        logits = logits - np.mean(logits, axis=1, keepdims=True)
        self.logits = logits
        if target.shape != logits.shape:
            target = _onehot(target, logits.shape[1])
        self.target = target
        (_, self.n_classes) = target.shape
        self.log_priors = self._get_log_priors(target)

    def __call__(self, logits):
        return self.predict(logits)

    def _get_log_priors(self, target):
        priors = np.sum(target, axis=0)
        priors = priors / np.sum(priors)
        return np.log(priors)

    def predict_post(self, logits):
        raise NotImplementedError

    def predict(self, logits):
        logits = logits - np.mean(logits, axis=1, keepdims=True)
        probs = self.predict_post(logits)
        return softmax(np.log(probs + 1e-7) - self.log_priors, axis=1)

    def evaluate(self, logits, target, bins=15):
        """Score the calibrated predictions of `logits` against `target`
        (labels or one-hot rows): {"nll", "ece", "accuracy", "n"} as
        utils.metrics computes them on predict()'s float64 probabilities."""
        from utils import metrics as M
        probs = self.predict(logits)
        target = np.asarray(target)
        return {"nll": M.neg_log_likelihood(probs, target),
                "ece": M.expected_calibration_error(probs, target, bins=bins),
                "accuracy": M.accuracy(probs, target), "n": int(probs.shape[0])}

    def score_sums(self, logits, target, bins=15, record=None):
        """The calibration record of predict(logits) against `target` (labels
        or one-hot rows) as cnf_hip.metrics.CalibrationSums; `record` (an int64
        tensor on the scoring device) accumulates over calls.  A ROCm tensor
        stays on the device: predict, then one cnf_metrics launch -- or, where
        a subclass has a fused score kernel, that ONE launch, which leaves the
        same words without storing the probabilities.  Host inputs are scored
        from predict()'s float64 probabilities."""
        from cnf_hip.metrics import CalibrationSums, calibration_record
        if torch.is_tensor(logits) and not logits.is_cuda:
            logits = logits.detach().numpy()
        probs = self.predict(logits)
        if not torch.is_tensor(probs):
            probs = torch.as_tensor(np.asarray(probs))
        y = _score_labels(target, probs.device)
        return CalibrationSums(calibration_record(probs, y, bins, record), bins)

    def score(self, logits, target, bins=15):
        """{"nll", "ece", "accuracy", "n"} of predict(logits) against `target`:
        score_sums for a ROCm tensor (only the 4 + 3 * bins record words reach
        the host), evaluate()'s float64 host path for anything else."""
        if _on_device(logits):
            return self.score_sums(logits, target, bins).as_dict()
        if torch.is_tensor(logits):
            logits = logits.detach().numpy()
        if torch.is_tensor(target):
            target = target.detach().cpu().numpy()
        return self.evaluate(logits, target, bins)

    def detection_curves(self, logits, target, priors=None, lims=(-2.5, 2.5), bins=100):
        """The detection view of predict(logits) against `target` (labels or
        one-hot rows) as cnf_hip.detection.EceCurveSums: the notebooks' steps
        log(p + 1e-7), detection_log_likelihood_ratios with `priors` (uniform
        1 / D by default) and the empirical cross-entropy curves of every
        class over np.linspace(lims, num=bins) prior log10-odds.  The steps
        after predict run in float64 on the host."""
        return _detection_curves(self.predict(logits), target, priors, lims, bins)


class DummyCalibrator(Calibrator):
    """Uncalibrated model (calibrators.py:47-53)."""

    def predict_post(self, logits):
        return softmax(logits, axis=1)

    def predict(self, logits):
        """A ROCm tensor stays on the device: the scalar scaling kind with
        a = 1 and no bias is softmax of the centred logits followed by the
        prior correction (one cnf_scaling_predict launch, fp32 result)."""
        if _on_device(logits):
            from cnf_hip import scaling
            return scaling.predict(logits, scaling.SCALAR, [1.0], None, self.log_priors)
        return super().predict(logits)


class _ScalingCalibrator(Calibrator):
    """Shared by the four scaling calibrators: the host / device convention
    (module docstring), and `fun` / `jac` formed from the raw sums
    [loss | gb | ga] of utils.ops.scaling_sums_fn exactly as the reference
    forms them."""

    kind = None

    def __init__(self, logits, target):
        from utils import ops
        if ops._is_device(logits):
            labels = ops.hard_labels(target, logits.shape)
            if labels is None or logits.dtype != torch.float32:  # soft targets: host path
                logits = logits.detach().cpu().numpy().astype(np.float64)
                target = target.detach().cpu().numpy() if torch.is_tensor(target) else target
        if ops._is_device(logits):
            # centred once, in float64, and rounded back to the fp32 the kernels read
            x = logits.detach().double()
            self.logits = (x - x.mean(dim=1, keepdim=True)).float()
            self.n_classes = int(logits.shape[1])
            if labels.size and (labels.min() < 0 or labels.max() >= self.n_classes):
                raise ValueError("labels must lie in [0, %d)" % self.n_classes)
            self.target = torch.from_numpy(labels).to(logits.device)
            priors = np.bincount(labels, minlength=self.n_classes).astype(np.float64)
            with np.errstate(divide="ignore"):
                self.log_priors = np.log(priors / np.sum(priors))
        else:
            super().__init__(np.asarray(logits), np.asarray(target))
        self._setup()
        self.fit(self.logits, self.target)

    def _setup(self):
        pass

    def _map(self):
        """(a, b) of the fitted map t = A(x) + b, as cnf_scaling_predict takes them."""
        raise NotImplementedError

    def predict(self, logits):
        from utils import ops
        if ops._is_device(logits):
            from cnf_hip import scaling
            a, b = self._map()
            return scaling.predict(logits, self.kind, a, b, self.log_priors)
        if torch.is_tensor(logits):
            logits = logits.detach().numpy()
        return super().predict(np.asarray(logits, dtype=np.float64))


class TempScalingCalibrator(_ScalingCalibrator):
    """softmax(logits / T), T from utils.ops.optim_temperature's Newton-CG run
    (calibrators.py:57-68).  Quirk kept: the objective carries the 1e-7, the
    gradient -mean(sum((p - t) * x)) / T^2 does not."""

    kind = 0

    def fit(self, logits, target):
        from utils import ops
        self.T, self.optim = ops._optim_temperature(logits, target)

    def _map(self):
        return [1. / self.T], None

    def predict_post(self, logits):
        return softmax(logits / self.T, axis=1)


class MatrixScalingCalibrator(_ScalingCalibrator):
    """softmax(logits @ W + b), SciPy CG from zeros (calibrators.py:71-116).
    Quirk kept: the objective evaluates logits @ (W + b), b broadcast over W's
    rows, while the gradient is that of logits @ W + b, so the line search
    usually ends with "precision loss", as the reference's does."""

    kind = 2

    def _setup(self):
        self.n = self.n_classes
        self.W = np.zeros([self.n, self.n])
        self.b = np.zeros(self.n)

    def fit(self, logits, target):
        from scipy.optimize import minimize
        from utils import ops
        n = self.n
        sums, B, _ = ops.scaling_sums_fn(logits, target, self.kind)
        zero = np.zeros(n)

        def fun(x):
            return sums((x[n:].reshape(n, n) + x[:n]).ravel(), zero, False)[0] / B

        def jac(x):
            s = sums(x[n:], x[:n], True)
            return np.concatenate([s[1:1 + n], s[1 + n:]]) / B

        self._fun, self._jac = fun, jac
        x0 = np.concatenate((self.b, self.W.ravel()))
        self.optim = minimize(fun, x0=x0, method='CG', jac=jac)
        self.b = self.optim.x[:n]
        self.W = self.optim.x[n:].reshape([n, n])

    def _map(self):
        return self.W.ravel(), self.b

    def predict_post(self, logits):
        return softmax(logits @ self.W + self.b, axis=1)


class VectorScalingCalibrator(_ScalingCalibrator):
    """softmax(W * logits + b), SciPy CG from zeros (calibrators.py:119-161).
    Quirk kept: the bias gradient is the one scalar mean(p - t) over all
    elements, broadcast to every class, so b never leaves rounding noise."""

    kind = 1

    def _setup(self):
        self.n = self.n_classes
        self.W = np.zeros(self.n)
        self.b = np.zeros(self.n)

    def fit(self, logits, target):
        from scipy.optimize import minimize
        from utils import ops
        n = self.n
        sums, B, _ = ops.scaling_sums_fn(logits, target, self.kind)

        def fun(x):
            return sums(x[n:], x[:n], True)[0] / B

        def jac(x):
            s = sums(x[n:], x[:n], True)
            grad = np.zeros(x.shape)
            grad[:n] = np.sum(s[1:1 + n]) / (B * n)
            grad[n:] = s[1 + n:] / B
            return grad

        self._fun, self._jac = fun, jac
        x0 = np.concatenate((self.b, self.W))
        self.optim = minimize(fun, x0=x0, method='CG', jac=jac)
        self.b = self.optim.x[:n]
        self.W = self.optim.x[n:]

    def _map(self):
        return self.W, self.b

    def predict_post(self, logits):
        return softmax(self.W * logits + self.b, axis=1)


class MLRCalibrator(_ScalingCalibrator):
    """softmax(alpha * logits + gamma), SciPy CG from (1, 0) (calibrators.py:164-205)."""

    kind = 0

    def _setup(self):
        self.alpha = 1.
        self.gamma = np.zeros(self.n_classes)

    def fit(self, logits, target):
        from scipy.optimize import minimize
        from utils import ops
        sums, B, D = ops.scaling_sums_fn(logits, target, self.kind)

        def fun(x):
            return sums(x[:1], x[1:], True)[0] / B

        def jac(x):
            s = sums(x[:1], x[1:], True)
            return np.concatenate([s[1 + D:], s[1:1 + D]]) / B

        self._fun, self._jac = fun, jac
        x0 = np.concatenate(([self.alpha], self.gamma))
        self.optim = minimize(fun, x0=x0, method='CG', jac=jac)
        self.alpha = self.optim.x[0]
        self.gamma = self.optim.x[1:]

    def _map(self):
        return [self.alpha], self.gamma

    def predict_post(self, logits):
        return softmax(self.alpha * logits + self.gamma, axis=1)


class PAVCalibrator(Calibrator):
    """One isotonic regression (y_min=0, y_max=1, out_of_bounds='clip') per
    class, one-vs-rest, on softmax(centred logits)[:, c] (calibrators.py:
    208-236).  `models` holds each class's fitted points as host arrays
    (X_thresholds_, y_thresholds_).  The fit is the package's NumPy isotonic
    fit in float64 on the host (tensor inputs, ROCm ones included, are copied
    there); `predict` of a ROCm tensor runs on the device."""

    def __init__(self, logits, target):
        if torch.is_tensor(logits):
            logits = logits.detach().cpu().numpy()
        if torch.is_tensor(target):
            target = target.detach().cpu().numpy()
        logits, target = np.asarray(logits, dtype=np.float64), np.asarray(target)
        if target.shape != logits.shape:
            labels = target.astype(int).reshape(-1)
            if labels.size and (labels.min() < 0 or labels.max() >= logits.shape[1]):
                raise ValueError("labels must lie in [0, %d)" % logits.shape[1])
        with np.errstate(divide="ignore"):
            super().__init__(logits, target)
        self._model = None
        self.fit(self.logits, self.target)

    def fit(self, logits, target):
        from cnf_hip import pav
        self._model = None
        self.models = pav.host_fit(softmax(logits, axis=1).astype(np.float64), np.asarray(target))

    def _device_model(self, device):
        from cnf_hip import pav
        if self._model is None or self._model.thr_x.device != device:
            self._model = pav.PavModel.from_host(self.models, device)
        return self._model

    def predict(self, logits):
        from utils import ops
        if ops._is_device(logits):
            from cnf_hip import pav
            return pav.predict(logits, self._device_model(logits.device), self.log_priors)
        if torch.is_tensor(logits):
            logits = logits.detach().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            return super().predict(np.asarray(logits, dtype=np.float64))

    def predict_post(self, logits):
        from cnf_hip import pav
        return pav.host_predict(self.models, softmax(logits, axis=1).astype(np.float64))


def _native_stack(flow, dev, need_vjp=True):
    """The fused CouplingStack behind `flow`, or None when the flow is not a
    stack of NvpCouplingLayers or the device is not a ROCm GPU (need_vjp: the
    shape must also have a native reverse mode)."""
    if torch.device(dev).type != "cuda":
        return None
    try:
        from flows.flows import Flow, NvpCouplingLayer
        import cnf_hip  # noqa: F401
    except ImportError:
        return None
    if not isinstance(flow, Flow) or not all(isinstance(l, NvpCouplingLayer) for l in flow.layers):
        return None
    if flow._strict():
        return None
    stack = flow._native_stack()
    if not need_vjp:
        return stack
    try:
        return stack if stack.has_native_vjp() else None
    except Exception:  # no library to ask
        return None


def _tensor_stack(flow, dev):
    """The fused PlanarStack, RadialStack, AffineStack or MixedStack behind `flow`
    (the stacks without a cnf_desc, whose parameters StackAdam steps as a tensor
    list), or None when the flow is not an all-planar, all-radial, all-affine or
    mixed planar/radial/affine Flow with fp32 parameters on the ROCm device `dev` (an affine layer needs
    both of its parameters), the shape is outside the kernels' envelope, or the
    family's switch (CNF_PLANAR_NATIVE=0 / CNF_RADIAL_NATIVE=0 /
    CNF_AFFINE_NATIVE=0) is off."""
    if torch.device(dev).type != "cuda":
        return None
    try:
        from flows import flows as F
        from cnf_hip import _lib
        from cnf_hip.rowstack import stack_class
    except ImportError:
        return None
    for family, native, layer, max_layers in (
            ("planar", F.PLANAR_NATIVE, F.PlanarLayer, _lib.PLANAR_MAX_LAYERS),
            ("radial", F.RADIAL_NATIVE, F.RadialLayer, _lib.RADIAL_MAX_LAYERS),
            ("affine", F.AFFINE_NATIVE, F.AffineConstantLayer, _lib.AFFINE_MAX_LAYERS)):
        if not native or not isinstance(flow, F.Flow):
            continue
        layers = list(flow.layers)
        if not layers or not all(isinstance(l, layer) for l in layers):
            continue
        cls = stack_class(family)
        ps = [p for l in layers for p in cls.layer_tensors(l)]
        if not all(isinstance(p, nn.Parameter) and p.is_cuda for p in ps):
            continue
        if not cls.compatible(layers, ps[0].device):
            continue
        if not (1 <= ps[0].numel() <= _lib.MAX_DIM and len(layers) <= max_layers):
            continue
        return flow._row_stack(cls, layers)
    return _mixed_stack(flow, F, _lib)


def _mixed_stack(flow, F, _lib):
    """The fused MixedStack behind a Flow that mixes planar, radial and affine
    layers of one width (parameters fp32 on the ROCm device), or None: as
    flows._mixed_class decides per call, here for any batch of two or more
    rows, which is what a fit, a predict and a score run on."""
    if not isinstance(flow, F.Flow) or not F.MIXED_NATIVE:
        return None
    layers = list(flow.layers)
    families = {getattr(l, "_family", None) for l in layers}
    switches = F._family_switches()
    if len(families) < 2 or not all(switches.get(f, False) for f in families):
        return None
    if layers[0]._family == "radial" or F.mixed_logdet_shape(layers, 2) is None:
        return None
    from cnf_hip.mixed import MixedStack
    ps = [p for l in layers for p in MixedStack.layer_tensors(l)]
    if not all(isinstance(p, nn.Parameter) and p.is_cuda for p in ps):
        return None
    if not MixedStack.compatible(layers, ps[0].device):
        return None
    if not (1 <= ps[0].numel() <= _lib.MAX_DIM and len(layers) <= _lib.MIXED_MAX_LAYERS):
        return None
    return flow._row_stack(MixedStack, layers)


def _history(terms_all, epochs, N):
    """The fit's history dict from the per-epoch (loss, ce, log-det) sums."""
    hist = terms_all[:epochs] / N
    return {'loss': list(hist[:, 0].unbind(0)), 'ce': list(hist[:, 1].unbind(0)),
            'log_det': list(hist[:, 2].unbind(0))}


def _loader_order(n):
    """The row order of one pass of DataLoader(TensorDataset(...), batch_size,
    shuffle=True) (calibrators.py:274-275) with torch's global CPU RNG in the
    same state: creating the loader iterator draws its base seed
    (torch.utils.data._BaseDataLoaderIter), then the RandomSampler draws the
    seed of a fresh CPU generator and takes randperm(n) from it.  Both draws
    are reproduced, so the global RNG advances exactly as in the reference.
    Returns a pinned int64 CPU tensor (one async H2D per pass)."""
    torch.empty((), dtype=torch.int64).random_()  # the iterator's _base_seed
    seed = int(torch.empty((), dtype=torch.int64).random_().item())
    g = torch.Generator()
    g.manual_seed(seed)
    order = torch.randperm(n, generator=g)
    return order.pin_memory() if torch.cuda.is_available() else order


class _EpochRunner:
    """One training epoch of TorchFlowCalibrator.fit on the fused kernels
    (calibrators.py:284-317): gather the pass's rows in loader order, per
    batch the stack's fused loss + reverse mode and one Adam launch, then the
    eval pass's fused forward + loss per batch, whose LAST batch's sums are the
    epoch's history terms.

    `stack` is a CouplingStack, a PlanarStack, a RadialStack or an AffineStack; the runner uses
    loss_and_grads(x, y, grad_scale=, grads_out=, terms_out=),
    forward_loss(x, y, terms_out=), reserve_workspace / release_workspace and
    invalidate() (no-ops where a stack has nothing to do).  The flat gradient
    and the terms of the batches nobody reads are persistent buffers, so a
    captured epoch allocates neither."""

    def __init__(self, stack, adam, logits, target, bs):
        self.stack, self.adam, self.x, self.y, self.bs = stack, adam, logits, target, bs
        self.N = logits.shape[0]
        self.nb = (self.N + bs - 1) // bs
        dev = logits.device
        self.flat = torch.empty(stack.param_count(), dtype=torch.float32, device=dev)
        self.step_terms = torch.empty(3, dtype=torch.float32, device=dev)
        self.eval_terms = torch.empty(3, dtype=torch.float32, device=dev)
        stack.reserve_workspace(min(bs, self.N), dev)

    def body(self, order_tr, order_ev, terms_out, sched=None):
        N, bs = self.N, self.bs
        xs, ys = self.x.index_select(0, order_tr), self.y.index_select(0, order_tr)
        for b, s in enumerate(range(0, N, bs)):
            xb, yb = xs[s:s + bs], ys[s:s + bs]
            _, grads, _ = self.stack.loss_and_grads(xb, yb, grad_scale=1.0 / xb.shape[0],
                                                    grads_out=self.flat,
                                                    terms_out=self.step_terms)
            if sched is None:
                self.adam.step(grads)
            else:
                self.adam.step_sched(grads, sched[b])
        xe, ye = self.x.index_select(0, order_ev), self.y.index_select(0, order_ev)
        for s in range(0, N, bs):
            last = s + bs >= N
            self.stack.forward_loss(xe[s:s + bs], ye[s:s + bs],
                                    terms_out=terms_out if last else self.eval_terms)

    def eager_epoch(self, terms_out):
        dev = self.x.device
        o_tr = _loader_order(self.N).to(dev, non_blocking=True)
        o_ev = _loader_order(self.N).to(dev, non_blocking=True)
        self.body(o_tr, o_ev, terms_out)


class _EpochGraph:
    """K epochs of _EpochRunner captured once as a HIP graph (torch.cuda.graph;
    every launch of the C ABI goes to the capturing stream).  Per replay the
    host draws the K epochs' loader orders (the global CPU RNG advances as the
    reference's DataLoader would) and the Adam scalars of the K * nb steps,
    stages both with ONE host-to-device copy into the graph's static buffers,
    replays, and copies the K per-epoch terms out."""

    CHUNK = 50

    def __init__(self, run, K):
        self.run, self.K = run, K
        N, nb, dev = run.N, run.nb, run.x.device
        self.ord = torch.empty(K, 2, N, dtype=torch.int64, device=dev)
        self.sched = torch.empty(K, nb, 2, dtype=torch.float32, device=dev)
        self.terms = torch.empty(K, 3, dtype=torch.float32, device=dev)
        run.stack.invalidate()  # the graph's first launch re-prepares the weights
        t0 = run.adam.t
        torch.cuda.synchronize(dev)
        self.g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.g):
            for k in range(K):
                run.body(self.ord[k, 0], self.ord[k, 1], self.terms[k], sched=self.sched[k])
        run.adam.t = t0  # capture recorded the steps; replays perform them

    def replay(self, terms_dst):
        run, K, N, nb = self.run, self.K, self.run.N, self.run.nb
        orders = torch.empty(K, 2, N, dtype=torch.int64)
        for k in range(K):
            orders[k, 0] = _loader_order(N)
            orders[k, 1] = _loader_order(N)
        t = run.adam.t
        sched = torch.tensor([run.adam.sched_values(t + 1 + i) for i in range(K * nb)],
                             dtype=torch.float32).reshape(K, nb, 2)
        self.ord.copy_(orders.pin_memory(), non_blocking=True)
        self.sched.copy_(sched.pin_memory(), non_blocking=True)
        self.g.replay()
        run.adam.t = t + K * nb
        terms_dst.copy_(self.terms)


class TorchFlowCalibrator(Calibrator):
    """Trains a normalizing flow on (logits, target) by minimising
    -mean(log(softmax(f(x))[y] + 1e-7) + log|det J_f(x)|)  (calibrators.py:239-353)."""

    def __init__(self, Flow, logits, target, **kwargs):
        super().__init__(logits, target)
        self.target = np.argmax(self.target, axis=1)
        self.logits = torch.as_tensor(self.logits, dtype=torch.float)
        self.target = torch.as_tensor(self.target, dtype=torch.long)
        self.flow = Flow(self.n_classes, **kwargs)
        self.dev = kwargs.get('dev', torch.device("cuda") if torch.cuda.is_available()
                              else torch.device("cpu"))
        self.CE = nn.CrossEntropyLoss()
        self.optimizer = torch.optim.Adam(self.flow.parameters())
        self._replica = None
        self._lp_dev = None
        # native fit: replay chunks of epochs as HIP graphs (False: eager epochs)
        self._graph_ok = bool(kwargs.get('cnf_graph', True))
        self.history = self.fit(self.logits, self.target,
                                epochs=kwargs.get('epochs', 1000),
                                batch_size=kwargs.get('batch_size', logits.shape[0]))

    # ------------------------------------------------------------------ fit
    def fit(self, logits, target, epochs, batch_size):
        logits = logits.to(self.dev)
        target = target.to(self.dev)
        self.flow.to(self.dev)
        stack, fit = _native_stack(self.flow, self.dev), self._fit_native
        if stack is None:
            stack = _tensor_stack(self.flow, self.dev)
            if stack is not None:
                from cnf_hip import adam
                if not adam.supports(self.optimizer):
                    fit = self._fit_torch_step
        if stack is not None:
            # the captured epochs launch on the CURRENT device's stream: make
            # that the calibrator's `dev`, which need not be the current GPU
            with torch.cuda.device(logits.device):
                history = fit(stack, logits, target, epochs, batch_size)
        else:
            history = self._fit_torch(logits, target, epochs, batch_size)
        self.flow.cpu()
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
        return history

    def _fit_torch(self, logits, target, epochs, batch_size):
        """The reference's loop (calibrators.py:273-317), unchanged semantics."""
        train_dl = DataLoader(TensorDataset(logits, target), batch_size=batch_size, shuffle=True)
        history = {'loss': [], 'ce': [], 'log_det': []}
        softmx = nn.Softmax(dim=1)
        for epoch in range(epochs):
            self.flow.train()
            for xb, yb in train_dl:
                pred, log_det = self.flow(xb)
                probs = softmx(pred)
                ce = torch.log(probs.gather(1, yb.view(-1, 1)) + 1e-7)
                loss = -torch.mean(ce.squeeze() + log_det)
                self.flow.zero_grad()
                loss.backward()
                self.optimizer.step()
            self.flow.eval()
            _loss = _ce = _log_det = 0
            num = 0
            with torch.no_grad():
                for xb, yb in train_dl:
                    pred, log_det = self.flow(xb)
                    probs = softmx(pred)
                    ce = torch.log(probs.gather(1, yb.view(-1, 1)) + 1e-7)
                    log_prob = ce.squeeze() + log_det
                    # the reference ASSIGNS per batch (calibrators.py:308-313): the
                    # history keeps the last batch's sums over the total count
                    _loss = -torch.mean(log_prob) * len(xb)
                    _ce = -torch.mean(ce.squeeze()) * len(xb)
                    _log_det = torch.mean(log_det) * len(xb)
                    num += len(xb)
                history['loss'].append(_loss / num)
                history['ce'].append(_ce / num)
                history['log_det'].append(_log_det / num)
        return history

    def _fit_native(self, stack, logits, target, epochs, batch_size):
        """Same schedule on the fused kernels: one cnf_loss_vjp launch plus one
        cnf_adam_step launch per training batch, one cnf_forward_loss launch per
        evaluation batch (a PlanarStack: cnf_planar_loss_vjp,
        cnf_adam_step_tensors, cnf_planar_forward_loss; a RadialStack or an
        AffineStack: the cnf_radial_* / cnf_affine_* siblings).  Each pass over the
        data draws its order exactly as
        the reference's DataLoader(shuffle=True) does (_loader_order), so
        minibatch runs see the reference's batches and the eval history keeps
        the reference's last-batch value (calibrators.py:274-317).

        After one eager epoch, chunks of epochs run as ONE captured HIP graph
        each (_EpochGraph): the chunk's orders and Adam step scalars are staged
        with one host-to-device copy, so the host issues three operations per
        chunk instead of ~10 launches per epoch.  kwargs cnf_graph=False keeps
        every epoch eager."""
        from cnf_hip.adam import StackAdam
        adam = StackAdam.like(stack, self.optimizer)
        N = logits.shape[0]
        bs = max(1, int(batch_size))
        terms_all = torch.empty(max(epochs, 1), 3, dtype=torch.float32, device=logits.device)
        run = _EpochRunner(stack, adam, logits, target, bs)
        e = 0
        if epochs > 0:  # the eager first epoch also builds every cached buffer
            run.eager_epoch(terms_all[0])
            e = 1
        if self._graph_ok and epochs - e >= 2:
            g = _EpochGraph(run, min(epochs - e, _EpochGraph.CHUNK))
            while epochs - e >= g.K:
                g.replay(terms_all[e:e + g.K])
                e += g.K
        while e < epochs:
            run.eager_epoch(terms_all[e])
            e += 1
        adam.store_into(self.optimizer)
        stack.invalidate()  # drop blobs / workspaces captured into a graph pool
        stack.release_workspace()
        return _history(terms_all, epochs, N)

    def _fit_torch_step(self, stack, logits, target, epochs, batch_size):
        """The fit of a planar, radial or affine stack under an optimizer the native
        Adam does not reproduce (cnf_hip.adam.supports is false: AdamW,
        amsgrad, ...), every epoch eager: per training batch one fused loss +
        reverse-mode launch (cnf_planar_loss_vjp / cnf_radial_loss_vjp /
        cnf_affine_loss_vjp) whose
        flat gradient is viewed into each parameter's .grad, then the torch
        optimizer's own step (its state stays torch's); per evaluation batch
        one fused forward + loss launch.  Every pass draws its order as the
        reference's DataLoader(shuffle=True) does (_loader_order), and the history keeps
        the last batch's sums over N (calibrators.py:274-317)."""
        N = logits.shape[0]
        bs = max(1, int(batch_size))
        dev = logits.device
        params = stack.param_tensors()
        flat = torch.empty(stack.param_count(), dtype=torch.float32, device=dev)
        views = stack.split(flat)
        terms_all = torch.empty(max(epochs, 1), 3, dtype=torch.float32, device=dev)
        for e in range(epochs):
            order = _loader_order(N).to(dev, non_blocking=True)
            xs, ys = logits.index_select(0, order), target.index_select(0, order)
            for s in range(0, N, bs):
                xb, yb = xs[s:s + bs], ys[s:s + bs]
                stack.loss_and_grads(xb, yb, grad_scale=1.0 / xb.shape[0], grads_out=flat)
                for p, g in zip(params, views):
                    p.grad = g
                self.optimizer.step()
            order = _loader_order(N).to(dev, non_blocking=True)
            xe, ye = logits.index_select(0, order), target.index_select(0, order)
            for s in range(0, N, bs):
                last = s + bs >= N
                stack.forward_loss(xe[s:s + bs], ye[s:s + bs],
                                   terms_out=terms_all[e] if last else None)
        for p in params:
            p.grad = None
        return _history(terms_all, epochs, N)

    # -------------------------------------------------------------- predict
    def _device_flow(self):
        """A device-resident replica of the (CPU) flow, refreshed only when a
        parameter changed -- the reference moves the flow to the device and
        back on every call (calibrators.py:335-343)."""
        import copy
        key = tuple((p.data_ptr(), p._version) for p in self.flow.parameters())
        if self._replica is None or self._replica[0] != key:
            rep = copy.deepcopy(self.flow).to(self.dev)
            rep.eval()
            self._replica = (key, rep)
        return self._replica[1]

    def _device_stack(self, logits):
        """(stack, x): the native stack of the resident replica and the logits
        as an fp32 tensor on self.dev; (None, None) when no native stack
        serves this flow there."""
        if torch.device(self.dev).type != "cuda":
            return None, None
        flow = self._device_flow()
        stack = _native_stack(flow, self.dev, need_vjp=False) or _tensor_stack(flow, self.dev)
        if stack is None:
            return None, None
        if _on_device(logits):
            x = logits.detach().to(device=self.dev, dtype=torch.float)
        else:
            x = torch.as_tensor(np.asarray(logits), dtype=torch.float).to(self.dev)
        if self._lp_dev is None:
            self._lp_dev = torch.as_tensor(self.log_priors, dtype=torch.float, device=self.dev)
        return stack, x

    def _predict_device(self, logits):
        """predict()'s fp32 probabilities as a tensor on self.dev, or None when
        no native stack serves this flow there (then predict() runs on the host)."""
        stack, x = self._device_stack(logits)
        if stack is None:
            return None
        with torch.no_grad():
            return stack.predict(x, self._lp_dev)

    def predict(self, logits):
        """Calibrator.predict (calibrators.py:40-44 with predict_post, :330-353):
        centring, the flow, softmax and the prior correction
        softmax(log(p + 1e-7) - log_priors).  On a ROCm device this is ONE fused
        launch (cnf_predict; cnf_planar_predict / cnf_radial_predict /
        cnf_affine_predict for a planar / radial / affine flow) on a
        resident replica of the flow, with one H2D copy of the logits and one
        D2H copy of the probabilities."""
        probs = self._predict_device(logits)
        if probs is not None:
            return probs.cpu().numpy().astype(np.float64)
        return super().predict(logits)

    def evaluate_sums(self, logits, target, bins=15, record=None):
        """The calibration record of predict(logits) against `target` (labels
        or one-hot rows) as cnf_hip.metrics.CalibrationSums.  On a ROCm device
        the probabilities stay there: the resident replica's fused predict,
        one cnf_metrics launch, and ONE D2H copy of the 4 + 3 * bins record
        words instead of the B * D probabilities.  `record` (int64 tensor on
        the scoring device) accumulates over calls."""
        from cnf_hip.metrics import CalibrationSums, calibration_record
        target = np.asarray(target)
        if target.ndim == 2:
            target = np.argmax(target, axis=1)
        probs = self._predict_device(logits)
        if probs is None:
            probs = torch.as_tensor(super().predict(logits))
        y = torch.as_tensor(target.astype(np.int64)).to(probs.device)
        return CalibrationSums(calibration_record(probs, y, bins, record), bins)

    def evaluate(self, logits, target, bins=15):
        """{"nll", "ece", "accuracy", "n"} of predict(logits), from evaluate_sums."""
        return self.evaluate_sums(logits, target, bins).as_dict()

    def score_sums(self, logits, target, bins=15, record=None):
        """evaluate_sums' record (logits: arrays or tensors, ROCm ones
        included).  A planar, radial or affine flow on a ROCm device scores in
        ONE cnf_planar_score / cnf_radial_score / cnf_affine_score launch on the
        resident replica; a
        coupling flow keeps
        its fused predict plus one cnf_metrics launch; without a native stack
        the host path scores predict()'s float64 probabilities."""
        from cnf_hip.metrics import CalibrationSums
        stack, x = self._device_stack(logits)
        if stack is None:
            if _on_device(logits):
                logits = logits.detach().cpu()
            if record is None or not record.is_cuda:
                return super().score_sums(logits, target, bins, record)
            # scored on the host; the caller's device record is still added to
            if record.dtype != torch.int64 or record.shape != (4 + 3 * int(bins),):
                raise ValueError("record must be an int64 [%d] tensor" % (4 + 3 * int(bins)))
            host = super().score_sums(logits, target, bins).record
            record += torch.as_tensor(host).to(record.device)
            return CalibrationSums(record, bins)
        y = _score_labels(target, x.device)
        with torch.no_grad():
            return CalibrationSums(stack.score(x, self._lp_dev, y, bins, record), bins)

    def score(self, logits, target, bins=15):
        return self.score_sums(logits, target, bins).as_dict()

    def predict_logits(self, logits):
        logits = torch.as_tensor(logits, dtype=torch.float)
        if torch.device(self.dev).type == "cuda":
            flow = self._device_flow()
            with torch.no_grad():
                preds, _ = flow(logits.to(self.dev))
            return preds.cpu().numpy()
        self.flow.to(self.dev)
        preds, _ = self.flow(logits.to(self.dev))
        return preds.cpu().detach().numpy()

    def predict_post(self, logits):
        logits = self.predict_logits(logits)
        return softmax(logits, axis=1)
