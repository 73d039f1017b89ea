"""Objective and gradient sums of the scaling calibrators on the device
(cnf_scaling_loss_grad / cnf_scaling_predict, include/cnf.h): temperature and
MLR scaling (SCALE_SCALAR, t = a*x + b), vector scaling (SCALE_DIAG,
t = w.x + b) and matrix scaling (SCALE_FULL, t = x@W + b).

`ScalingObjective` holds the centred fp32 logits and the labels on the device
and owns the float64 `sums` buffer and the per-block workspace.  One call of
`sums(a, b, want_grad)` is one small H2D copy of the parameters, one native
call and one D2H copy of the words

    [0] sum_r -log(p_r[y_r] + 1e-7)      [1 .. 1+D) sum_r (p_r - onehot_r)_j
    then ga: 1 word (scalar), D (diagonal) or D*D (full, ga[i*D + j])

from which calibrators.py and utils/ops.py form the reference's own `fun` and
`jac`.  The last result is cached by the parameter bytes: SciPy asks for `fun`
and `jac` at the same point and one launch serves both.  The logits are read
as fp32; every step after that is float64 on the device.
"""
import ctypes

import numpy as np
import torch

from . import _lib, engine

SCALAR, DIAG, FULL = _lib.SCALE_SCALAR, _lib.SCALE_DIAG, _lib.SCALE_FULL
MAX_ROWS = 1 << 26

engine.stats.setdefault("scaling", 0)
engine.stats.setdefault("scaling_predict", 0)


def a_len(kind, D):
    return 1 if kind == SCALAR else D if kind == DIAG else D * D


def sums_words(kind, D):
    return 1 + D + a_len(kind, D)


def check_shape(kind, D):
    if kind not in (SCALAR, DIAG, FULL):
        raise ValueError("kind must be SCALE_SCALAR, SCALE_DIAG or SCALE_FULL")
    top = _lib.SCALE_FULL_MAX_DIM if kind == FULL else _lib.MAX_DIM
    if not 2 <= D <= top:
        raise ValueError("kind %d serves 2 <= D <= %d, got %d" % (kind, top, D))


def _params(kind, D, a, b):
    """(a, b) as one float64 host array [a | b] (b None: no bias)."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    if a.size != a_len(kind, D):
        raise ValueError("a must hold %d values" % a_len(kind, D))
    if b is None:
        if kind != SCALAR:
            raise ValueError("only the scalar kind runs without a bias")
        return a, False
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    if b.size != D:
        raise ValueError("b must hold %d values" % D)
    return np.concatenate([a, b]), True


def workspace_bytes(kind, D, B):
    n = ctypes.c_size_t()
    st = _lib.lib().cnf_scaling_workspace_bytes(ctypes.c_int32(kind), ctypes.c_int32(D),
                                                ctypes.c_int64(B), ctypes.byref(n))
    _lib.check("cnf_scaling_workspace_bytes", st)
    return n.value


def loss_grad(x, y, kind, a, b, want_grad, sums, workspace):
    """One cnf_scaling_loss_grad call on the current stream: x fp32 [B, D],
    y int64 [B], a / b / sums float64 device tensors (b None: no bias)."""
    ops = engine._ops()
    if ops is not None:
        ops.scaling_loss_grad(x, y, kind, a, b, bool(want_grad), sums, workspace)
        engine.stats["torch_ops"] += 1
    else:
        with torch.cuda.device(x.device):
            st = _lib.lib().cnf_scaling_loss_grad(
                engine._ptr(x), engine._ptr(y), ctypes.c_int32(kind), ctypes.c_int32(x.shape[1]),
                engine._ptr(a), engine._ptr(b), ctypes.c_int32(int(bool(want_grad))),
                ctypes.c_int64(x.shape[0]), engine._ptr(sums), engine._ptr(workspace),
                ctypes.c_size_t(workspace.numel() * workspace.element_size()),
                engine._stream(x.device))
        _lib.check("cnf_scaling_loss_grad", st)
    engine.stats["scaling"] += 1
    return sums


def predict(x, kind, a, b, log_priors):
    """Calibrated fp32 probabilities of the ROCm fp32 tensor x [B, D] under
    the map (kind, a, b): one cnf_scaling_predict launch.  a, b, log_priors:
    host float64 values (one H2D copy)."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 2):
        raise ValueError("x must be a [B, D] tensor on a ROCm device")
    D = x.shape[1]
    check_shape(kind, D)
    x = x.detach().to(torch.float32).contiguous()
    host, has_b = _params(kind, D, a, b)
    lp = np.asarray(log_priors, dtype=np.float64).reshape(-1)
    if lp.size != D:
        raise ValueError("log_priors must hold %d values" % D)
    dev = torch.from_numpy(np.concatenate([host, lp])).to(x.device)
    na = a_len(kind, D)
    a_d = dev[:na]
    b_d = dev[na:na + D] if has_b else None
    lp_d = dev[dev.numel() - D:]
    ops = engine._ops()
    if ops is not None:
        probs = ops.scaling_predict(x, kind, a_d, b_d, lp_d)
        engine.stats["torch_ops"] += 1
    else:
        probs = torch.empty_like(x)
        with torch.cuda.device(x.device):
            st = _lib.lib().cnf_scaling_predict(
                engine._ptr(x), ctypes.c_int32(kind), ctypes.c_int32(D), engine._ptr(a_d),
                engine._ptr(b_d), engine._ptr(lp_d), engine._ptr(probs),
                ctypes.c_int64(x.shape[0]), engine._stream(x.device))
        _lib.check("cnf_scaling_predict", st)
    engine.stats["scaling_predict"] += 1
    return probs


class ScalingObjective:
    """The sums of one (x_dev, y_dev, kind) problem; see the module docstring."""

    def __init__(self, x_dev, y_dev, kind):
        if not (torch.is_tensor(x_dev) and x_dev.is_cuda and x_dev.dtype == torch.float32
                and x_dev.dim() == 2):
            raise ValueError("x_dev must be an fp32 [B, D] tensor on a ROCm device")
        self.B, self.D = int(x_dev.shape[0]), int(x_dev.shape[1])
        check_shape(kind, self.D)
        if self.B > MAX_ROWS:
            raise ValueError("at most 2^26 rows")
        self.kind = int(kind)
        self.x = x_dev.detach().contiguous()
        self.y = torch.as_tensor(y_dev).to(device=self.x.device, dtype=torch.int64).reshape(-1)
        if self.y.shape[0] != self.B:
            raise ValueError("y must hold one label per row")
        self.words = sums_words(self.kind, self.D)
        dev = self.x.device
        self._sums = torch.zeros(self.words, dtype=torch.float64, device=dev)
        nbytes = workspace_bytes(self.kind, self.D, self.B)
        self._ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
        self._params = torch.empty(a_len(self.kind, self.D) + self.D, dtype=torch.float64,
                                   device=dev)
        self._key = None
        self._val = None
        self.calls = 0  # native calls made (cache hits excluded)

    def sums(self, a, b=None, want_grad=True):
        """Host float64 array of the sums at (a, b): `words` values with
        want_grad, else the one objective word."""
        host, has_b = _params(self.kind, self.D, a, b)
        key = (host.tobytes(), has_b)
        if self._key == key and (self._val.size > 1 or not want_grad):
            return self._val if want_grad else self._val[:1]
        na = a_len(self.kind, self.D)
        p = self._params[:host.size]
        p.copy_(torch.from_numpy(host))
        loss_grad(self.x, self.y, self.kind, p[:na], p[na:] if has_b else None, want_grad,
                  self._sums, self._ws)
        self.calls += 1
        n = self.words if want_grad else 1
        self._key, self._val = key, self._sums[:n].cpu().numpy()
        return self._val
