"""Host side of the native radial-flow path (cnf_radial_*, include/cnf.h).

`RadialStack` binds a run of RadialLayers of one width to the fused kernels
and has `PlanarStack`'s surface: one launch for the forward (every layer's
output optional), one for the forward + loss terms, one for the reverse mode,
one for the fused forward + loss + reverse mode, one for the calibrator's
predict (`predict`, cnf_radial_predict) and one for that predict ending in the
calibration record (`score`, cnf_radial_score).  The layer's log-det is the
reference's constant log(1) = 0: no launch computes one, `run` returns the 0-d
fp32 zero the torch-op path returns, and the third loss term is 0.
`cnf_hip.adam.StackAdam` steps the stack's parameters in one launch
(cnf_adam_step_tensors) from the flat gradient `loss_and_grads` writes, and
`invalidate()` is a no-op, so the calibrator's epoch runner and its HIP-graph
replay drive a RadialStack as they drive the other stacks.  The layers keep
owning `z0`, `a`, `b`; the stack passes their device pointers on every call.
Buffers are torch allocations on the input's device and the launches go to
torch's current stream.
"""
import ctypes

import torch

from . import _lib
from .engine import _ptr, _stream, _stream_key, stats

_ws_cache = {}


def workspace_bytes(dim, n_layers, B):
    n = ctypes.c_size_t()
    st = _lib.lib().cnf_radial_workspace_bytes(ctypes.c_int32(dim), ctypes.c_int32(n_layers),
                                               ctypes.c_int64(B), ctypes.byref(n))
    _lib.check("cnf_radial_workspace_bytes", st)
    return n.value


def param_count(dim, n_layers):
    n = ctypes.c_int64()
    st = _lib.lib().cnf_radial_param_count(ctypes.c_int32(dim), ctypes.c_int32(n_layers),
                                           ctypes.byref(n))
    _lib.check("cnf_radial_param_count", st)
    return n.value


def _workspace(dim, n_layers, B, device):
    """One buffer per (device, stream), grown on demand."""
    n = workspace_bytes(dim, n_layers, B)
    key = _stream_key(device)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < n:
        buf = torch.empty(max(n, 16), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf, n


def _layer_tensors(ly):
    return [ly.z0, ly.a, ly.b]


class RadialStack:
    """A fused stack of RadialLayers (flows/flows.py:168-193) of one width."""

    def __init__(self, layers):
        self.layers = list(layers)
        self.L = len(self.layers)
        self.dim = int(self.layers[0].z0.numel())
        self._params = [t for ly in self.layers for t in _layer_tensors(ly)]
        self._own_ws = None

    @staticmethod
    def compatible(layers, device=None):
        """Every layer a RadialLayer of one width whose z0, a, b are contiguous
        fp32 tensors on `device` (default: the first z0's device)."""
        from flows.flows import RadialLayer
        layers = list(layers)
        if not layers or not all(isinstance(ly, RadialLayer) for ly in layers):
            return False
        z0 = layers[0].z0
        if not torch.is_tensor(z0) or z0.dim() != 1:
            return False
        D = z0.numel()
        dev = z0.device if device is None else torch.device(device)
        for ly in layers:
            for t, n in ((ly.z0, D), (ly.a, 1), (ly.b, 1)):
                if not torch.is_tensor(t) or t.numel() != n or t.dim() > 1:
                    return False
                if t.dtype != torch.float32 or not t.is_contiguous():
                    return False
                td = t.device
                if td.type != dev.type or (dev.index is not None and td.index != dev.index):
                    return False
        return True

    def param_tensors(self):
        """ABI order: z0, a, b per layer (the state_dict order)."""
        return self._params

    def param_count(self):
        return self.L * (self.dim + 2)

    def requires_grad(self):
        return any(p.requires_grad for p in self._params)

    def state_key(self):
        return tuple((p.data_ptr(), p._version) for p in self._params)

    def _ptrs(self):
        return (ctypes.c_void_p * (3 * self.L))(*[p.data_ptr() for p in self._params])

    def _check_input(self, x):
        if not x.is_cuda:
            raise RuntimeError("native radial path needs a ROCm device tensor")
        if x.dtype != torch.float32:
            raise TypeError("native radial path is fp32; got %s" % x.dtype)
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError("expected [B, %d] rows, got %s" % (self.dim, tuple(x.shape)))
        return x.contiguous()

    def reserve_workspace(self, B, device):
        """Hold one private workspace for batches up to B rows on `device`,
        whatever stream the calls go to (the calibrator's fit: eager epochs
        and the capturing stream of its HIP graph use the same buffer, which
        exists before the capture).  The caller keeps this stack's calls on
        one stream at a time until release_workspace()."""
        n = workspace_bytes(self.dim, self.L, B)
        self._own_ws = (torch.empty(max(n, 16), dtype=torch.uint8, device=device), int(B))

    def release_workspace(self):
        self._own_ws = None

    def _ws(self, B, dev):
        if self._own_ws is not None and B <= self._own_ws[1] and self._own_ws[0].device == dev:
            return self._own_ws[0], workspace_bytes(self.dim, self.L, B)
        return _workspace(self.dim, self.L, B, dev)

    # ---------------------------------------------------------------- launches
    def run(self, x, want_all=False, want_final=True):
        """(final [B, D] or None, the 0-d fp32 zero log-det, all [L, B, D] or
        None): one cnf_radial_forward call."""
        x = self._check_input(x.detach())
        B, dev = x.shape[0], x.device
        ws, n = self._ws(B, dev)
        allt = torch.empty(self.L, B, self.dim, dtype=torch.float32, device=dev) \
            if want_all else None
        fin = torch.empty_like(x) if (want_final and not want_all) else None
        with torch.cuda.device(dev):
            st = _lib.lib().cnf_radial_forward(
                ctypes.c_int32(self.dim), ctypes.c_int32(self.L), self._ptrs(), _ptr(x), _ptr(fin),
                _ptr(allt), ctypes.c_int64(B), _ptr(ws), ctypes.c_size_t(n), _stream(dev))
        _lib.check("cnf_radial_forward", st)
        stats["radial_forward"] += 1
        if want_all and want_final:
            fin = allt[-1]
        # the reference's log(1.0): a 0-d fp32 tensor on the host, as the torch ops return
        return fin, torch.log(torch.tensor(1.0)), allt

    def forward_loss(self, x, y, kind=_lib.LOSS_CAL, want_outputs=False, terms_out=None):
        """(terms[3] = sums over the rows of (loss, ce, 0), z or None): one
        cnf_radial_forward_loss call."""
        x = self._check_input(x.detach())
        y = y.contiguous().to(torch.int64)
        B, dev = x.shape[0], x.device
        ws, n = self._ws(B, dev)
        terms = torch.empty(3, dtype=torch.float32, device=dev) if terms_out is None else terms_out
        if terms.numel() != 3 or terms.dtype != torch.float32 or terms.device != dev \
                or not terms.is_contiguous():
            raise ValueError("forward_loss: terms_out must be contiguous fp32 [3] on %s" % dev)
        z = torch.empty_like(x) if want_outputs else None
        with torch.cuda.device(dev):
            st = _lib.lib().cnf_radial_forward_loss(
                ctypes.c_int32(self.dim), ctypes.c_int32(self.L), self._ptrs(), _ptr(x), _ptr(y),
                ctypes.c_int32(kind), _ptr(z), _ptr(terms), ctypes.c_int64(B), _ptr(ws),
                ctypes.c_size_t(n), _stream(dev))
        _lib.check("cnf_radial_forward_loss", st)
        stats["radial_forward"] += 1
        return terms, z

    def vjp(self, x, g_out, all_grads, need_dx):
        """(dx or None, flat grads) for the upstream gradient of z_all (when
        all_grads) or z_final: one cnf_radial_vjp call."""
        x = self._check_input(x.detach())
        B, dev = x.shape[0], x.device
        ws, n = self._ws(B, dev)
        grads = torch.empty(self.param_count(), dtype=torch.float32, device=dev)
        dx = torch.empty_like(x) if need_dx else None
        gz = gza = None
        if g_out is not None:
            g_out = g_out.contiguous().float()
            if all_grads:
                gza = g_out
            else:
                gz = g_out
        with torch.cuda.device(dev):
            st = _lib.lib().cnf_radial_vjp(
                ctypes.c_int32(self.dim), ctypes.c_int32(self.L), self._ptrs(), _ptr(x), _ptr(gz),
                _ptr(gza), _ptr(grads), _ptr(dx), ctypes.c_int64(B), _ptr(ws),
                ctypes.c_size_t(n), _stream(dev))
        _lib.check("cnf_radial_vjp", st)
        stats["radial_vjp"] += 1
        return dx, grads

    def loss_and_grads(self, x, y, kind=_lib.LOSS_CAL, grad_scale=1.0, need_dx=False,
                       grads_out=None, terms_out=None):
        """Fused forward + loss + reverse mode (cnf_radial_loss_vjp): returns
        (terms[3], flat grads, dx) with terms the sums over this batch and
        grads = grad_scale * d(sum of per-row loss)/d(params), z0, a, b per
        layer."""
        x = self._check_input(x.detach())
        y = y.contiguous().to(torch.int64)
        B, dev = x.shape[0], x.device
        ws, n = self._ws(B, dev)
        P = self.param_count()
        grads = torch.empty(P, dtype=torch.float32, device=dev) if grads_out is None else grads_out
        terms = torch.empty(3, dtype=torch.float32, device=dev) if terms_out is None else terms_out
        for t, k in ((grads, P), (terms, 3)):
            if t.numel() != k or not t.is_contiguous() or t.dtype != torch.float32 \
                    or t.device != dev:
                raise ValueError("loss_and_grads: output buffer must be contiguous fp32 [%d] on %s"
                                 % (k, dev))
        dx = torch.empty_like(x) if need_dx else None
        with torch.cuda.device(dev):
            st = _lib.lib().cnf_radial_loss_vjp(
                ctypes.c_int32(self.dim), ctypes.c_int32(self.L), self._ptrs(), _ptr(x), _ptr(y),
                ctypes.c_int32(kind), ctypes.c_float(grad_scale), _ptr(terms), _ptr(grads),
                _ptr(dx), ctypes.c_int64(B), _ptr(ws), ctypes.c_size_t(n), _stream(dev))
        _lib.check("cnf_radial_loss_vjp", st)
        stats["radial_loss_vjp"] += 1
        return terms, grads, dx

    def _log_priors(self, log_priors, dev):
        lp = torch.as_tensor(log_priors, dtype=torch.float32, device=dev).reshape(-1).contiguous()
        if lp.numel() != self.dim:
            raise ValueError("log_priors must have %d entries" % self.dim)
        return lp

    def predict(self, x, log_priors):
        """Calibrated probabilities softmax(log(softmax(flow(x - mean x)) + 1e-7)
        - log_priors) (Calibrator.predict, calibrators.py:40-44, 330-353): one
        cnf_radial_predict call.  Returns probs [B, D]."""
        x = self._check_input(x.detach())
        B, dev = x.shape[0], x.device
        lp = self._log_priors(log_priors, dev)
        ws, n = self._ws(B, dev)
        probs = torch.empty_like(x)
        with torch.cuda.device(dev):
            st = _lib.lib().cnf_radial_predict(
                ctypes.c_int32(self.dim), ctypes.c_int32(self.L), self._ptrs(), _ptr(x), _ptr(lp),
                _ptr(probs), ctypes.c_int64(B), _ptr(ws), ctypes.c_size_t(n), _stream(dev))
        _lib.check("cnf_radial_predict", st)
        stats["radial_predict"] += 1
        return probs

    def score(self, x, log_priors, y, bins=15, record=None):
        """ADD the calibration record (cnf_hip.metrics) of predict(x,
        log_priors) against the labels y into `record` (a zeroed int64
        [4 + 3 * bins] tensor when None) and return it: one cnf_radial_score
        call, the probabilities never stored.  The words are those of
        calibration_record(predict(x, log_priors), y, bins, record)."""
        from .metrics import score_args
        x = self._check_input(x.detach())
        B, dev = x.shape[0], x.device
        lp = self._log_priors(log_priors, dev)
        y, bins, record = score_args(x, y, bins, record)
        ws, n = self._ws(B, dev)
        with torch.cuda.device(dev):
            st = _lib.lib().cnf_radial_score(
                ctypes.c_int32(self.dim), ctypes.c_int32(self.L), self._ptrs(), _ptr(x), _ptr(lp),
                _ptr(y), ctypes.c_int32(bins), _ptr(record), ctypes.c_int64(B), _ptr(ws),
                ctypes.c_size_t(n), _stream(dev))
        _lib.check("cnf_radial_score", st)
        stats["radial_score"] += 1
        return record

    def invalidate(self):
        """Nothing is prepared between calls (every call re-derives the layer
        scalars), so there is nothing to forget; kept so callers treat every
        stack alike."""

    def split(self, flat):
        """Views of a flat gradient, one per parameter tensor."""
        out, off = [], 0
        for p in self._params:
            out.append(flat[off:off + p.numel()].view_as(p))
            off += p.numel()
        return out

    # -------------------------------------------------------------- autograd
    def forward_autograd(self, x, want_all):
        """Forward with gradients w.r.t. x and every parameter: backward is
        cnf_radial_vjp.  Returns (z_all or z_final, the 0-d zero log-det)."""
        out = _RadialFn.apply(self, want_all, x, *self._params)
        return out, torch.log(torch.tensor(1.0))


class _RadialFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, stack, want_all, x, *params):
        fin, _, allt = stack.run(x, want_all=want_all)
        ctx.stack = stack
        ctx.want_all = want_all
        ctx.key = stack.state_key()
        ctx.save_for_backward(x)
        return allt if want_all else fin

    @staticmethod
    def backward(ctx, g_out):
        (x,) = ctx.saved_tensors
        stack = ctx.stack
        if stack.state_key() != ctx.key:
            raise RuntimeError(
                "one of the variables needed for gradient computation has been modified by an "
                "inplace operation: a radial-layer parameter changed between the native forward "
                "and its backward")
        dx, flat = stack.vjp(x, g_out, all_grads=ctx.want_all, need_dx=ctx.needs_input_grad[2])
        out = [None, None, dx]
        for i, g in enumerate(stack.split(flat)):
            out.append(g if ctx.needs_input_grad[3 + i] else None)
        return tuple(out)
