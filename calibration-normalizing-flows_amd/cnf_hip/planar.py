"""Host side of the native planar-flow path (cnf_planar_*, include/cnf.h).

`PlanarStack` binds a run of PlanarLayers of one width to the fused kernels:
one launch for the forward + log-det (every layer's output optional), one for
the forward + loss terms, one for the reverse mode, one for the fused
forward + loss + reverse mode, one for the calibrator's predict (`predict`:
centring, the stack, both softmaxes and the prior correction,
cnf_planar_predict) and one for that predict ending in the calibration record
instead of the probabilities (`score`, cnf_planar_score).
`cnf_hip.adam.StackAdam` steps the stack's parameters in one launch
(cnf_adam_step_tensors) from the flat gradient `loss_and_grads` writes, and
`invalidate()` is a no-op, so the calibrator's epoch runner and its HIP-graph
replay drive a PlanarStack as they drive a CouplingStack.  The layers keep
owning `w`, `u`, `b`; the library re-derives `u_hat` inside every call.

Everything that does not depend on the family -- the parameter table, the
checks, the workspace, the launch frame, `score`, the autograd backward -- is
`cnf_hip.rowstack.RowStack`'s (over `cnf_hip.stack.Stack`, the base of every
stack), shared with `RadialStack`; this module holds
the launches whose arguments are planar's own (the log-det and its gradient).
"""
import ctypes
import operator

import torch

from . import _lib, rowstack
from .stack import StackFn, _ptr, upstream_grads


def workspace_bytes(dim, n_layers, B):
    return rowstack.workspace_bytes("planar", dim, n_layers, B)


def param_count(dim, n_layers):
    return rowstack.param_count("planar", dim, n_layers)


class PlanarStack(rowstack.RowStack):
    """A fused stack of PlanarLayers (flows/flows.py:129-165) of one width."""
    family = "planar"
    slot = "_pstack"  # where a flows.Flow keeps its stack of this class
    layer = "PlanarLayer"
    layer_tensors = operator.attrgetter("w", "u", "b")
    _ws_cache = {}

    @staticmethod
    def sizes(D):
        return D, D, 1

    # ---------------------------------------------------------------- launches
    def run(self, x, want_all=False, want_final=True):
        """(final [B, D] or None, logdet [B], all [L, B, D] or None): one
        cnf_planar_forward call."""
        x = self._check_input(x.detach())
        ws = self._ws(x)
        B, dev = x.shape[0], x.device
        ld = torch.empty(B, dtype=torch.float32, device=dev)
        allt = torch.empty(self.L, B, self.dim, dtype=torch.float32, device=dev) \
            if want_all else None
        fin = torch.empty_like(x) if (want_final and not want_all) else None
        self._call("forward", x, ws, _ptr(fin), _ptr(ld), _ptr(allt))
        if want_all and want_final:
            fin = allt[-1]
        return fin, ld, allt

    def forward_loss(self, x, y, kind=_lib.LOSS_CAL, det=1.0, want_outputs=False, terms_out=None):
        """(terms[3] = sums over the rows of (loss, ce, log-det), z or None, ld
        or None): one cnf_planar_forward_loss call."""
        x = self._check_input(x.detach())
        y = y.contiguous().to(torch.int64)
        ws = self._ws(x)
        B, dev = x.shape[0], x.device
        terms = self._out_buffer(terms_out, 3, dev, "forward_loss: terms_out")
        z = torch.empty_like(x) if want_outputs else None
        ld = torch.empty(B, dtype=torch.float32, device=dev) if want_outputs else None
        self._call("forward_loss", x, ws, _ptr(y), ctypes.c_int32(kind), ctypes.c_float(det),
                   _ptr(z), _ptr(ld), _ptr(terms))
        return terms, z, ld

    def vjp(self, x, g_out, g_ld, all_grads, need_dx):
        """(dx or None, flat grads) for the upstream gradients of (z_all if
        all_grads else z_final, log-det): one cnf_planar_vjp call."""
        x = self._check_input(x.detach())
        ws = self._ws(x)
        B, dev = x.shape[0], x.device
        grads = torch.empty(self.param_count(), dtype=torch.float32, device=dev)
        dx = torch.empty_like(x) if need_dx else None
        gz, gza, gld = upstream_grads(g_out, g_ld, all_grads, B)
        self._call("vjp", x, ws, _ptr(gz), _ptr(gza), _ptr(gld), _ptr(grads), _ptr(dx))
        return dx, grads

    def loss_and_grads(self, x, y, kind=_lib.LOSS_CAL, det=1.0, grad_scale=1.0, need_dx=False,
                       grads_out=None, terms_out=None):
        """Fused forward + loss + reverse mode (cnf_planar_loss_vjp): returns
        (terms[3], flat grads, dx) with terms the sums over this batch and
        grads = grad_scale * d(sum of per-row loss)/d(params), w, u, b per
        layer."""
        x = self._check_input(x.detach())
        y = y.contiguous().to(torch.int64)
        ws = self._ws(x)
        dev = x.device
        what = "loss_and_grads: output buffer"
        grads = self._out_buffer(grads_out, self.param_count(), dev, what)
        terms = self._out_buffer(terms_out, 3, dev, what)
        dx = torch.empty_like(x) if need_dx else None
        self._call("loss_vjp", x, ws, _ptr(y), ctypes.c_int32(kind), ctypes.c_float(det),
                   ctypes.c_float(grad_scale), _ptr(terms), _ptr(grads), _ptr(dx))
        return terms, grads, dx

    def predict(self, x, log_priors, want_logdet=False):
        """Calibrated probabilities softmax(log(softmax(flow(x - mean x)) + 1e-7)
        - log_priors) (Calibrator.predict, calibrators.py:40-44, 330-353): one
        cnf_planar_predict call.  Returns probs [B, D], or (probs, logdet [B]
        of the centred rows)."""
        x = self._check_input(x.detach())
        B, dev = x.shape[0], x.device
        lp = self._log_priors(log_priors, dev)
        ws = self._ws(x)
        probs = torch.empty_like(x)
        ld = torch.empty(B, dtype=torch.float32, device=dev) if want_logdet else None
        self._call("predict", x, ws, _ptr(lp), _ptr(probs), _ptr(ld))
        return (probs, ld) if want_logdet else probs

    # -------------------------------------------------------------- autograd
    def forward_autograd(self, x, want_all):
        """Forward with gradients w.r.t. x and every parameter: backward is
        cnf_planar_vjp."""
        return _PlanarFn.apply(self, want_all, x, *self._params)


class _PlanarFn(StackFn):
    @staticmethod
    def forward(ctx, stack, want_all, x, *params):
        fin, ld, allt = stack.run(x, want_all=want_all)
        StackFn.saved(ctx, stack, want_all, x)
        return (allt if want_all else fin), ld
