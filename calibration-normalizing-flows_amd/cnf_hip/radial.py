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
owning `z0`, `a`, `b`.

Everything that does not depend on the family -- the parameter table, the
checks, the workspace, the launch frame, `score`, the autograd backward -- is
`cnf_hip.rowstack.RowStack`'s (over `cnf_hip.stack.Stack`, the base of every
stack), shared with `PlanarStack`; this module holds
the launches whose arguments are radial's own (no log-det anywhere).
"""
import ctypes
import operator

import torch

from . import _lib, rowstack
from .stack import StackFn, _ptr, upstream_grads


def workspace_bytes(dim, n_layers, B):
    return rowstack.workspace_bytes("radial", dim, n_layers, B)


def param_count(dim, n_layers):
    return rowstack.param_count("radial", dim, n_layers)


class RadialStack(rowstack.RowStack):
    """A fused stack of RadialLayers (flows/flows.py:168-193) of one width."""
    family = "radial"
    slot = "_rstack"  # where a flows.Flow keeps its stack of this class
    layer = "RadialLayer"
    layer_tensors = operator.attrgetter("z0", "a", "b")
    _ws_cache = {}

    @staticmethod
    def sizes(D):
        return D, 1, 1

    # ---------------------------------------------------------------- launches
    def run(self, x, want_all=False, want_final=True):
        """(final [B, D] or None, the 0-d fp32 zero log-det, all [L, B, D] or
        None): one cnf_radial_forward call."""
        x = self._check_input(x.detach())
        ws = self._ws(x)
        B, dev = x.shape[0], x.device
        allt = torch.empty(self.L, B, self.dim, dtype=torch.float32, device=dev) \
            if want_all else None
        fin = torch.empty_like(x) if (want_final and not want_all) else None
        self._call("forward", x, ws, _ptr(fin), _ptr(allt))
        if want_all and want_final:
            fin = allt[-1]
        # the reference's log(1.0): a 0-d fp32 tensor on the host, as the torch ops return
        return fin, torch.log(torch.tensor(1.0)), allt

    def forward_loss(self, x, y, kind=_lib.LOSS_CAL, want_outputs=False, terms_out=None):
        """(terms[3] = sums over the rows of (loss, ce, 0), z or None): one
        cnf_radial_forward_loss call."""
        x = self._check_input(x.detach())
        y = y.contiguous().to(torch.int64)
        ws = self._ws(x)
        terms = self._out_buffer(terms_out, 3, x.device, "forward_loss: terms_out")
        z = torch.empty_like(x) if want_outputs else None
        self._call("forward_loss", x, ws, _ptr(y), ctypes.c_int32(kind), _ptr(z), _ptr(terms))
        return terms, z

    def vjp(self, x, g_out, all_grads, need_dx):
        """(dx or None, flat grads) for the upstream gradient of z_all (when
        all_grads) or z_final: one cnf_radial_vjp call."""
        x = self._check_input(x.detach())
        ws = self._ws(x)
        grads = torch.empty(self.param_count(), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x) if need_dx else None
        gz, gza, _ = upstream_grads(g_out, None, all_grads, x.shape[0])
        self._call("vjp", x, ws, _ptr(gz), _ptr(gza), _ptr(grads), _ptr(dx))
        return dx, grads

    def loss_and_grads(self, x, y, kind=_lib.LOSS_CAL, grad_scale=1.0, need_dx=False,
                       grads_out=None, terms_out=None):
        """Fused forward + loss + reverse mode (cnf_radial_loss_vjp): returns
        (terms[3], flat grads, dx) with terms the sums over this batch and
        grads = grad_scale * d(sum of per-row loss)/d(params), z0, a, b per
        layer."""
        x = self._check_input(x.detach())
        y = y.contiguous().to(torch.int64)
        ws = self._ws(x)
        dev = x.device
        what = "loss_and_grads: output buffer"
        grads = self._out_buffer(grads_out, self.param_count(), dev, what)
        terms = self._out_buffer(terms_out, 3, dev, what)
        dx = torch.empty_like(x) if need_dx else None
        self._call("loss_vjp", x, ws, _ptr(y), ctypes.c_int32(kind), ctypes.c_float(grad_scale),
                   _ptr(terms), _ptr(grads), _ptr(dx))
        return terms, grads, dx

    def predict(self, x, log_priors):
        """Calibrated probabilities softmax(log(softmax(flow(x - mean x)) + 1e-7)
        - log_priors) (Calibrator.predict, calibrators.py:40-44, 330-353): one
        cnf_radial_predict call.  Returns probs [B, D]."""
        x = self._check_input(x.detach())
        lp = self._log_priors(log_priors, x.device)
        ws = self._ws(x)
        probs = torch.empty_like(x)
        self._call("predict", x, ws, _ptr(lp), _ptr(probs))
        return probs

    # -------------------------------------------------------------- autograd
    def forward_autograd(self, x, want_all):
        """Forward with gradients w.r.t. x and every parameter: backward is
        cnf_radial_vjp.  Returns (z_all or z_final, the 0-d zero log-det)."""
        out = _RadialFn.apply(self, want_all, x, *self._params)
        return out, torch.log(torch.tensor(1.0))


class _RadialFn(StackFn):
    @staticmethod
    def forward(ctx, stack, want_all, x, *params):
        fin, _, allt = stack.run(x, want_all=want_all)
        StackFn.saved(ctx, stack, want_all, x)
        return allt if want_all else fin
