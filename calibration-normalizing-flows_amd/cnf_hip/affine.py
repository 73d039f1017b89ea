"""Host side of the native affine-constant path (cnf_affine_*, include/cnf.h).

`AffineStack` binds a run of AffineConstantLayers of one width, each with both
of its parameters, to the fused kernels and has `PlanarStack`'s surface: one
launch for the forward or the inverse (every layer's output optional), one for
the forward + loss terms, one for the reverse mode of the forward, one for the
fused forward + loss + reverse mode, one for the calibrator's predict and one
for that predict ending in the calibration record (`score`).  The stack's
log-det is ONE number per call, a [1] tensor as the reference's
`torch.sum(s, dim=1)` is, and so is its upstream gradient: it never goes
through `upstream_grads`' expansion to the rows.  The inverse has no reverse
mode.  `cnf_hip.adam.StackAdam` steps the stack's parameters in one launch from
the flat gradient `loss_and_grads` writes, and `invalidate()` is a no-op, so
the calibrator's epoch runner and its HIP-graph replay drive an AffineStack as
they drive the other stacks.  The layers keep owning `s` and `t`.

Everything that does not depend on the family is `cnf_hip.rowstack.RowStack`'s,
and so are `loss_and_grads`, `score` and `forward_autograd`; the launches here
are the four the [1] log-det makes different.
"""
import ctypes
import operator

import torch

from . import _lib, rowstack
from .stack import _ptr, upstream_grads


def workspace_bytes(dim, n_layers, B):
    return rowstack.workspace_bytes("affine", dim, n_layers, B)


def param_count(dim, n_layers):
    return rowstack.param_count("affine", dim, n_layers)


class AffineStack(rowstack.RowStack):
    """A fused stack of AffineConstantLayers (flows/flows.py:40-65) of one
    width, scale and shift both present."""
    family = "affine"
    slot = "_astack"  # where a flows.Flow keeps its stack of this class
    layer = "AffineConstantLayer"
    layer_tensors = operator.attrgetter("s", "t")
    param_dims = (2,)  # [1, D]
    entries = ("inverse",)
    has_inverse = True
    squeeze_logdet = False  # torch.sum(s, dim=1) of a [1, D] parameter: [1], never squeezed
    _ws_cache = {}

    @staticmethod
    def sizes(D):
        return D, D

    @staticmethod
    def param_shape(n):
        return 1, n  # a [D, 1] tensor would broadcast over the rows, not the columns

    # ---------------------------------------------------------------- launches
    def run(self, x, inverse=False, want_all=False, want_final=True):
        """(final [B, D] or None, logdet [1], all [L, B, D] or None): one
        cnf_affine_forward call, or one cnf_affine_inverse call (all[k]: the
        rows after undoing layer L-1-k, Flow.backward's xs)."""
        x = self._check_input(x.detach())
        ws = self._ws(x)
        B, dev = x.shape[0], x.device
        ld = torch.empty(1, dtype=torch.float32, device=dev)
        allt = torch.empty(self.L, B, self.dim, dtype=torch.float32, device=dev) \
            if want_all else None
        fin = torch.empty_like(x) if (want_final and not want_all) else None
        self._call("inverse" if inverse else "forward", x, ws, _ptr(fin), _ptr(ld), _ptr(allt))
        if B == 0:  # no launch forms the log-det of an empty batch
            ld = self._logdet_ops(inverse)
        if want_all and want_final:
            fin = allt[-1]
        return fin, ld, allt

    def _logdet_ops(self, inverse):
        ld = 0.0
        for s in (self._params[-2::-2] if inverse else self._params[0::2]):
            ld = ld + torch.sum(-s.detach() if inverse else s.detach(), dim=1)
        return ld

    def forward_loss(self, x, y, kind=_lib.LOSS_CAL, det=1.0, want_outputs=False, terms_out=None):
        """(terms[3] = (sum of the per-row loss, sum of ce, B * log-det), z or
        None, ld [1] or None): one cnf_affine_forward_loss call."""
        x = self._check_input(x.detach())
        y = y.contiguous().to(torch.int64)
        ws = self._ws(x)
        dev = x.device
        terms = self._out_buffer(terms_out, 3, dev, "forward_loss: terms_out")
        z = torch.empty_like(x) if want_outputs else None
        ld = torch.empty(1, dtype=torch.float32, device=dev) if want_outputs else None
        self._call("forward_loss", x, ws, _ptr(y), ctypes.c_int32(kind), ctypes.c_float(det),
                   _ptr(z), _ptr(ld), _ptr(terms))
        return terms, z, ld

    def vjp(self, x, g_out, g_ld, all_grads, need_dx):
        """(dx or None, flat grads) for the upstream gradients of (z_all if
        all_grads else z_final, the [1] log-det): one cnf_affine_vjp call."""
        x = self._check_input(x.detach())
        ws = self._ws(x)
        grads = torch.empty(self.param_count(), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x) if need_dx else None
        gz, gza, _ = upstream_grads(g_out, None, all_grads, x.shape[0])
        gld = None
        if g_ld is not None:  # one number: never expanded to the rows
            gld = g_ld.detach().to(device=x.device, dtype=torch.float32).reshape(-1).contiguous()
            if gld.numel() != 1:
                raise ValueError("the log-det's gradient must have one element")
        self._call("vjp", x, ws, _ptr(gz), _ptr(gza), _ptr(gld), _ptr(grads), _ptr(dx))
        if x.shape[0] == 0 and gld is not None:
            # an empty batch launches nothing (grads zeroed), yet the log-det
            # and its gradient do not depend on the rows: grad s = gld
            grads.view(self.L, 2, self.dim)[:, 0, :] += gld
        return dx, grads

    def predict(self, x, log_priors):
        """Calibrated probabilities softmax(log(softmax(flow(x - mean x)) + 1e-7)
        - log_priors) (Calibrator.predict, calibrators.py:40-44, 330-353): one
        cnf_affine_predict call.  Returns probs [B, D]."""
        x = self._check_input(x.detach())
        lp = self._log_priors(log_priors, x.device)
        ws = self._ws(x)
        probs = torch.empty_like(x)
        self._call("predict", x, ws, _ptr(lp), _ptr(probs))
        return probs
