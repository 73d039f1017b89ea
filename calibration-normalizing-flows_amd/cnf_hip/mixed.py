"""Host side of the native mixed row-wise path (cnf_mixed_*, include/cnf.h).

`MixedStack` binds a run of PlanarLayers, RadialLayers and AffineConstantLayers
(both parameters) of one width, in any order, to the fused kernels and has
`PlanarStack`'s surface: one launch for the forward + per-row log-det (every
layer's output optional), one for the forward + loss terms, one for the
reverse mode, one for the fused forward + loss + reverse mode, one for the
calibrator's predict and one for that predict ending in the calibration record
(`score`).  `kinds`, the host array of CNF_LAYER_* words the entry points take
after n_layers, is built once from the layer classes; the parameter table has
each layer's tensors in its own family's order (planar w, u, b; radial z0, a,
b; affine s, t), which is the state_dict order, and so has the flat gradient.

The log-det the kernels return is a row's, [B].  The shape the reference's
loop would give it (its in-place accumulation admits only some orders) is the
caller's business: flows.Flow asks `flows.mixed_logdet_shape` and reshapes.

`cnf_hip.adam.StackAdam` steps the stack's parameters in one launch from the
flat gradient `loss_and_grads` writes, and `invalidate()` is a no-op, so the
calibrator's epoch runner and its HIP-graph replay drive a MixedStack as they
drive the single-family stacks.  The layers keep owning their parameters.
"""
import ctypes

import torch

from . import _lib, rowstack
from .stack import StackFn, _ptr, _stream, _stream_key, stats, upstream_grads

KIND = {"planar": _lib.LAYER_PLANAR, "radial": _lib.LAYER_RADIAL, "affine": _lib.LAYER_AFFINE}


# per family: parameter names in ABI order, how many trailing ones are scalars,
# the dimensions of the vectors (affine: [1, D])
_SPEC = {"planar": (("w", "u", "b"), 1, 1), "radial": (("z0", "a", "b"), 2, 1),
         "affine": (("s", "t"), 0, 2)}


def _layer_class(family):
    from flows import flows
    return {"planar": flows.PlanarLayer, "radial": flows.RadialLayer,
            "affine": flows.AffineConstantLayer}[family]


def _kinds_array(kinds):
    return (ctypes.c_int32 * len(kinds))(*kinds)


def workspace_bytes(dim, kinds, B):
    n = ctypes.c_size_t()
    st = _lib.lib().cnf_mixed_workspace_bytes(ctypes.c_int32(dim), ctypes.c_int32(len(kinds)),
                                              _kinds_array(kinds), ctypes.c_int64(B),
                                              ctypes.byref(n))
    _lib.check("cnf_mixed_workspace_bytes", st)
    return n.value


def launch_plan(dim, kinds, B):
    """What a call of this shape launches (cnf_mixed_launch_plan, host only):
    a dict of rowstack.PLAN_FIELDS."""
    out = (ctypes.c_int32 * 8)()
    st = _lib.lib().cnf_mixed_launch_plan(ctypes.c_int32(dim), ctypes.c_int32(len(kinds)),
                                          _kinds_array(kinds), ctypes.c_int64(B), out)
    _lib.check("cnf_mixed_launch_plan", st)
    return dict(zip(rowstack.PLAN_FIELDS, out))


def param_count(dim, kinds):
    n = ctypes.c_int64()
    st = _lib.lib().cnf_mixed_param_count(ctypes.c_int32(dim), ctypes.c_int32(len(kinds)),
                                          _kinds_array(kinds), ctypes.byref(n))
    _lib.check("cnf_mixed_param_count", st)
    return n.value


class MixedStack(rowstack.RowStack):
    """A fused stack of PlanarLayers, RadialLayers and AffineConstantLayers of
    one width (flows/flows.py), in any order."""
    family = "mixed"
    slot = "_mstack"  # where a flows.Flow keeps its stack of this class
    squeeze_logdet = False  # the flow shapes the log-det itself (flows.mixed_logdet_shape)
    _ws_cache = {}

    @staticmethod
    def sizes(D):  # per layer kind, not per stack: see param_count
        return ()

    @staticmethod
    def layer_tensors(layer):
        """The layer's parameter tensors in its family's ABI order."""
        return rowstack.stack_class(layer._family).layer_tensors(layer)

    def __init__(self, layers):
        self.layers = list(layers)
        self.L = len(self.layers)
        self.kinds = [KIND[ly._family] for ly in self.layers]
        self._kinds = _kinds_array(self.kinds)
        self._params = [t for ly in self.layers for t in self.layer_tensors(ly)]
        self.dim = int(self._params[0].numel())
        self._own_ws = None

    @classmethod
    def compatible(cls, layers, device=None):
        """Every layer a planar, radial or affine layer that its own family's
        stack would take (an affine layer with both parameters; contiguous
        fp32 tensors on `device`), all of one width.  The checks are
        RowStack.compatible's, per layer, in one loop: this runs on every call
        of a mixed flow."""
        layers = list(layers)
        if not layers:
            return False
        dev = None if device is None else torch.device(device)
        width = None
        for ly in layers:
            spec = _SPEC.get(getattr(ly, "_family", None))
            if spec is None or not isinstance(ly, _layer_class(ly._family)):
                return False
            names, scalars, ndim = spec
            for i, name in enumerate(names):
                t = getattr(ly, name, None)
                if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous():
                    return False
                if width is None:
                    if t.dim() != ndim:
                        return False
                    width = t.numel()
                n = 1 if i >= len(names) - scalars else width
                if t.numel() != n:
                    return False
                if ndim == 2:
                    if tuple(t.shape) != (1, n):
                        return False
                elif t.dim() > 1 or (i == 0 and t.dim() != 1):
                    return False
                td = t.device
                if dev is None:
                    dev = td
                if td.type != dev.type or (dev.index is not None and td.index != dev.index):
                    return False
        return True

    def param_count(self):
        return sum(p.numel() for p in self._params)

    def launch_plan(self, B):
        return launch_plan(self.dim, self.kinds, B)

    def reserve_workspace(self, B, device):
        n = workspace_bytes(self.dim, self.kinds, B)
        self._own_ws = (torch.empty(max(n, 16), dtype=torch.uint8, device=device), int(B))

    def _ws(self, x):
        B, dev = x.shape[0], x.device
        n = workspace_bytes(self.dim, self.kinds, B)
        if self._own_ws is not None and B <= self._own_ws[1] and self._own_ws[0].device == dev:
            return self._own_ws[0], n
        return self._buffer(self._ws_cache, _stream_key(dev), n, dev), n

    def _call(self, entry, x, ws, *args):
        """One launch of cnf_mixed_<entry>: RowStack._call's frame with `kinds`
        after n_layers."""
        fn, counter = self._names[entry]
        B, dev = x.shape[0], x.device
        ws, n = ws
        ptrs = (ctypes.c_void_p * len(self._params))(*[p.data_ptr() for p in self._params])
        with torch.cuda.device(dev):
            st = getattr(_lib.lib(), fn)(
                ctypes.c_int32(self.dim), ctypes.c_int32(self.L), self._kinds, ptrs, _ptr(x),
                *args, ctypes.c_int64(B), _ptr(ws), ctypes.c_size_t(n), _stream(dev))
        _lib.check(fn, st)
        stats[counter] += 1

    # ---------------------------------------------------------------- launches
    def run(self, x, want_all=False, want_final=True):
        """(final [B, D] or None, logdet [B], all [L, B, D] or None): one
        cnf_mixed_forward call."""
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
        or None): one cnf_mixed_forward_loss call."""
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
        all_grads else z_final, the per-row log-det): one cnf_mixed_vjp call."""
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
        """Fused forward + loss + reverse mode (cnf_mixed_loss_vjp): returns
        (terms[3], flat grads, dx) with terms the sums over this batch and
        grads = grad_scale * d(sum of per-row loss)/d(params) in the
        state_dict order."""
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
        cnf_mixed_predict call.  Returns probs [B, D], or (probs, logdet [B] of
        the centred rows)."""
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
        cnf_mixed_vjp."""
        return _MixedFn.apply(self, want_all, x, *self._params)


class _MixedFn(StackFn):
    @staticmethod
    def forward(ctx, stack, want_all, x, *params):
        fin, ld, allt = stack.run(x, want_all=want_all)
        StackFn.saved(ctx, stack, want_all, x)
        return (allt if want_all else fin), ld
