"""What the host sides of the row-wise flow families share (cnf_hip/planar.py,
cnf_hip/radial.py; csrc/cnf_rowflow.h is the library's counterpart).

`RowStack` binds a run of layers of one family and one width to that family's
entry points, cnf_<family>_* (include/cnf.h).  Every launching entry point
takes (dim, n_layers, params, x, ..., B, workspace, bytes, stream); `_call`
supplies that frame, and a family's launch methods pass what goes between.  A
subclass declares

  family                "planar" / "radial": the entry-point and `stats` key prefix
  slot                  the attribute under which a flows.Flow caches its stack
  layer                 the name of its layer class in flows.flows
  layer_tensors(layer)  the layer's three parameter tensors, in ABI order
  sizes(D)              their element counts

and keeps one workspace cache (`_ws_cache`, one buffer per (device, stream)).
The layers keep owning their parameters; the stack passes their device
pointers on every call and the library re-derives the per-layer constants
inside the call, so there is no prepared state to invalidate.  Buffers are
torch allocations on the input's device and the launches go to torch's
current stream.
"""
import ctypes
import functools

import torch

from . import _lib
from .engine import _ptr, _stream, _stream_key, stats


@functools.lru_cache(maxsize=None)
def stack_class(family):
    """PlanarStack for "planar", RadialStack for "radial" (a layer's `_family`)."""
    from . import planar, radial
    return {"planar": planar.PlanarStack, "radial": radial.RadialStack}[family]


def workspace_bytes(family, dim, n_layers, B):
    fn = "cnf_%s_workspace_bytes" % family
    n = ctypes.c_size_t()
    st = getattr(_lib.lib(), fn)(ctypes.c_int32(dim), ctypes.c_int32(n_layers), ctypes.c_int64(B),
                                 ctypes.byref(n))
    _lib.check(fn, st)
    return n.value


def param_count(family, dim, n_layers):
    fn = "cnf_%s_param_count" % family
    n = ctypes.c_int64()
    st = getattr(_lib.lib(), fn)(ctypes.c_int32(dim), ctypes.c_int32(n_layers), ctypes.byref(n))
    _lib.check(fn, st)
    return n.value


class RowStack:
    def __init_subclass__(cls):
        # entry -> (entry point, `stats` key): forward_loss counts as a forward
        cls._names = {e: ("cnf_%s_%s" % (cls.family, e),
                          "%s_%s" % (cls.family, "forward" if e == "forward_loss" else e))
                      for e in ("forward", "forward_loss", "vjp", "loss_vjp", "predict", "score")}

    def __init__(self, layers):
        self.layers = list(layers)
        self.L = len(self.layers)
        self._params = [t for ly in self.layers for t in self.layer_tensors(ly)]
        self.dim = int(self._params[0].numel())
        self._own_ws = None

    @classmethod
    def compatible(cls, layers, device=None):
        """Every layer of this family's layer class and of one width, its
        parameters contiguous fp32 tensors on `device` (default: the first
        parameter's device).  PlanarLayer(params=...) holds plain tensors that
        `.to()` leaves where they are: such a stack is not compatible with a
        ROCm input."""
        from flows import flows
        layer = getattr(flows, cls.layer)
        layers = list(layers)
        if not layers or not all(isinstance(ly, layer) for ly in layers):
            return False
        tensors = cls.layer_tensors
        p0 = tensors(layers[0])[0]
        if not torch.is_tensor(p0) or p0.dim() != 1:
            return False
        sizes = cls.sizes(p0.numel())
        dev = p0.device if device is None else torch.device(device)
        for ly in layers:
            for t, n in zip(tensors(ly), sizes):
                if not torch.is_tensor(t) or t.numel() != n or t.dim() > 1:
                    return False
                if t.dtype != torch.float32 or not t.is_contiguous():
                    return False
                td = t.device
                if td.type != dev.type or (dev.index is not None and td.index != dev.index):
                    return False
        return True

    def param_tensors(self):
        """ABI order: the family's layer_tensors per layer (the state_dict order)."""
        return self._params

    def param_count(self):
        return self.L * sum(self.sizes(self.dim))

    def requires_grad(self):
        return any(p.requires_grad for p in self._params)

    def state_key(self):
        return tuple((p.data_ptr(), p._version) for p in self._params)

    def _check_input(self, x):
        if not x.is_cuda:
            raise RuntimeError("native %s path needs a ROCm device tensor" % self.family)
        if x.dtype != torch.float32:
            raise TypeError("native %s path is fp32; got %s" % (self.family, x.dtype))
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError("expected [B, %d] rows, got %s" % (self.dim, tuple(x.shape)))
        return x.contiguous()

    def _log_priors(self, log_priors, dev):
        lp = torch.as_tensor(log_priors, dtype=torch.float32, device=dev).reshape(-1).contiguous()
        if lp.numel() != self.dim:
            raise ValueError("log_priors must have %d entries" % self.dim)
        return lp

    @staticmethod
    def _out_buffer(given, n, dev, what):
        """`given`, checked, or a new fp32 [n] on dev when None."""
        if given is None:
            return torch.empty(n, dtype=torch.float32, device=dev)
        if given.numel() != n or not given.is_contiguous() or given.dtype != torch.float32 \
                or given.device != dev:
            raise ValueError("%s must be contiguous fp32 [%d] on %s" % (what, n, dev))
        return given

    def reserve_workspace(self, B, device):
        """Hold one private workspace for batches up to B rows on `device`,
        whatever stream the calls go to (the calibrator's fit: eager epochs
        and the capturing stream of its HIP graph use the same buffer, which
        exists before the capture).  The caller keeps this stack's calls on
        one stream at a time until release_workspace()."""
        n = workspace_bytes(self.family, self.dim, self.L, B)
        self._own_ws = (torch.empty(max(n, 16), dtype=torch.uint8, device=device), int(B))

    def release_workspace(self):
        self._own_ws = None

    def _ws(self, x):
        """(buffer, bytes needed) for x's rows: the reserved workspace when it
        fits, else this family's buffer for (device, stream), grown on demand.
        The first point at which a shape outside the envelope raises."""
        B, dev = x.shape[0], x.device
        n = workspace_bytes(self.family, self.dim, self.L, B)
        if self._own_ws is not None and B <= self._own_ws[1] and self._own_ws[0].device == dev:
            return self._own_ws[0], n
        key = _stream_key(dev)
        buf = self._ws_cache.get(key)
        if buf is None or buf.numel() < n:
            buf = self._ws_cache[key] = torch.empty(max(n, 16), dtype=torch.uint8, device=dev)
        return buf, n

    def _call(self, entry, x, ws, *args):
        """One launch of cnf_<family>_<entry> on x's device and torch's
        current stream there; `ws` is _ws(x)'s pair and `args` are what the
        entry point takes between x and B."""
        fn, counter = self._names[entry]
        B, dev = x.shape[0], x.device
        ws, n = ws
        ptrs = (ctypes.c_void_p * (3 * self.L))(*[p.data_ptr() for p in self._params])
        with torch.cuda.device(dev):
            st = getattr(_lib.lib(), fn)(
                ctypes.c_int32(self.dim), ctypes.c_int32(self.L), ptrs, _ptr(x), *args,
                ctypes.c_int64(B), _ptr(ws), ctypes.c_size_t(n), _stream(dev))
        _lib.check(fn, st)
        stats[counter] += 1

    def score(self, x, log_priors, y, bins=15, record=None):
        """ADD the calibration record (cnf_hip.metrics) of predict(x,
        log_priors) against the labels y into `record` (a zeroed int64
        [4 + 3 * bins] tensor when None) and return it: one cnf_<family>_score
        call, the probabilities never stored.  The words are those of
        calibration_record(predict(x, log_priors), y, bins, record)."""
        from .metrics import score_args
        x = self._check_input(x.detach())
        lp = self._log_priors(log_priors, x.device)
        y, bins, record = score_args(x, y, bins, record)
        ws = self._ws(x)
        self._call("score", x, ws, _ptr(lp), _ptr(y), ctypes.c_int32(bins), _ptr(record))
        return record

    def invalidate(self):
        """Nothing is prepared between calls (every call re-derives the layer
        constants), so there is nothing to forget; kept so callers treat every
        stack alike."""

    def split(self, flat):
        """Views of a flat gradient, one per parameter tensor."""
        out, off = [], 0
        for p in self._params:
            out.append(flat[off:off + p.numel()].view_as(p))
            off += p.numel()
        return out


class RowFn(torch.autograd.Function):
    """The autograd function of a family's forward: the subclass gives
    forward(ctx, stack, want_all, x, *params), which calls saved(); backward is
    the stack's vjp with the upstream gradients in forward's output order."""

    @staticmethod
    def saved(ctx, stack, want_all, x):
        ctx.stack = stack
        ctx.want_all = want_all
        ctx.key = stack.state_key()
        ctx.save_for_backward(x)

    @staticmethod
    def backward(ctx, *grads):
        (x,) = ctx.saved_tensors
        stack = ctx.stack
        if stack.state_key() != ctx.key:
            raise RuntimeError(
                "one of the variables needed for gradient computation has been modified by an "
                "inplace operation: a %s-layer parameter changed between the native forward "
                "and its backward" % stack.family)
        dx, flat = stack.vjp(x, *grads, all_grads=ctx.want_all, need_dx=ctx.needs_input_grad[2])
        out = [None, None, dx]
        for i, g in enumerate(stack.split(flat)):
            out.append(g if ctx.needs_input_grad[3 + i] else None)
        return tuple(out)
