"""What the host sides of the row-wise flow families share (cnf_hip/planar.py,
cnf_hip/radial.py, cnf_hip/affine.py, cnf_hip/mixed.py; csrc/cnf_rowflow.h is
the library's counterpart).

`RowStack` binds a run of layers of one family and one width to that family's
entry points, cnf_<family>_* (include/cnf.h).  Every launching entry point
takes (dim, n_layers, params, x, ..., B, workspace, bytes, stream), the mixed
family's with `kinds` after n_layers (`_kinds`, None elsewhere); `_call`
supplies that frame, and the launch methods pass what goes between.  The launch
methods here -- run, forward_loss, vjp, loss_and_grads, predict,
forward_autograd -- are those of a family whose log-det is a row's, [B]: planar
and mixed inherit them all, affine overrides the four its [1] log-det changes,
radial (no log-det in any signature) every one.  A subclass declares

  family                "planar" / "radial" / "affine" / "mixed": the entry-point
                        and `stats` key prefix
  slot                  the attribute under which a flows.Flow caches its stack
  layer                 the name of its layer class in flows.flows
  layer_tensors(layer)  the layer's parameter tensors, in ABI order
  sizes(D)              their element counts (as many as the layer has tensors)
  param_dims            the dimensions a parameter tensor may have (1-d vectors
                        and 0-d scalars by default; affine: 2)
  param_shape(n)        the shape a parameter of n elements must have, or None
                        for any of param_dims (affine: (1, n))
  entries               its launching entry points besides the common six
  has_inverse           whether run(x, inverse=True) exists

and keeps one workspace cache (`_ws_cache`, one buffer per (device, stream)).
The parameter table, the checks, `split` and the autograd backward are the
base's (cnf_hip/stack.py), shared with the coupling stack.
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
from .stack import Stack, StackFn, _ptr, _stream, _stream_key, stats, upstream_grads


@functools.lru_cache(maxsize=None)
def stack_class(family):
    """PlanarStack for "planar", RadialStack for "radial", AffineStack for
    "affine" (a layer's `_family`)."""
    from . import affine, planar, radial
    return {"planar": planar.PlanarStack, "radial": radial.RadialStack,
            "affine": affine.AffineStack}[family]


def kinds_array(kinds):
    return (ctypes.c_int32 * len(kinds))(*kinds)


def _head(dim, n_layers, kinds):
    """(dim, n_layers) as the entry points take them, then `kinds` for the
    family whose layers differ in kind (a sequence or a ctypes int32 array)."""
    head = (ctypes.c_int32(dim), ctypes.c_int32(n_layers))
    if kinds is None:
        return head
    return head + (kinds if isinstance(kinds, ctypes.Array) else kinds_array(kinds),)


def workspace_bytes(family, dim, n_layers, B, kinds=None):
    fn = "cnf_%s_workspace_bytes" % family
    n = ctypes.c_size_t()
    st = getattr(_lib.lib(), fn)(*_head(dim, n_layers, kinds), ctypes.c_int64(B), ctypes.byref(n))
    _lib.check(fn, st)
    return n.value


PLAN_FIELDS = ("lpr", "cpl", "regt", "rega", "gacc", "fwd_blocks", "bwd_blocks", "bwd_units")


def launch_plan(family, dim, n_layers, B, kinds=None):
    """What a call of this shape launches (cnf_<family>_launch_plan, host only):
    a dict of PLAN_FIELDS -- the row geometry <lpr, cpl> of the forward,
    predict and score kernels, the reverse kernel's <regt, rega>, whether the
    wave records sit in the workspace (gacc), and the grids."""
    fn = "cnf_%s_launch_plan" % family
    out = (ctypes.c_int32 * 8)()
    st = getattr(_lib.lib(), fn)(*_head(dim, n_layers, kinds), ctypes.c_int64(B), out)
    _lib.check(fn, st)
    return dict(zip(PLAN_FIELDS, out))


def param_count(family, dim, n_layers, kinds=None):
    fn = "cnf_%s_param_count" % family
    n = ctypes.c_int64()
    st = getattr(_lib.lib(), fn)(*_head(dim, n_layers, kinds), ctypes.byref(n))
    _lib.check(fn, st)
    return n.value


class RowStack(Stack):
    param_dims = (0, 1)
    entries = ()
    has_inverse = False
    _kinds = None  # mixed: the ctypes array of its layers' CNF_LAYER_* words

    @staticmethod
    def param_shape(n):
        return None

    def __init_subclass__(cls):
        # entry -> (entry point, `stats` key): forward_loss counts as a forward
        cls._names = {e: ("cnf_%s_%s" % (cls.family, e),
                          "%s_%s" % (cls.family, "forward" if e == "forward_loss" else e))
                      for e in ("forward", "forward_loss", "vjp", "loss_vjp", "predict", "score")
                      + tuple(cls.entries)}

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
        if not torch.is_tensor(p0) or p0.dim() != max(cls.param_dims):
            return False
        sizes = cls.sizes(p0.numel())
        dev = p0.device if device is None else torch.device(device)
        for ly in layers:
            for t, n in zip(tensors(ly), sizes):
                if not torch.is_tensor(t) or t.numel() != n or t.dim() not in cls.param_dims:
                    return False
                shape = cls.param_shape(n)
                if shape is not None and tuple(t.shape) != shape:
                    return False
                if t.dtype != torch.float32 or not t.is_contiguous():
                    return False
                td = t.device
                if td.type != dev.type or (dev.index is not None and td.index != dev.index):
                    return False
        return True

    def param_count(self):
        return self.L * sum(self.sizes(self.dim))

    def launch_plan(self, B):
        """The kernels and grids a call on B rows takes (rowstack.launch_plan)."""
        return launch_plan(self.family, self.dim, self.L, B, self._kinds)

    def reserve_workspace(self, B, device):
        """Hold one private workspace for batches up to B rows on `device`,
        whatever stream the calls go to (the calibrator's fit: eager epochs
        and the capturing stream of its HIP graph use the same buffer, which
        exists before the capture).  The caller keeps this stack's calls on
        one stream at a time until release_workspace()."""
        n = workspace_bytes(self.family, self.dim, self.L, B, self._kinds)
        self._own_ws = (torch.empty(max(n, 16), dtype=torch.uint8, device=device), int(B))

    def release_workspace(self):
        self._own_ws = None

    def _ws(self, x):
        """(buffer, bytes needed) for x's rows: the reserved workspace when it
        fits, else this family's buffer for (device, stream), grown on demand.
        The first point at which a shape outside the envelope raises."""
        B, dev = x.shape[0], x.device
        n = workspace_bytes(self.family, self.dim, self.L, B, self._kinds)
        if self._own_ws is not None and B <= self._own_ws[1] and self._own_ws[0].device == dev:
            return self._own_ws[0], n
        return self._buffer(self._ws_cache, _stream_key(dev), n, dev), n

    def _call(self, entry, x, ws, *args):
        """One launch of cnf_<family>_<entry> on x's device and torch's
        current stream there; `ws` is _ws(x)'s pair and `args` are what the
        entry point takes between x and B."""
        fn, counter = self._names[entry]
        B, dev = x.shape[0], x.device
        ws, n = ws
        ptrs = (ctypes.c_void_p * len(self._params))(*[p.data_ptr() for p in self._params])
        with torch.cuda.device(dev):
            st = getattr(_lib.lib(), fn)(
                *_head(self.dim, self.L, self._kinds), ptrs, _ptr(x), *args,
                ctypes.c_int64(B), _ptr(ws), ctypes.c_size_t(n), _stream(dev))
        _lib.check(fn, st)
        stats[counter] += 1

    # ---------------------------------------------------------------- launches
    # The surface of a family whose log-det is a row's, [B] (planar, mixed).
    # Affine overrides what its [1] log-det makes different, radial (no log-det
    # in any signature) all of it.
    def run(self, x, want_all=False, want_final=True):
        """(final [B, D] or None, logdet [B], all [L, B, D] or None): one
        cnf_<family>_forward call."""
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
        or None): one cnf_<family>_forward_loss call."""
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
        all_grads else z_final, the per-row log-det): one cnf_<family>_vjp call."""
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
        """Fused forward + loss + reverse mode (cnf_<family>_loss_vjp): returns
        (terms[3], flat grads, dx) with terms the sums over this batch and
        grads = grad_scale * d(sum of per-row loss)/d(params), each layer's
        tensors in ABI order, which is the state_dict order."""
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
        cnf_<family>_predict call.  Returns probs [B, D], or (probs, logdet [B]
        of the centred rows)."""
        x = self._check_input(x.detach())
        B, dev = x.shape[0], x.device
        lp = self._log_priors(log_priors, dev)
        ws = self._ws(x)
        probs = torch.empty_like(x)
        ld = torch.empty(B, dtype=torch.float32, device=dev) if want_logdet else None
        self._call("predict", x, ws, _ptr(lp), _ptr(probs), _ptr(ld))
        return (probs, ld) if want_logdet else probs

    def forward_autograd(self, x, want_all):
        """Forward with gradients w.r.t. x and every parameter: backward is
        cnf_<family>_vjp.  Returns (z_all or z_final, logdet)."""
        return _RowFn.apply(self, want_all, x, *self._params)

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


class _RowFn(StackFn):
    @staticmethod
    def forward(ctx, stack, want_all, x, *params):
        fin, ld, allt = stack.run(x, want_all=want_all)
        StackFn.saved(ctx, stack, want_all, x)
        return (allt if want_all else fin), ld
