"""Drop-in replacement for the reference's flows/flows.py.

Same classes, constructor arguments, attributes, state_dict keys and return
conventions as the reference (SergioAlvarezB/calibration-normalizing-flows,
flows/flows.py), so `from flows.flows import Flow, NvpCouplingLayer` works
unchanged.  On a ROCm device a Flow made of NvpCouplingLayers runs as ONE fused
HIP launch per call (libcnf_hip.so, include/cnf.h), and so does a Flow made of
PlanarLayers (cnf_planar_*) or of RadialLayers (cnf_radial_*; both forward
only, neither flow has a tractable inverse), and a Flow made of
AffineConstantLayers that have both parameters (cnf_affine_*: forward and
inverse, the log-det one number of shape [1] as the reference's):

  Flow.forward(x)  -> (zs, cum_log_det)   fused cnf_forward, zs = views of one
                                           [L, B, D] buffer       (flows.py:17-25)
  Flow.backward(z) -> (xs, cum_log_det)   fused cnf_inverse        (flows.py:27-37)
  NvpCouplingLayer.forward / .backward    the same kernels, L = 1  (flows.py:101-126)

`backward` is the reference's name for the INVERSE transform; gradients come
from torch autograd, which calls the native VJP kernel.

Host tensors (CPU) run the same math with torch ops, as the reference does.
A Flow that mixes PlanarLayers, RadialLayers and AffineConstantLayers of one
width runs as one fused launch too (cnf_mixed_*), whenever the layer loop
would accept its order (mixed_logdet_shape).
Layers the native engine does not cover (an AffineConstantLayer built with
scale=False or shift=False) and stacks that mix them or coupling layers in run
layer by layer, and so does Flow.backward of an affine flow under autograd
(the native inverse has no reverse mode).  CNF_MIXED_NATIVE=0 keeps mixed
flows on that loop.  CNF_PLANAR_NATIVE=0 keeps planar flows on the torch ops
as well, CNF_RADIAL_NATIVE=0 radial ones and CNF_AFFINE_NATIVE=0 affine ones.  A radial stack's log-det is the reference's
constant log(1) = 0: the native path returns the same 0-d fp32 zero.

A planar, radial or affine stack's other launches hang off the same kind of
binding (cnf_hip/planar.py, cnf_hip/radial.py, cnf_hip/affine.py over the base
they share,
cnf_hip/rowstack.py): the fused training step and loss
evaluation, the calibrator's fused predict and score (cnf_planar_predict,
cnf_radial_predict, cnf_affine_predict, ..._score) and the one-launch Adam step
(cnf_adam_step_tensors); calibrators.TorchFlowCalibrator drives them, HIP-graph
epoch replay included.
"""
import os
import warnings

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .utils import MLP

# Reproduce the reference's `0 * inf = NaN` at masked positions when exp(s)
# overflows there (flows/flows.py:107).  Off by default: it costs the kernel
# the masked half of the last Linear; finite results are identical either way.
STRICT_NAN = os.environ.get("CNF_STRICT_NAN", "0") == "1"
# Raise instead of running torch ops when a ROCm tensor cannot take the
# native path (unsupported shape or activation).
STRICT_NATIVE = os.environ.get("CNF_STRICT_NATIVE", "0") == "1"

# CNF_PLANAR_NATIVE=0: planar flows on a ROCm device stay on the torch ops
# (the baseline of tools/planar_bench.py).
PLANAR_NATIVE = os.environ.get("CNF_PLANAR_NATIVE", "1") != "0"
# CNF_RADIAL_NATIVE=0: the same for radial flows (the baseline of
# tools/radial_bench.py).
RADIAL_NATIVE = os.environ.get("CNF_RADIAL_NATIVE", "1") != "0"
# CNF_AFFINE_NATIVE=0: the same for affine-constant flows (the baseline of
# tools/affine_bench.py).
AFFINE_NATIVE = os.environ.get("CNF_AFFINE_NATIVE", "1") != "0"
# CNF_MIXED_NATIVE=0: flows that mix planar, radial and affine layers run layer
# by layer, each layer on its own family's launch (the baseline of
# tools/mixed_bench.py).
MIXED_NATIVE = os.environ.get("CNF_MIXED_NATIVE", "1") != "0"

_warned = set()


def _not_native(reason):
    if STRICT_NATIVE:
        raise RuntimeError("native coupling path unavailable: " + reason)
    if reason not in _warned:
        _warned.add(reason)
        warnings.warn("cnf: running torch ops on the GPU (%s)" % reason, RuntimeWarning)


def _device_rows(x):
    """True when x is a 2-d fp32 tensor on a ROCm device."""
    return isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 \
        and x.dim() == 2


def _strict(obj):
    """The strictness rule of a Flow or a layer: its own `strict_nan` when
    set, else CNF_STRICT_NAN."""
    return STRICT_NAN if obj.strict_nan is None else bool(obj.strict_nan)


def _native_eligible(layers, x):
    """True when these layers can run as one fused native stack on x."""
    if not _device_rows(x):
        return False
    if not layers or not all(isinstance(ly, NvpCouplingLayer) for ly in layers):
        return False
    for ly in layers:
        for net in (ly.s, ly.t):
            if isinstance(net, MLP) and net.activation is not F.relu:
                _not_native("conditioner activation %r" % (net.activation,))
                return False
    from cnf_hip.engine import CouplingStack
    if not CouplingStack.compatible(layers):
        return False
    if x.shape[1] != layers[0].dim:
        return False
    return True


def _family_switches():
    return {"planar": PLANAR_NATIVE, "radial": RADIAL_NATIVE, "affine": AFFINE_NATIVE}


def mixed_logdet_shape(layers, B):
    """The shape of the log-det the layer loop of Flow.forward gives a flow of
    planar, radial and affine layers on B rows, or None when the loop raises.
    The loop accumulates in place into the first layer's log-det, so that
    shape must already be the broadcast of every layer's: planar [B] (0-d for
    one row, after its squeeze), radial 0-d, affine [1]."""
    per = {"planar": () if B == 1 else (B,), "radial": (), "affine": (1,)}
    shapes = {per[ly._family] for ly in layers}
    # the broadcast of 0-d, [1] and [B] shapes: the rows' where there is one
    # ([0] for no row), else [1] where there is one, else 0-d
    full = (B,) if (B,) in shapes else (1,) if (1,) in shapes else ()
    first = per[layers[0]._family]
    return first if full == first else None


def _mixed_class(layers, x, families):
    """MixedStack when these layers -- planar, radial and affine, at least two
    of the classes -- can run on x as one fused launch, or None: every layer
    compatible on its own (an affine layer with both parameters, every tensor
    on x's device), one width, no switch of a family present turned off, and an
    order whose log-det the layer loop accepts on x's rows
    (mixed_logdet_shape).  A radial first layer stays on the loop: its log-det
    is a host tensor, into which the loop cannot accumulate a device one."""
    switches = _family_switches()
    if not MIXED_NATIVE or not all(switches.get(f, False) for f in families):
        return None
    if not _device_rows(x) or layers[0]._family == "radial":
        return None
    shape = mixed_logdet_shape(layers, x.shape[0])
    if shape is None or (shape == (1,) and x.shape[0] == 0):  # [1] of no row: the loop's ops
        return None
    from cnf_hip.mixed import MixedStack
    if not MixedStack.compatible(layers, x.device):
        return None
    return MixedStack if x.shape[1] == MixedStack.layer_tensors(layers[0])[0].numel() else None


def _row_class(layers, x):
    """The stack class (PlanarStack / RadialStack / AffineStack, or MixedStack for
    layers of more than one of their classes) under which these layers can
    run on x as one fused launch of a row-wise family, or None.  The family's
    switch is read here, at call time, and with the input's device before
    anything of cnf_hip is touched."""
    families = {getattr(ly, "_family", None) for ly in layers}
    if len(families) > 1:
        return None if None in families else _mixed_class(layers, x, families)
    family = getattr(layers[0], "_family", None) if layers else None
    if family is None or not _family_switches()[family]:
        return None
    if not _device_rows(x):
        return None
    from cnf_hip.rowstack import stack_class
    cls = stack_class(family)
    # every layer of the family's class; PlanarLayer(params=...) tensors that
    # sit on another device fall through to the torch ops, which fail there as
    # the reference does
    if not cls.compatible(layers, x.device):
        return None
    return cls if x.shape[1] == cls.layer_tensors(layers[0])[0].numel() else None


def _run_stack(stack, x, want_all, inverse=False):
    """(zs list | final z, log-det) from one fused launch of any stack (a
    RadialStack's log-det is the 0-d zero), under autograd when a gradient is
    wanted, or None when the shape is outside the kernels' envelope.  A
    CouplingStack and an AffineStack have an inverse; only the former's has a
    reverse mode.  An AffineStack's log-det keeps its shape [1], as the
    reference's torch.sum(s, dim=1) does for every batch size."""
    from cnf_hip._lib import UnsupportedShape
    try:
        if torch.is_grad_enabled() and (x.requires_grad or stack.requires_grad()):
            if inverse:  # cnf_vjp_inverse (strict_nan included)
                out, ld = stack.inverse_autograd(x, want_all=want_all)
            else:
                out, ld = stack.forward_autograd(x, want_all=want_all)
        else:
            if inverse:
                fin, ld, allt = stack.run(x, inverse=True, want_all=want_all)
            else:
                fin, ld, allt = stack.run(x, want_all=want_all)
            out = allt if want_all else fin
        if stack.squeeze_logdet:
            ld = _squeeze_ld(ld)
        elif stack.family == "mixed":
            # the loop's shape: the rows' [B], or the first row of [B] rows that
            # agree ([1], 0-d) -- a slice, so autograd reaches the kernel's gld
            shape = mixed_logdet_shape(stack.layers, x.shape[0])
            if shape != tuple(ld.shape):
                ld = ld[:1].reshape(shape)
        return (list(out.unbind(0)) if want_all else out), ld
    except UnsupportedShape as e:
        _not_native(str(e))
        return None


def _wants_grad(x, stack):
    return torch.is_grad_enabled() and (x.requires_grad or stack.requires_grad())


def _layer_native(layer, x, inverse=False):
    """A PlanarLayer's, RadialLayer's or AffineConstantLayer's forward (the
    last one's inverse as well, when no gradient is wanted) as one fused launch
    on its own single-layer stack (rebuilt when a parameter was replaced), or
    None."""
    cls = _row_class([layer], x)
    if cls is None or (inverse and not cls.has_inverse):
        return None
    st = getattr(layer, "_stack", None)
    if st is None or any(t is not p for t, p in zip(st.param_tensors(), cls.layer_tensors(layer))):
        st = layer._stack = cls([layer])
    if inverse and _wants_grad(x, st):
        return None
    return _run_stack(st, x, False, inverse)


def _squeeze_ld(ld):
    # torch.sum(..., dim=1).squeeze(): 0-d for a single row (flows/flows.py:109)
    return ld.squeeze()


class Flow(nn.Module):
    """Sequential flow (reference flows/flows.py:8-37)."""

    def __init__(self, layers, **kwargs):
        super().__init__()
        self.layers = nn.ModuleList(layers)
        # a flow is computationally invertible iff every layer is
        self.invertible = all(ly.invertible for ly in self.layers)
        self.strict_nan = kwargs.get("strict_nan", None)
        # cnf_desc.options bits (cnf_hip._lib.OPT_*): keep launches off a kernel
        # family, for A/B runs and tests; 0 = the fastest kernel
        self.native_options = int(kwargs.get("native_options", 0))
        self._drop_bindings(self.__dict__)

    # the lazily built native bindings, each with the key it was built for:
    # the CouplingStack, the PlanarStack, the RadialStack, the AffineStack, the
    # MixedStack
    _BINDINGS = ("_stack", "_pstack", "_rstack", "_astack", "_mstack")

    @classmethod
    def _drop_bindings(cls, attrs):
        for slot in cls._BINDINGS:
            attrs[slot] = None
            attrs[slot + "_key"] = None

    def __getstate__(self):
        # the native binding (ctypes descriptor, device blobs) is rebuilt lazily
        st = self.__dict__.copy()
        self._drop_bindings(st)
        return st

    # -- native plumbing --------------------------------------------------
    def _native_stack(self):
        key = (tuple(id(ly) for ly in self.layers), self._strict(), self.native_options)
        if self._stack is None or self._stack_key != key:
            from cnf_hip.engine import CouplingStack
            self._stack = CouplingStack(list(self.layers), strict_nan=self._strict(),
                                        options=self.native_options)
            self._stack_key = key
        return self._stack

    def _row_stack(self, cls, layers):
        """The stack of class `cls` over `layers` (list(self.layers)), kept in
        the slot the class names (_pstack, _rstack, _astack, _mstack) and rebuilt when a layer or
        one of its parameters was replaced; a flow unpickled from before the
        slot existed builds it as well."""
        tensors = cls.layer_tensors
        key = list(map(id, layers)) + [id(t) for ly in layers for t in tensors(ly)]
        st = getattr(self, cls.slot, None)
        if st is None or getattr(self, cls.slot + "_key") != key:
            st = cls(layers)
            setattr(self, cls.slot, st)
            setattr(self, cls.slot + "_key", key)
        return st

    def _planar_stack(self):
        from cnf_hip.planar import PlanarStack
        return self._row_stack(PlanarStack, list(self.layers))

    def _radial_stack(self):
        from cnf_hip.radial import RadialStack
        return self._row_stack(RadialStack, list(self.layers))

    def invalidate_native(self):
        """Drop the native binding's prepared weights.  Needed only after writes
        that bypass torch's version counters (`p.data.copy_(...)`); optimizer
        steps, `load_state_dict` and in-place ops are tracked automatically."""
        self._drop_bindings(self.__dict__)
        for ly in self.layers:
            if isinstance(ly, NvpCouplingLayer):
                ly._stack = None

    def _strict(self):
        return _strict(self)

    def _try_native(self, x, inverse, want_all=True):
        """(zs list | final z, log-det) from one fused launch, or None."""
        layers = list(self.layers)
        cls = _row_class(layers, x)
        if cls is not None:
            if not inverse:
                return _run_stack(self._row_stack(cls, layers), x, want_all)
            if not cls.has_inverse:
                return None
            # a row family's inverse (affine) has no reverse mode: under
            # autograd it stays on the torch ops
            st = self._row_stack(cls, layers)
            return None if _wants_grad(x, st) else _run_stack(st, x, want_all, True)
        if not _native_eligible(layers, x):
            return None
        return _run_stack(self._native_stack(), x, want_all, inverse)

    def transform(self, x):
        """Final output and log-det only -- (zs[-1], cum_log_det) without
        materialising the intermediate layer outputs."""
        out = self._try_native(x, inverse=False, want_all=False)
        if out is not None:
            return out
        zs, ld = Flow.forward(self, x)
        return zs[-1], ld

    def inverse_transform(self, z):
        """(xs[-1], cum_log_det) of Flow.backward without the intermediates."""
        if not self.invertible:
            raise ValueError('Flow inverse not tractable!')
        out = self._try_native(z, inverse=True, want_all=False)
        if out is not None:
            return out
        xs, ld = Flow.backward(self, z)
        return xs[-1], ld

    # -- reference API ----------------------------------------------------
    def forward(self, x):
        out = self._try_native(x, inverse=False)
        if out is not None:
            return out
        cum_log_det = 0.0
        zs = []
        for layer in self.layers:
            x, log_det = layer(x)
            zs.append(x)
            cum_log_det += log_det
        return zs, cum_log_det

    def backward(self, z):
        if not self.invertible:
            raise ValueError('Flow inverse not tractable!')
        out = self._try_native(z, inverse=True)
        if out is not None:
            return out
        cum_log_det = 0.0
        xs = []
        for layer in reversed(self.layers):
            z, log_det = layer.backward(z)
            xs.append(z)
            cum_log_det += log_det
        return xs, cum_log_det


class AffineConstantLayer(nn.Module):
    """z = x*exp(s) + t with per-feature constants (reference flows/flows.py:40-65).
    With both parameters, on a ROCm device one fused launch per direction
    (cnf_affine_forward / cnf_affine_inverse, L = 1; the inverse only when no
    gradient is wanted); torch ops on the host and for scale=False /
    shift=False layers.  The log-det has shape [1]."""
    _family = "affine"

    def __init__(self, dim, scale=True, shift=True):
        super().__init__()
        self.s = nn.Parameter(torch.zeros(1, dim, requires_grad=True)) if scale else None
        self.t = nn.Parameter(torch.zeros(1, dim, requires_grad=True)) if shift else None
        self.invertible = True
        self._stack = None

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_stack"] = None
        return st

    def _st(self, x):
        s = self.s if self.s is not None else x.new_zeros(x.size())
        t = self.t if self.t is not None else x.new_zeros(x.size())
        return s, t

    def forward(self, x):
        out = _layer_native(self, x)
        if out is not None:
            return out
        s, t = self._st(x)
        return x * torch.exp(s) + t, torch.sum(s, dim=1)

    def backward(self, z):
        out = _layer_native(self, z, inverse=True)
        if out is not None:
            return out
        s, t = self._st(z)
        return (z - t) * torch.exp(-s), torch.sum(-s, dim=1)


class NvpCouplingLayer(nn.Module):
    """RealNVP affine coupling (NICE additive when scale=False), fixed half
    mask, feature flip after the layer, optional random permutation
    (reference flows/flows.py:68-126)."""

    def __init__(self, dim, hidden_size=[5, 5], scale=True, shift=True, random_flip=False):
        super().__init__()
        # conditioner nets; the reference draws their init in this order
        self.s = MLP(dim, hidden_size, wscale=0.001) if scale \
            else (lambda x: x.new_zeros(x.size()))
        self.t = MLP(dim, hidden_size, wscale=0.001) if shift \
            else (lambda x: x.new_zeros(x.size()))
        mask = np.zeros((1, dim))
        mask[:, dim // 2:] = 1
        self.mask = nn.Parameter(torch.as_tensor(mask.copy(), dtype=torch.float),
                                 requires_grad=False)
        self.invertible = True
        self.random_flip = random_flip
        # shape record used by the native engine (not part of the state_dict)
        self.dim = dim
        self.hidden_size = list(hidden_size)
        self.scale = bool(scale)
        self.shift = bool(shift)
        self.strict_nan = None
        self._stack = None
        if random_flip:
            perm = np.random.permutation(dim)
            rev = np.zeros(dim)
            rev[perm] = np.arange(dim)
            self.perm = nn.Parameter(torch.as_tensor(perm[None], dtype=torch.long),
                                     requires_grad=False)
            self.rev_perm = nn.Parameter(torch.as_tensor(rev[None], dtype=torch.long),
                                         requires_grad=False)

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_stack"] = None
        return st

    def _native(self, x, inverse):
        if not _native_eligible([self], x):
            return None
        from cnf_hip.engine import CouplingStack
        strict = _strict(self)
        if self._stack is None or self._stack.strict_nan != strict:
            self._stack = CouplingStack([self], strict_nan=strict)
        return _run_stack(self._stack, x, False, inverse)

    def forward(self, x):
        out = self._native(x, inverse=False)
        if out is not None:
            return out
        keep = self.mask * x              # conditioning half (mask = 1)
        free = 1 - self.mask              # transformed half
        s, t = self.s(keep), self.t(keep)
        z = keep + free * (x * torch.exp(s) + t)
        log_det = torch.sum(free * s, dim=1).squeeze()
        if self.random_flip:
            z = z[:, self.perm.reshape(-1)]
        return z.flip((1,)), log_det

    def backward(self, z):
        out = self._native(z, inverse=True)
        if out is not None:
            return out
        z = z.flip((1,))
        if self.random_flip:
            z = z[:, self.rev_perm.reshape(-1)]
        keep = self.mask * z
        free = 1 - self.mask
        s, t = self.s(keep), self.t(keep)
        x = keep + free * (z - t) * torch.exp(-s)
        log_det = torch.sum(free * (-s), dim=1).squeeze()
        return x, log_det


class PlanarLayer(nn.Module):
    """Planar flow (reference flows/flows.py:129-165); non-invertible.  On a
    ROCm device one fused launch (cnf_planar_forward, L = 1); torch ops on the
    host."""
    _family = "planar"  # the row-wise family of cnf_hip.rowstack

    def __init__(self, dim=0, params=None):
        super().__init__()
        if params is not None:
            self.w = params['w'].squeeze()
            self.u = params['u'].squeeze()
            self.b = params['b'].squeeze()
        else:
            if dim < 1:
                raise ValueError('Either dim of params must be provided!')
            self.w = nn.Parameter(torch.rand(dim))
            self.u = nn.Parameter(torch.rand(dim))
            self.b = nn.Parameter(torch.rand(1))
        self.invertible = False
        self._stack = None

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_stack"] = None
        return st

    def forward(self, x):
        out = _layer_native(self, x)
        if out is not None:
            return out
        wtu = torch.dot(self.w, self.u)
        m = -1 + torch.log1p(torch.exp(wtu))   # keeps w.u_hat >= -1
        u_hat = self.u + (m - wtu) * self.w / torch.norm(self.w)
        h = torch.tanh(torch.matmul(x, self.w) + self.b)
        z = x + torch.matmul(h.view(-1, 1), u_hat.view(1, -1))
        psi = torch.matmul((1 - h ** 2).view(-1, 1), self.w.view(1, -1))
        det = torch.abs(1 + torch.matmul(psi, u_hat.view(-1, 1)))
        return z, torch.log(det.squeeze())


class RadialLayer(nn.Module):
    """Radial flow (reference flows/flows.py:168-193); non-invertible.  Its
    log-det is the constant log(1) = 0, as in the reference.  On a ROCm device
    one fused launch (cnf_radial_forward, L = 1); torch ops on the host."""
    _family = "radial"

    def __init__(self, dim):
        super().__init__()
        self.z0 = nn.Parameter(torch.rand(dim))
        self.a = nn.Parameter(torch.rand(1))
        self.b = nn.Parameter(torch.rand(1))
        self.invertible = False
        self._stack = None

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_stack"] = None
        return st

    def forward(self, x):
        out = _layer_native(self, x)
        if out is not None:
            return out
        b_hat = -self.a + torch.log1p(torch.exp(self.b))
        diff = x - self.z0
        h = 1. / (self.a + torch.norm(diff, dim=1, keepdim=True))
        z = x + b_hat * h.expand_as(diff) * diff
        return z, torch.log(torch.tensor(1.0))
