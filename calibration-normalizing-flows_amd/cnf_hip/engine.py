"""Host side of the native coupling-flow path: descriptor, prepared-weight
cache, launches on torch's current HIP stream, and the autograd binding.

`CouplingStack` binds a run of identically-shaped NvpCouplingLayers to ONE
fused launch (cnf_forward / cnf_inverse / cnf_vjp in include/cnf.h).  All
buffers are torch allocations on the input's device; the stream is
`torch.cuda.current_stream()`, so launches order with surrounding torch work
and can be captured into a CUDA(HIP) graph.

Cache validity.  The prepared blob (weights re-laid out for the kernels, the
flip / random_flip permutation folded into gather tables) is rebuilt whenever
a parameter's or a permutation's storage or in-place version changes: optimizer
steps, `load_state_dict` and `copy_` all bump `_version`.  Writes through
`.data` do not (torch hides them from autograd too); after such a write call
`Flow.invalidate_native()` (or `CouplingStack.invalidate()`).  A backward whose
weights changed in place since its forward raises, as autograd does.
"""
import ctypes

import torch

from . import _lib
from .stack import Stack, StackFn, _ptr, _stream, _stream_key, stats, upstream_grads
from .vjp import _torch_vjp

# Dispatch through torch.ops.cnf (C++ operators, autograd in C++) when
# libcnf_torch.so is built; False: the ctypes calls of the same C ABI.
USE_TORCH_OPS = True


def _ops():
    return _lib.torch_ops() if USE_TORCH_OPS else None


def vjp_launch_plan(desc, B, inverse=False):
    """cnf_vjp_launch_plan (host only) as a dict with "path" and, per path, the
    fields include/cnf.h lists -- layerwise: kNJ, keep_acts, nkb, rows_kb,
    nseed, wave_blocks, dw16_z, gemms (a set of (BT, EPI, PAIR, NC)), ny,
    chunks; wide-fused: row, nets, nkb, rows_kb, nseed, wdwg, dw16_z, classes
    (a set of (G tiles, H tiles))."""
    out = (ctypes.c_int32 * _lib.VJP_PLAN_WORDS)()
    _lib.check("cnf_vjp_launch_plan", _lib.lib().cnf_vjp_launch_plan(
        ctypes.byref(desc), ctypes.c_int64(B), ctypes.c_int32(int(bool(inverse))), out))
    plan = {"path": _lib.VJP_PATHS[out[0]]}
    bits = lambda names, w: {n for i, n in enumerate(names) if w >> i & 1}
    if plan["path"] == "layerwise":
        plan.update(kNJ=out[1], keep_acts=bool(out[2]), nkb=out[3], rows_kb=out[4],
                    nseed=out[5], wave_blocks=out[6], dw16_z=out[7],
                    gemms=bits(_lib.WGEMM_BITS, out[8]), ny=out[9], chunks=out[10])
    elif plan["path"] == "wide-fused":
        plan.update(row=out[1], nets=out[2], nkb=out[3], rows_kb=out[4], nseed=out[5],
                    wdwg=bool(out[6]), dw16_z=out[7], classes=bits(_lib.WDWG_CLASSES, out[8]))
    return plan


class CouplingStack(Stack):
    """A fused stack of NvpCouplingLayers (flows/flows.py:68-126) sharing
    dim / hidden_size / scale / shift.  Layers keep owning their parameters;
    the stack only reads them (state_dict order) through cnf_prepare."""
    family = "coupling"
    _rows = "logits"
    _fp32_why = " (the reference's nn.Linear weights are fp32)"
    _stale = "weight or permutation"
    # reverse-mode workspaces (per-block gradient partials) of every coupling
    # stack: one per (entry point, device, stream).  Nothing is reserved for the
    # calibrator's epoch runner: the workspaces a capture creates live in the
    # graph's private pool.
    _ws_cache = {}

    def __init__(self, layers, strict_nan=False, options=0):
        layers = list(layers)
        l0 = layers[0]
        self.layers = layers
        self.dim = l0.dim
        self.hidden = list(l0.hidden_size)
        self.scale = bool(l0.scale)
        self.shift = bool(l0.shift)
        self.strict_nan = bool(strict_nan)
        self.options = int(options)
        self.L = len(layers)
        self._perm_key = None
        self._perms = None
        # the Parameter objects are fixed for the stack's life (load_state_dict
        # and .to() update them in place); nn.Module attribute lookups cost
        # ~4 us each, so the list is gathered once
        self._params = self._gather_params()
        self._refresh_desc()
        self._cache = {}
        self._loss_ws = {}
        self._vjp_ok = None
        self._vjp_inv_ok = None

    # -- descriptor and permutations ----------------------------------------
    def _perm_tensors(self):
        return [ly.perm for ly in self.layers if ly.random_flip]

    def _perm_state(self):
        return tuple((p.data_ptr(), p._version) for p in self._perm_tensors())

    def _refresh_desc(self):
        """(Re)build the host permutation table and the descriptor from the
        layers' current `perm` values (one small D2H copy, only on change)."""
        self._perm_key = self._perm_state()
        if any(ly.random_flip for ly in self.layers):
            p = torch.full((self.L, self.dim), -1, dtype=torch.int64)
            for i, ly in enumerate(self.layers):
                if ly.random_flip:
                    p[i] = ly.perm.detach().reshape(-1).cpu()
            self._perms = p.contiguous()
        else:
            self._perms = None
        self.desc = _lib.make_desc(self.dim, self.L, self.hidden, self.scale, self.shift,
                                   self.strict_nan, self._perms, self.options)
        self.desc_ints = _lib.desc_list(self.desc)

    def invalidate(self):
        """Forget every prepared blob (after writes the version counters do
        not see, e.g. through `.data`)."""
        self._cache.clear()
        self._perm_key = None

    @staticmethod
    def compatible(layers):
        l0 = layers[0]
        return all(ly.dim == l0.dim and list(ly.hidden_size) == list(l0.hidden_size)
                   and ly.scale == l0.scale and ly.shift == l0.shift for ly in layers)

    def kernel_name(self, all_outputs=False):
        """Kernel family serving this stack; every-layer-output calls of an
        sgpr-fused stack run on valu-fused (cnf_valu.hip valu_run)."""
        name = _lib.lib().cnf_kernel_name(ctypes.byref(self.desc)).decode()
        return "valu-fused" if all_outputs and name == "sgpr-fused" else name

    def vjp_kernel_name(self):
        """Reverse-mode path of cnf_vjp / cnf_loss_vjp for this stack: "vjp2",
        "vjp-rows", "layerwise", "wide-fused" or "none" (cnf_vjp_kernel_name)."""
        return _lib.lib().cnf_vjp_kernel_name(ctypes.byref(self.desc)).decode()

    def vjp_launch_plan(self, B, inverse=False):
        """What the reverse mode of a call on B rows launches (vjp_launch_plan
        above; inverse: cnf_vjp_inverse)."""
        return vjp_launch_plan(self.desc, B, inverse)

    def has_native_vjp(self):
        """True when cnf_vjp serves this descriptor (every shape within the
        ABI's limits, strict_nan included, except strict stacks under the legacy
        alternate mask or tanh s-net).  Cached: support depends only on the
        shape and options."""
        if self._vjp_ok is None:
            n = ctypes.c_size_t()
            st = _lib.lib().cnf_vjp_workspace_bytes(ctypes.byref(self.desc), ctypes.c_int64(1),
                                                    ctypes.byref(n))
            self._vjp_ok = st == 0
        return self._vjp_ok

    def _gather_params(self):
        out = []
        for ly in self.layers:
            for net, on in ((ly.s, self.scale), (ly.t, self.shift)):
                if on:
                    for lin in net.layers:
                        out.append(lin.weight)
                        out.append(lin.bias)
        return out

    def param_count(self):
        n = ctypes.c_int64()
        _lib.check("cnf_param_count", _lib.lib().cnf_param_count(ctypes.byref(self.desc),
                                                                  ctypes.byref(n)))
        return n.value

    def state_key(self):
        """Identity of everything the prepared blob encodes."""
        return (Stack.state_key(self), self._perm_state())

    def prepared(self, device):
        """Device blob for this stack, rebuilt only when a parameter or a
        permutation changed (storage or in-place version counter)."""
        if self._perm_state() != self._perm_key:
            self._refresh_desc()
            self._cache.clear()
        key = self.state_key()
        ent = self._cache.get(device)
        if ent is not None and ent[0] == key:
            return ent[1]
        ps = self._params
        for p in ps:
            if p.device != device or p.dtype != torch.float32:
                raise TypeError("native coupling path needs fp32 parameters on %s" % device)
        lib = _lib.lib()
        nbytes = ctypes.c_size_t()
        _lib.check("cnf_prepared_bytes", lib.cnf_prepared_bytes(ctypes.byref(self.desc),
                                                                 ctypes.byref(nbytes)))
        blob = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=device)
        cps = [p.detach().contiguous() for p in ps]
        arr = (ctypes.c_void_p * max(len(cps), 1))(*[c.data_ptr() for c in cps])
        _lib.check("cnf_prepare", lib.cnf_prepare(ctypes.byref(self.desc), arr, _ptr(blob),
                                                  _stream(device)))
        stats["prepare"] += 1
        # keep the parameter tensors referenced so the key's pointers stay theirs
        self._cache[device] = (key, blob, cps)
        return blob

    # ---------------------------------------------------------------- launches
    def _workspace(self, entry, cache, B, dev):
        """(buffer, bytes) of <entry>_workspace_bytes for B rows: cache's
        buffer for (entry, device, stream), grown on demand."""
        fn = entry + "_workspace_bytes"
        n = ctypes.c_size_t()
        _lib.check(fn, getattr(_lib.lib(), fn)(ctypes.byref(self.desc), ctypes.c_int64(B),
                                               ctypes.byref(n)))
        return self._buffer(cache, (entry,) + _stream_key(dev), n.value, dev), n.value

    def run(self, x, inverse=False, want_all=False, want_final=True, blob=None):
        """Returns (final [B,D] or None, logdet [B], all [L,B,D] or None)."""
        x = self._check_input(x)
        B = x.shape[0]
        dev = x.device
        if blob is None:
            blob = self.prepared(dev)
        ops = _ops()
        if ops is not None:
            out, ld = ops.forward(x, blob, self.desc_ints, self._perms, inverse, want_all)
            stats["inverse" if inverse else "forward"] += 1
            stats["torch_ops"] += 1
            if want_all:
                return (out[-1] if want_final else None), ld, out
            return out, ld, None
        ld = torch.empty(B, dtype=torch.float32, device=dev)
        allt = torch.empty(self.L, B, self.dim, dtype=torch.float32, device=dev) \
            if want_all else None
        fin = torch.empty(B, self.dim, dtype=torch.float32, device=dev) \
            if (want_final and not want_all) else None
        lib = _lib.lib()
        fn = lib.cnf_inverse if inverse else lib.cnf_forward
        st = fn(ctypes.byref(self.desc), _ptr(blob), _ptr(x), _ptr(fin), _ptr(ld), _ptr(allt),
                ctypes.c_int64(B), _stream(dev))
        _lib.check("cnf_inverse" if inverse else "cnf_forward", st)
        stats["inverse" if inverse else "forward"] += 1
        if want_all and want_final:
            fin = allt[-1]
        return fin, ld, allt

    def forward_loss(self, x, y, kind=_lib.LOSS_CAL, det=1.0, want_outputs=False,
                     terms_out=None):
        """Fused forward + log-det + loss terms (cnf_forward_loss): returns
        (terms[3] = sums over the rows of (loss, ce, log-det), z or None, ld or None).
        A label outside [0, D) makes the terms NaN (the reference raises).
        terms_out: a caller-provided fp32 [3] destination on x's device."""
        x = self._check_input(x)
        y = y.contiguous().to(torch.int64)
        B = x.shape[0]
        dev = x.device
        blob = self.prepared(dev)
        # this stack's partial-sum records, one workspace per (device, stream)
        ws, nws = self._workspace("cnf_forward_loss", self._loss_ws, B, dev)
        terms = self._out_buffer(terms_out, 3, dev, "forward_loss: terms_out")
        z = torch.empty_like(x) if want_outputs else None
        ld = torch.empty(B, dtype=torch.float32, device=dev) if want_outputs else None
        st = _lib.lib().cnf_forward_loss(
            ctypes.byref(self.desc), _ptr(blob), _ptr(x), _ptr(y), ctypes.c_int32(kind),
            ctypes.c_float(det), _ptr(z), _ptr(ld), _ptr(terms), ctypes.c_int64(B), _ptr(ws),
            ctypes.c_size_t(nws), _stream(dev))
        _lib.check("cnf_forward_loss", st)
        stats["forward"] += 1
        return terms, z, ld

    def loss_and_grads(self, x, y, kind=_lib.LOSS_CAL, det=1.0, grad_scale=1.0, need_dx=False,
                       grads_out=None, terms_out=None):
        """Fused forward + loss + reverse mode (cnf_loss_vjp).  Returns
        (terms[3], flat grads, dx) where terms = (sum of per-row loss, sum of
        ce, sum of log-det) over THIS batch and grads = grad_scale * d(sum of
        per-row loss)/d(params).  grads_out / terms_out: caller-provided
        contiguous fp32 destinations (e.g. the two parts of one all-reduce
        buffer)."""
        x = x.contiguous()
        y = y.contiguous().to(torch.int64)
        B = x.shape[0]
        dev = x.device
        blob = self.prepared(dev)
        ws, nws = self._workspace("cnf_vjp", self._ws_cache, B, dev)
        what = "loss_and_grads: output buffer"
        grads = self._out_buffer(grads_out, self.param_count(), dev, what)
        terms = self._out_buffer(terms_out, 3, dev, what)
        dx = torch.empty_like(x) if need_dx else None
        st = _lib.lib().cnf_loss_vjp(
            ctypes.byref(self.desc), _ptr(blob), _ptr(x), _ptr(y), ctypes.c_int32(kind),
            ctypes.c_float(det), ctypes.c_float(grad_scale), _ptr(terms), _ptr(grads), _ptr(dx),
            ctypes.c_int64(B), _ptr(ws), ctypes.c_size_t(nws), _stream(dev))
        _lib.check("cnf_loss_vjp", st)
        stats["loss_vjp"] += 1
        return terms, grads, dx

    def _reverse(self, entry, x, g_out, g_ld, all_grads, need_dx, blob, ws):
        """One cnf_vjp / cnf_vjp_inverse call: (status, dx or None, flat grads)."""
        B, dev = x.shape[0], x.device
        grads = torch.empty(self.param_count(), dtype=torch.float32, device=dev)
        dx = torch.empty_like(x) if need_dx else None
        gz, gza, gld = upstream_grads(g_out, g_ld, all_grads, B)
        st = getattr(_lib.lib(), entry)(
            ctypes.byref(self.desc), _ptr(blob), _ptr(x), _ptr(gz), _ptr(gza), _ptr(gld),
            _ptr(grads), _ptr(dx), ctypes.c_int64(B), _ptr(ws[0]), ctypes.c_size_t(ws[1]),
            _stream(dev))
        return st, dx, grads

    def vjp(self, x, g_out, g_ld, all_grads, need_dx, blob=None):
        """(dx or None, [grad per parameter]) for the upstream gradients of
        (z_all if all_grads else z_final, log-det); `blob`: the prepared weights
        the forward ran with.  A shape without a native reverse mode goes to
        torch autograd (vjp._torch_vjp)."""
        x = x.contiguous()
        try:
            if blob is None:
                blob = self.prepared(x.device)
            ws = self._workspace("cnf_vjp", self._ws_cache, x.shape[0], x.device)
        except _lib.UnsupportedShape:
            return _torch_vjp(self, x, g_out, g_ld, all_grads, need_dx)
        st, dx, grads = self._reverse("cnf_vjp", x, g_out, g_ld, all_grads, need_dx, blob, ws)
        if st == -3:
            return _torch_vjp(self, x, g_out, g_ld, all_grads, need_dx)
        _lib.check("cnf_vjp", st)
        stats["vjp"] += 1
        return dx, self.split(grads)

    def vjp_inverse(self, z, g_out, g_ld, all_grads, need_dx, blob=None):
        """(dz or None, [grad per parameter]) of the INVERSE transform for the
        upstream gradients of (x_all if all_grads else x_final, log-det)
        (cnf_vjp_inverse, include/cnf.h)."""
        z = z.contiguous()
        if blob is None:
            blob = self.prepared(z.device)
        ws = self._workspace("cnf_vjp_inverse", self._ws_cache, z.shape[0], z.device)
        st, dz, grads = self._reverse("cnf_vjp_inverse", z, g_out, g_ld, all_grads, need_dx,
                                      blob, ws)
        _lib.check("cnf_vjp_inverse", st)
        stats["vjp"] += 1
        return dz, self.split(grads)

    def predict(self, x, log_priors, want_logdet=False):
        """Calibrated probabilities softmax(log(softmax(flow(x - mean x)) + 1e-7)
        - log_priors) (Calibrator.predict, calibrators.py:40-44, 330-353):
        one fused cnf_predict launch (k_sgpr, random_flip included; k_wide),
        or -- for shapes it does not cover (strict_nan, legacy options, wide
        shapes outside k_wide's table) -- cnf_forward followed by the same
        math as device torch ops."""
        x = self._check_input(x)
        B = x.shape[0]
        dev = x.device
        lp = self._log_priors(log_priors, dev)
        blob = self.prepared(dev)
        probs = torch.empty_like(x)
        ld = torch.empty(B, dtype=torch.float32, device=dev) if want_logdet else None
        st = _lib.lib().cnf_predict(ctypes.byref(self.desc), _ptr(blob), _ptr(x), _ptr(lp),
                                    _ptr(probs), _ptr(ld), ctypes.c_int64(B), _stream(dev))
        if st == 0:
            stats["predict"] += 1
            return (probs, ld) if want_logdet else probs
        if st != -3:
            _lib.check("cnf_predict", st)
        xc = x - x.mean(dim=1, keepdim=True)
        z, ld, _ = self.run(xc, blob=blob)
        p = torch.softmax(z, dim=1)
        probs = torch.softmax(torch.log(p + 1e-7) - lp, dim=1)
        return (probs, ld) if want_logdet else probs

    def score(self, x, log_priors, y, bins=15, record=None):
        """ADD the calibration record (cnf_hip.metrics) of predict(x,
        log_priors) against the labels y into `record` and return it: the
        fused predict plus one cnf_metrics launch."""
        from .metrics import calibration_record
        return calibration_record(self.predict(x, log_priors), y, bins, record)

    # -------------------------------------------------------------- autograd
    def forward_autograd(self, x, want_all):
        """Forward with gradients w.r.t. x and every parameter (cnf_vjp): the
        cnf::flow operator (autograd kernel in C++) or the Python Function.
        Stacks whose reverse mode the ABI reports unsupported (legacy strict
        options) take the Python Function, whose backward falls back to torch
        autograd (vjp._torch_vjp); the C++ kernel would raise there."""
        ps = self.param_tensors()
        ops = _ops()
        if ops is not None and self.has_native_vjp():
            x = self._check_input(x)
            blob = self.prepared(x.device)
            stats["forward"] += 1
            stats["torch_ops"] += 1
            return ops.flow(x, blob, self.desc_ints, self._perms, want_all, ps)
        return _StackFn.apply(self, want_all, x, *ps)

    def has_native_vjp_inverse(self):
        """True when cnf_vjp_inverse serves this descriptor (strict_nan included)."""
        if self._vjp_inv_ok is None:
            n = ctypes.c_size_t()
            st = _lib.lib().cnf_vjp_inverse_workspace_bytes(ctypes.byref(self.desc),
                                                            ctypes.c_int64(1), ctypes.byref(n))
            self._vjp_inv_ok = st == 0
        return self._vjp_inv_ok

    def inverse_autograd(self, z, want_all):
        """Inverse with gradients w.r.t. z and every parameter
        (cnf_vjp_inverse, the layer-at-a-time reverse mode): the
        cnf::inverse_flow operator (autograd kernel in C++) or the Python
        Function."""
        ps = self.param_tensors()
        ops = _ops()
        if ops is not None and self.has_native_vjp_inverse():
            z = self._check_input(z)
            blob = self.prepared(z.device)
            stats["inverse"] += 1
            stats["torch_ops"] += 1
            return ops.inverse_flow(z, blob, self.desc_ints, self._perms, want_all, ps)
        return _InvStackFn.apply(self, want_all, z, *ps)


class _StackFn(StackFn):
    """Flow.forward under autograd: cnf_forward forward, cnf_vjp backward on
    the prepared blob the forward ran with."""

    @staticmethod
    def forward(ctx, stack, want_all, x, *params):
        blob = stack.prepared(x.device)
        fin, ld, allt = stack.run(x, inverse=False, want_all=want_all, blob=blob)
        StackFn.saved(ctx, stack, want_all, x, blob=blob)
        return (allt if want_all else fin), ld


class _InvStackFn(StackFn):
    """Flow.backward (the inverse transform) under autograd: cnf_inverse
    forward, cnf_vjp_inverse backward."""

    @staticmethod
    def forward(ctx, stack, want_all, z, *params):
        blob = stack.prepared(z.device)
        fin, ld, allt = stack.run(z, inverse=True, want_all=want_all, blob=blob)
        StackFn.saved(ctx, stack, want_all, z, vjp="vjp_inverse", blob=blob)
        return (allt if want_all else fin), ld
