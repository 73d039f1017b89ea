"""What every native stack shares: `Stack`, the base of `CouplingStack`
(cnf_hip/engine.py) and of `RowStack` (cnf_hip/rowstack.py, under
`PlanarStack`, `RadialStack` and `AffineStack`), and `StackFn`, the base of their autograd
Functions.

A stack binds a run of layers to the library's fused launches.  The layers
keep owning their parameters; the stack lists them once in ABI order
(`_params`).  Buffers are torch allocations on the input's device and the
launches go to torch's current stream there.  A subclass sets

  family      "coupling" / "planar" / "radial" / "affine" / "mixed": the word in the
              error texts
  _rows       what the input check calls its rows
  _fp32_why   why the path is fp32, in the dtype error
  _stale      what a stale backward says changed
  squeeze_logdet  whether the flow squeezes the stack's log-det as the reference's
              layers do (torch.sum(..., dim=1).squeeze()); False for a stack whose
              log-det is one number of shape [1]
"""
import ctypes

import torch

# counts of native launches (tests assert the HIP path really ran); "torch_ops"
# counts the launches that went through the torch.library operators
stats = {"forward": 0, "inverse": 0, "prepare": 0, "vjp": 0, "loss_vjp": 0, "predict": 0,
         "metrics": 0, "torch_ops": 0, "planar_forward": 0, "planar_vjp": 0,
         "planar_loss_vjp": 0, "planar_predict": 0, "planar_score": 0,
         "radial_forward": 0, "radial_vjp": 0, "radial_loss_vjp": 0, "radial_predict": 0,
         "radial_score": 0,
         "affine_forward": 0, "affine_inverse": 0, "affine_vjp": 0, "affine_loss_vjp": 0,
         "affine_predict": 0, "affine_score": 0,
         "mixed_forward": 0, "mixed_vjp": 0, "mixed_loss_vjp": 0, "mixed_predict": 0,
         "mixed_score": 0}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _stream_key(device):
    return (device, torch.cuda.current_stream(device).cuda_stream)


def upstream_grads(g_out, g_ld, all_grads, B):
    """(gz, gz_all, gld) as the reverse-mode entry points take them, from
    autograd's upstream gradients of (z_all if all_grads else z_final,
    log-det): contiguous fp32 or None, a 0-d log-det gradient expanded to the
    B rows."""
    gz = gz_all = None
    if g_out is not None:
        g_out = g_out.contiguous().float()
        if all_grads:
            gz_all = g_out
        else:
            gz = g_out
    gld = g_ld.contiguous().float().reshape(-1) if g_ld is not None else None
    if gld is not None and gld.numel() == 1 and B != 1:
        gld = gld.expand(B).contiguous()
    return gz, gz_all, gld


class Stack:
    _rows = "rows"
    _fp32_why = ""
    _stale = "parameter"
    squeeze_logdet = True

    def param_tensors(self):
        """ABI order (the state_dict order)."""
        return self._params

    def requires_grad(self):
        return any([p.requires_grad for p in self._params])

    def state_key(self):
        return tuple([(p.data_ptr(), p._version) for p in self._params])

    def _check_input(self, x):
        if not x.is_cuda:
            raise RuntimeError("native %s path needs a ROCm device tensor" % self.family)
        if x.dtype != torch.float32:
            raise TypeError("native %s path is fp32%s; got %s"
                            % (self.family, self._fp32_why, x.dtype))
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError("expected [B, %d] %s, got %s"
                             % (self.dim, self._rows, tuple(x.shape)))
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

    @staticmethod
    def _buffer(cache, key, nbytes, device):
        """cache[key], a byte buffer of at least nbytes on device, grown on
        demand.  The callers key it per (device, stream), so launches on two
        streams never share a workspace."""
        buf = cache.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = cache[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
        return buf

    def split(self, flat):
        """Views of a flat gradient, one per parameter tensor."""
        out, off = [], 0
        for p in self._params:
            out.append(flat[off:off + p.numel()].view_as(p))
            off += p.numel()
        return out

    # the calibrator's epoch runner calls these on every stack; a stack with
    # nothing to reserve or to forget keeps the no-ops
    def reserve_workspace(self, B, device):
        pass

    def release_workspace(self):
        pass

    def invalidate(self):
        pass


class StackFn(torch.autograd.Function):
    """The autograd function of a stack's transform: the subclass gives
    forward(ctx, stack, want_all, x, *params), which calls saved(); backward is
    the stack's reverse mode (`vjp` names the method; `kw`: what it takes
    besides the gradients, e.g. the prepared blob of the forward) with the
    upstream gradients in forward's output order."""

    @staticmethod
    def saved(ctx, stack, want_all, x, vjp="vjp", **kw):
        ctx.stack = stack
        ctx.want_all = want_all
        ctx.vjp_name, ctx.kw = vjp, kw
        ctx.key = stack.state_key()
        ctx.save_for_backward(x)

    @staticmethod
    def backward(ctx, *grads):
        (x,) = ctx.saved_tensors
        stack = ctx.stack
        if stack.state_key() != ctx.key:
            raise RuntimeError(
                "one of the variables needed for gradient computation has been modified by an "
                "inplace operation: a %s-layer %s changed between the native %s and its backward"
                % (stack.family, stack._stale,
                   "inverse" if ctx.vjp_name == "vjp_inverse" else "forward"))
        dx, pg = getattr(stack, ctx.vjp_name)(x, *grads, all_grads=ctx.want_all,
                                              need_dx=ctx.needs_input_grad[2], **ctx.kw)
        if torch.is_tensor(pg):  # a flat gradient: one view per parameter
            pg = stack.split(pg)
        out = [None, None, dx]
        for i, g in enumerate(pg):
            out.append(g if ctx.needs_input_grad[3 + i] else None)
        return tuple(out)
