"""Reverse mode of the fused coupling stack (cnf_vjp / cnf_loss_vjp, include/cnf.h).

The launches are `CouplingStack`'s methods (cnf_hip/engine.py): `vjp` is what
torch autograd calls for Flow.forward on a ROCm device, `loss_and_grads` the
fused calibrator step (forward + loss + reverse mode in one launch plus a
fixed-order reduction), used by the native TorchFlowCalibrator and by the
data-parallel trainer.  The module-level names below are the call forms that
tests and tools use.  This module keeps the torch-autograd reverse mode of the
shapes without a native one.
"""
import warnings

import torch

from . import _lib


def stack_vjp(stack, x, g_out, g_ld, all_grads, need_dx, blob=None):
    return stack.vjp(x, g_out, g_ld, all_grads, need_dx, blob)


def stack_vjp_inverse(stack, z, g_out, g_ld, all_grads, need_dz, blob=None):
    return stack.vjp_inverse(z, g_out, g_ld, all_grads, need_dz, blob)


def loss_and_grads(stack, x, y, **kw):
    return stack.loss_and_grads(x, y, **kw)


def _split(stack, flat):
    return stack.split(flat)


_warned = set()


def _torch_vjp(stack, x, g_out, g_ld, all_grads, need_dx):
    """Reverse modes the ABI reports unsupported (CNF_ERR_UNSUPPORTED: shapes
    past the layer-at-a-time kernels' LDS envelope): autograd through the
    layers' own torch ops, on the same device.  strict_nan stacks have native
    reverse modes for the forward and the inverse."""
    key = (stack.dim, tuple(stack.hidden), stack.strict_nan)
    if stack.options & (_lib.OPT_ALT_MASK | _lib.OPT_S_TANH):
        # _torch_forward restates the maintained (ReLU, data-flip) layer only:
        # a legacy stack must not differentiate through it
        raise _lib.UnsupportedShape("cnf_vjp", -3, _lib.lib())
    from flows.flows import STRICT_NATIVE
    if STRICT_NATIVE:
        raise RuntimeError("native coupling path unavailable: no native VJP for %s" % (key,))
    if key not in _warned:
        _warned.add(key)
        warnings.warn("cnf: no native VJP for %s; using torch autograd" % (key,), RuntimeWarning)
    ps = stack.param_tensors()
    with torch.enable_grad():
        xx = x.detach().requires_grad_(need_dx)
        leaves = [p.detach().requires_grad_(True) for p in ps]
        # re-bind the detached leaves into the layers' math
        zs, ld = _torch_forward(stack, xx, leaves)
        outs, grads_in = [], []
        if g_out is not None:
            outs.append(torch.stack(zs) if all_grads else zs[-1])
            grads_in.append(g_out)
        if g_ld is not None:
            outs.append(ld)
            grads_in.append(g_ld.reshape(ld.shape))
        inputs = leaves + ([xx] if need_dx else [])
        if not outs:
            return (torch.zeros_like(x) if need_dx else None), [torch.zeros_like(p) for p in ps]
        res = torch.autograd.grad(outs, inputs, grads_in, allow_unused=True)
    res = [torch.zeros_like(t) if r is None else r for r, t in zip(res, inputs)]
    dx = res[-1] if need_dx else None
    return dx, list(res[:len(leaves)])


def _torch_forward(stack, x, leaves):
    it = iter(leaves)
    ld = torch.zeros(x.shape[0], device=x.device)
    zs = []
    n_lin = len(stack.hidden) + 1
    for ly in stack.layers:
        nets = []
        for on in (stack.scale, stack.shift):
            nets.append([(next(it), next(it)) for _ in range(n_lin)] if on else None)
        mask = ly.mask
        keep = mask * x
        free = 1 - mask

        def run(net, h):
            if net is None:
                return torch.zeros_like(h)
            for i, (W, b) in enumerate(net):
                h = torch.nn.functional.linear(h, W, b)
                if i < len(net) - 1:
                    h = torch.relu(h)
            return h
        s, t = run(nets[0], keep), run(nets[1], keep)
        z = keep + free * (x * torch.exp(s) + t)
        ld = ld + torch.sum(free * s, dim=1)
        if ly.random_flip:
            z = z[:, ly.perm.reshape(-1)]
        x = z.flip((1,))
        zs.append(x)
    return zs, ld
