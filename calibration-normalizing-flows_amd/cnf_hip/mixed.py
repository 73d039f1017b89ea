"""Host side of the native mixed row-wise path (cnf_mixed_*, include/cnf.h).

`MixedStack` binds a run of PlanarLayers, RadialLayers and AffineConstantLayers
(both parameters) of one width, in any order, to the fused kernels.  Its
surface is `cnf_hip.rowstack.RowStack`'s, inherited whole as `PlanarStack`
inherits it: one launch for the forward + per-row log-det (every layer's
output optional), one for the forward + loss terms, one for the reverse mode,
one for the fused forward + loss + reverse mode, one for the calibrator's
predict and one for that predict ending in the calibration record (`score`).
This module holds what the layers' differing kinds add: `kinds`, the host
array of CNF_LAYER_* words the entry points take after n_layers, built once
from the layer classes (RowStack's launch frame passes it); `compatible`, per
layer; and the parameter count, a per-kind sum.  The parameter table has
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
import torch

from . import _lib, rowstack

KIND = {"planar": _lib.LAYER_PLANAR, "radial": _lib.LAYER_RADIAL, "affine": _lib.LAYER_AFFINE}


# per family: parameter names in ABI order, how many trailing ones are scalars,
# the dimensions of the vectors (affine: [1, D])
_SPEC = {"planar": (("w", "u", "b"), 1, 1), "radial": (("z0", "a", "b"), 2, 1),
         "affine": (("s", "t"), 0, 2)}


def _layer_class(family):
    from flows import flows
    return {"planar": flows.PlanarLayer, "radial": flows.RadialLayer,
            "affine": flows.AffineConstantLayer}[family]


def workspace_bytes(dim, kinds, B):
    return rowstack.workspace_bytes("mixed", dim, len(kinds), B, kinds)


def launch_plan(dim, kinds, B):
    """What a call of this shape launches (cnf_mixed_launch_plan, host only):
    a dict of rowstack.PLAN_FIELDS."""
    return rowstack.launch_plan("mixed", dim, len(kinds), B, kinds)


def param_count(dim, kinds):
    return rowstack.param_count("mixed", dim, len(kinds), kinds)


class MixedStack(rowstack.RowStack):
    """A fused stack of PlanarLayers, RadialLayers and AffineConstantLayers of
    one width (flows/flows.py), in any order."""
    family = "mixed"
    slot = "_mstack"  # where a flows.Flow keeps its stack of this class
    squeeze_logdet = False  # the flow shapes the log-det itself (flows.mixed_logdet_shape)
    _ws_cache = {}
    # no `sizes`, on purpose: tensor sizes go by a layer's kind, so the two
    # RowStack methods that ask it, compatible and param_count, are overridden

    @staticmethod
    def layer_tensors(layer):
        """The layer's parameter tensors in its family's ABI order."""
        return rowstack.stack_class(layer._family).layer_tensors(layer)

    def __init__(self, layers):
        super().__init__(layers)
        self.kinds = [KIND[ly._family] for ly in self.layers]
        self._kinds = rowstack.kinds_array(self.kinds)  # what RowStack's frame passes

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
