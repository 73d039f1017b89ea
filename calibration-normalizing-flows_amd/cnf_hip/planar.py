"""Host side of the native planar-flow path (cnf_planar_*, include/cnf.h).

`PlanarStack` binds a run of PlanarLayers of one width to the fused kernels:
one launch for the forward + log-det (every layer's output optional), one for
the forward + loss terms, one for the reverse mode, one for the fused
forward + loss + reverse mode, one for the calibrator's predict (`predict`:
centring, the stack, both softmaxes and the prior correction,
cnf_planar_predict) and one for that predict ending in the calibration record
instead of the probabilities (`score`, cnf_planar_score).
`cnf_hip.adam.StackAdam` steps the stack's parameters in one launch
(cnf_adam_step_tensors) from the flat gradient `loss_and_grads` writes, and
`invalidate()` is a no-op, so the calibrator's epoch runner and its HIP-graph
replay drive a PlanarStack as they drive a CouplingStack.  The layers keep
owning `w`, `u`, `b`; the library re-derives `u_hat` inside every call.

All of that is `cnf_hip.rowstack.RowStack`'s (over `cnf_hip.stack.Stack`, the
base of every stack), the launch methods included: its surface is the one of
a family with a per-row log-det, which planar is.  This module says what a
PlanarLayer's tensors are.
"""
import operator

from . import rowstack


def workspace_bytes(dim, n_layers, B):
    return rowstack.workspace_bytes("planar", dim, n_layers, B)


def param_count(dim, n_layers):
    return rowstack.param_count("planar", dim, n_layers)


class PlanarStack(rowstack.RowStack):
    """A fused stack of PlanarLayers (flows/flows.py:129-165) of one width;
    the flat gradient is w, u, b per layer."""
    family = "planar"
    slot = "_pstack"  # where a flows.Flow keeps its stack of this class
    layer = "PlanarLayer"
    layer_tensors = operator.attrgetter("w", "u", "b")
    _ws_cache = {}

    @staticmethod
    def sizes(D):
        return D, D, 1
