"""Flow factories for TorchFlowCalibrator (calibrators.py:239-353).

The calibrator builds its flow as `Flow(n_classes, **kwargs)` (calibrators.py:251)
with kwargs that also carry `dev`, `epochs`, `batch_size`, and calls it as
`pred, log_det = self.flow(x)` (calibrators.py:287, 304, 339): the FINAL output,
not the reference Flow's list.  The reference notebooks import such factories
from `flows.realNVP_torch` / `flows.nice_torch`, modules absent from the
reference repo; their defaults here follow code-old/realNVP.py:46-52
(layers=4, hidden_size=[dim]) and are otherwise unpinned.

PlanarFlow, RadialFlow and AffineConstantFlow are what the calibration
notebooks import from `flows.normalizing_flows_torch` (re-exported there),
another module absent from the reference repo, so their defaults are unpinned
too: layers=10 is the notebooks' planar / radial depth, layers=5 the
AffineConstantFlow depth of train-flows-det.ipynb.
"""
from .flows import AffineConstantLayer, Flow, NvpCouplingLayer, PlanarLayer, RadialLayer


class CouplingFlow(Flow):
    """A Flow of NvpCouplingLayers whose call returns (z_final, log_det)."""

    scale = True

    def __init__(self, dim, layers=4, hidden_size=None, random_flip=False, strict_nan=None,
                 **kwargs):
        hidden = [dim] if hidden_size is None else list(hidden_size)
        super().__init__([NvpCouplingLayer(dim, hidden, scale=self.scale, shift=True,
                                           random_flip=random_flip) for _ in range(layers)],
                         strict_nan=strict_nan)
        self.dim = dim

    def forward(self, x):
        return self.transform(x)

    def backward(self, z):
        return self.inverse_transform(z)

    def forward_all(self, x):
        """The reference Flow.forward: (zs list, cum_log_det)."""
        return Flow.forward(self, x)


class PlanarFlow(Flow):
    """A Flow of PlanarLayers whose call returns (z_final, log_det); layers=10
    as get_Planarmodel of the reference's calibration notebooks."""

    def __init__(self, dim, layers=10, **kwargs):
        super().__init__([PlanarLayer(dim) for _ in range(layers)])
        self.dim = dim

    def forward(self, x):
        return self.transform(x)

    def forward_all(self, x):
        """The reference Flow.forward: (zs list, cum_log_det)."""
        return Flow.forward(self, x)


class RadialFlow(Flow):
    """A Flow of RadialLayers whose call returns (z_final, log_det), the
    log-det being the reference's constant 0-d zero; layers=10 as the planar
    factory."""

    def __init__(self, dim, layers=10, **kwargs):
        super().__init__([RadialLayer(dim) for _ in range(layers)])
        self.dim = dim

    def forward(self, x):
        return self.transform(x)

    def forward_all(self, x):
        """The reference Flow.forward: (zs list, cum_log_det)."""
        return Flow.forward(self, x)


class AffineConstantFlow(Flow):
    """A Flow of AffineConstantLayers (z = x * exp(s) + t per layer) whose call
    returns (z_final, log_det), the log-det of shape [1] as the reference's
    layers return it.  On a ROCm device one fused launch per call
    (cnf_affine_forward / cnf_affine_inverse), as the planar and radial
    factories; layers=5 is the depth of train-flows-det.ipynb."""

    def __init__(self, dim, layers=5, **kwargs):
        super().__init__([AffineConstantLayer(dim) for _ in range(layers)])
        self.dim = dim

    def forward(self, x):
        return self.transform(x)

    def backward(self, z):
        return self.inverse_transform(z)

    def forward_all(self, x):
        """The reference Flow.forward: (zs list, cum_log_det)."""
        return Flow.forward(self, x)


class MixedFlow(Flow):
    """A Flow that mixes the three row-wise layers, whose call returns
    (z_final, log_det): `layers` is a spec string over P (PlanarLayer), R
    (RadialLayer) and A (AffineConstantLayer), one letter per layer in order,
    e.g. "PRPRA".  On a ROCm device one fused launch per call (cnf_mixed_*)
    for every order whose log-det the layer loop accepts: planar first for a
    batch of more than one row (flows.mixed_logdet_shape).  The default is
    unpinned (no notebook builds one)."""

    _LAYERS = {"P": PlanarLayer, "R": RadialLayer, "A": AffineConstantLayer}

    def __init__(self, dim, layers="PRPRA", **kwargs):
        spec = str(layers).upper()
        if not spec or any(c not in self._LAYERS for c in spec):
            raise ValueError("MixedFlow: layers must be a non-empty string over P, R, A; got %r"
                             % (layers,))
        super().__init__([self._LAYERS[c](dim) for c in spec])
        self.dim = dim
        self.spec = spec

    def forward(self, x):
        return self.transform(x)

    def forward_all(self, x):
        """The reference Flow.forward: (zs list, cum_log_det)."""
        return Flow.forward(self, x)
