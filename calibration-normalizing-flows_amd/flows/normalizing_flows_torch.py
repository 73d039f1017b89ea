"""The module the calibration notebooks import their flow factories from:

    from flows.normalizing_flows_torch import PlanarFlow, RadialFlow, AffineConstantFlow

It is absent from the reference repo; the factories live in flows/_factory.py
(whose docstring says which defaults are pinned by the notebooks and which are
not) and are re-exported here so that line works verbatim.  MixedFlow, the
factory of flows that mix the three layers, is exported alongside them.
"""
from ._factory import AffineConstantFlow, MixedFlow, PlanarFlow, RadialFlow

__all__ = ["PlanarFlow", "RadialFlow", "AffineConstantFlow", "MixedFlow"]
