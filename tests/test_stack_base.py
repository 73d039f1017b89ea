"""What cnf_hip.stack.Stack gives every stack, on host layers (no device):
the flat-gradient split, the parameter count and the normalisation of
autograd's upstream gradients."""
import pytest
import torch

from cnf_hip.engine import CouplingStack
from cnf_hip.planar import PlanarStack
from cnf_hip.radial import RadialStack
from cnf_hip.stack import Stack, upstream_grads
from flows.flows import NvpCouplingLayer, PlanarLayer, RadialLayer


def _stacks():
    torch.manual_seed(0)
    return [CouplingStack([NvpCouplingLayer(5, [3, 4], random_flip=True) for _ in range(2)]),
            CouplingStack([NvpCouplingLayer(4, [3], scale=False)]),
            PlanarStack([PlanarLayer(5) for _ in range(3)]),
            RadialStack([RadialLayer(5) for _ in range(3)])]


@pytest.mark.parametrize("stack", _stacks(), ids=lambda s: "%s-%d" % (s.family, s.dim))
def test_split_and_param_count(stack):
    assert isinstance(stack, Stack)
    ps = stack.param_tensors()
    n = sum(p.numel() for p in ps)
    assert stack.param_count() == n
    flat = torch.arange(n, dtype=torch.float32)
    views = stack.split(flat)
    assert [v.shape for v in views] == [p.shape for p in ps]
    assert torch.equal(torch.cat([v.reshape(-1) for v in views]), flat)
    assert all(v.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
               for v in views)


def test_upstream_grads():
    B, D, L = 4, 3, 2
    g, g_all = torch.randn(B, D), torch.randn(L, B, D)
    gld = torch.randn(B)
    gz, gza, out_ld = upstream_grads(g, gld, False, B)
    assert gz is not None and torch.equal(gz, g) and gza is None and torch.equal(out_ld, gld)
    gz, gza, _ = upstream_grads(g_all, gld, True, B)
    assert gz is None and torch.equal(gza, g_all)
    # strided or double upstream gradients arrive contiguous fp32
    gz, _, out_ld = upstream_grads(g.double().t().contiguous().t(), gld.double(), False, B)
    assert gz.is_contiguous() and gz.dtype == torch.float32 and out_ld.dtype == torch.float32
    # a 0-d log-det gradient (the sum of a broadcast) covers the B rows
    _, _, out_ld = upstream_grads(None, torch.tensor(2.0), False, B)
    assert out_ld.shape == (B,) and out_ld.is_contiguous()
    assert torch.equal(out_ld, torch.full((B,), 2.0))
    _, _, out_ld = upstream_grads(None, torch.tensor(2.0), False, 1)
    assert out_ld.shape == (1,)
    assert upstream_grads(None, None, True, B) == (None, None, None)
