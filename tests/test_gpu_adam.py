"""cnf_adam_step (one-launch Adam over a stack's parameters, cnf_hip/adam.py)
against torch.optim.Adam on the same gradients: the optimizer half of the
calibrator's on-device training step (reference: calibrators.py:239-295 steps
torch.optim.Adam at its defaults)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "calibration-normalizing-flows_amd"))

from cnf_hip import vjp as V  # noqa: E402
from cnf_hip.adam import StackAdam  # noqa: E402
from flows.flows import Flow, NvpCouplingLayer  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _flow(D, L, hidden, seed=0):
    # 100-wide conditioners at N(0, 0.1) make the loss chaotic within a few
    # Adam steps (gradients grow 5x): rounding-level parameter differences then
    # grow past any tolerance, so the wide case starts near the smooth regime
    torch.manual_seed(seed)
    f = Flow([NvpCouplingLayer(D, hidden) for _ in range(L)])
    g = torch.Generator().manual_seed(seed)
    sigma = 0.1 if D <= 16 else 0.02
    with torch.no_grad():
        for p in f.parameters():
            if p.requires_grad:
                p.copy_(torch.randn(p.shape, generator=g) * sigma)
    return f


@pytest.mark.parametrize("D,L,hidden,wd", [(10, 6, [5, 5], 0.0), (100, 2, [100, 100], 0.01),
                                           (20, 24, [8, 8], 0.0),  # 288 tensors: 3 launches
                                           (10, 12, [5, 5], 0.0)])  # narrow, L > 8
def test_stack_adam_matches_torch_adam(D, L, hidden, wd):
    fa = _flow(D, L, hidden).to(DEV)
    fb = _flow(D, L, hidden).to(DEV)
    sa = fa._native_stack()
    ta = torch.optim.Adam([p for p in fb.parameters() if p.requires_grad], lr=3e-3,
                          weight_decay=wd)
    na = StackAdam.like(sa, torch.optim.Adam([p for p in fa.parameters() if p.requires_grad],
                                             lr=3e-3, weight_decay=wd))
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(4096, D, device=DEV, generator=g)
    y = torch.randint(0, D, (4096,), device=DEV, generator=g)
    for _ in range(5):
        _, ga, _ = V.loss_and_grads(sa, x, y, grad_scale=1.0 / 4096)
        na.step(ga)
        _, gb, _ = V.loss_and_grads(fb._native_stack(), x, y, grad_scale=1.0 / 4096)
        for p, gg in zip([p for p in fb.parameters() if p.requires_grad],
                         V._split(fb._native_stack(), gb)):
            p.grad = gg.view_as(p)
        ta.step()
    # Adam's step is ~lr per element whatever the gradient's size, so the scale
    # of a difference is the total movement (5 lr), not |p|
    for (k, p), (_, q) in zip(fa.named_parameters(), fb.named_parameters()):
        if p.requires_grad:
            assert ((p - q).abs() / (q.abs() + 5 * 3e-3)).max().item() <= 1e-4, k
    # the updated weights reach the kernels (the prepared-weight cache rebuilt)
    z1, _ = fa.transform(x)
    z2, _ = fb.transform(x)
    assert ((z1 - z2).abs() / (z2.abs() + 1)).max().item() <= 1e-5


def test_desc_entry_points_match_tensor_list():
    """The three cnf_desc Adam entry points against cnf_adam_step_tensors over
    the same tensor list, through ctypes on copies of one state (parameters,
    a flat gradient, moments from one prior step): StackAdam steps every stack
    through cnf_adam_step_tensors, so this is the device run of cnf_adam_step,
    _sched and _guarded.  Same kernel, same grid: parameters and both moments
    equal bit for bit; a raised skip flag moves nothing."""
    import ctypes

    from cnf_hip import _lib
    from cnf_hip.stack import _ptr, _stream

    stack = _flow(3, 2, [3, 3], seed=3).to(DEV)._native_stack()
    ps0 = [p.detach().clone() for p in stack.param_tensors()]
    n = stack.param_count()
    g = torch.Generator(device=DEV).manual_seed(4)
    grad = torch.randn(n, device=DEV, generator=g) * 0.1
    g1 = torch.randn(n, device=DEV, generator=g) * 0.1  # the prior step's gradient
    m0, v0 = 0.1 * g1, 0.001 * g1 * g1
    hp = [ctypes.c_double(v) for v in (0.9, 0.999, 1e-8, 0.01)]
    step, lr = ctypes.c_int64(2), ctypes.c_double(3e-3)
    sched = torch.tensor([3e-3 / (1 - 0.9 ** 2), (1 - 0.999 ** 2) ** 0.5], device=DEV)
    flags = [torch.tensor([f], dtype=torch.int32, device=DEV) for f in (0, 1)]
    lib, desc, st = _lib.lib(), ctypes.byref(stack.desc), _stream(torch.device(DEV))
    numel = (ctypes.c_int64 * len(ps0))(*[p.numel() for p in ps0])

    def run(call):
        ps = [p.clone() for p in ps0]
        m, v = m0.clone(), v0.clone()
        arr = (ctypes.c_void_p * len(ps))(*[p.data_ptr() for p in ps])
        _lib.check("adam", call(arr, _ptr(grad), _ptr(m), _ptr(v)))
        torch.cuda.synchronize()
        return ps + [m, v]

    def tensors(sched_t, skip_t):
        return run(lambda arr, g_, m, v: lib.cnf_adam_step_tensors(
            ctypes.c_int32(len(ps0)), numel, arr, g_, m, v, step, lr, _ptr(sched_t), *hp,
            _ptr(skip_t), st))

    def same(a, b):
        return all(torch.equal(s, t) for s, t in zip(a, b))

    plain = run(lambda arr, g_, m, v: lib.cnf_adam_step(desc, arr, g_, m, v, step, lr, *hp, st))
    assert same(plain, tensors(None, None))
    assert not same(plain, ps0 + [m0, v0])  # the step moved the state
    sch = run(lambda arr, g_, m, v: lib.cnf_adam_step_sched(desc, arr, g_, m, v, _ptr(sched),
                                                            *hp, st))
    assert same(sch, tensors(sched, None))
    for flag in flags:
        guarded = run(lambda arr, g_, m, v: lib.cnf_adam_step_guarded(
            desc, arr, g_, m, v, step, lr, None, *hp, _ptr(flag), st))
        assert same(guarded, tensors(None, flag))
    assert same(guarded, ps0 + [m0, v0])  # flag 1: nothing moves
    assert same(run(lambda arr, g_, m, v: lib.cnf_adam_step_guarded(
        desc, arr, g_, m, v, step, lr, None, *hp, _ptr(flags[0]), st)), plain)
