"""The generic MFMA-tile family (k_tile, cnf_tile.hip) at the edges of
tile_configure: narrow shapes outside the compile-time tables, exact tile
multiples, width 1, nothing a multiple of 4 or 16, the deepest conditioner the
ABI takes, and the wide shapes where the block drops to 3, 2 and 1 waves.

Forward, inverse and every-layer outputs, non-strict and strict_nan, against
the float64 numpy oracle at the bars of tests/test_gpu_table_forward.py; the
layer-at-a-time reverse mode against float64 CPU autograd at 1e-4 where
vjp_kernel_name() is "layerwise", and "none" asserted where the shape is past
its LDS bound."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import _sweep
from _golden import rel_err
from cnf_hip import _lib, engine
from oracle import cnf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
GRAD_TOL = 1e-4

# (D, hidden, L, flip, tile_waves, reverse-mode path)
SHAPES = [
    (7, [5, 5], 3, True, 4, "layerwise"),     # D <= 16 outside the table; odd D
    (16, [16], 2, False, 4, "layerwise"),     # exact tile multiples
    (9, [1], 2, False, 4, "layerwise"),       # hidden width 1
    (33, [17, 15], 2, False, 4, "layerwise"),  # nothing a multiple of 4 or 16
    (12, [6] * 8, 2, False, 4, "layerwise"),  # CNF_MAX_HIDDEN hidden layers
    (100, [160], 2, False, 3, "layerwise"),
    (128, [256], 2, False, 2, "layerwise"),
    (256, [512], 2, False, 1, "none"),        # CNF_MAX_DIM, CNF_MAX_WIDTH; past wvjp_ok's LDS
]
IDS = [_sweep.shape_id(s[0], s[1]) for s in SHAPES]


def tile_waves(D, hidden, strict):
    """tile_configure (cnf_tile.hip): 16-row wave tiles of [2 dp + 2 hp + 2 nop]
    floats per row, as many waves (at most 4) as fit 160 KB of LDS."""
    NO = D if strict else D // 2
    hp = max([16] + [(h + 15) // 16 * 16 for h in hidden])
    nop = (NO + 15) // 16 * 16
    dp = (D + 3) // 4 * 4 + 4
    per_wave = (2 * dp + 2 * hp + 2 * nop) * 16 * 4
    return min(4, (160 * 1024) // per_wave)


def test_tile_waves_of_the_table_rows():
    for D, hidden, _, _, waves, _ in SHAPES:
        assert tile_waves(D, hidden, False) == waves, (D, hidden)
    assert [tile_waves(D, h, True) for D, h, *_ in SHAPES[-3:]] == [3, 2, 1]


def _sigma(D):
    return 0.2 if D <= 24 else 0.05


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("strict", [False, True], ids=["fast", "strict"])
@pytest.mark.parametrize("D,hidden,L,flip,waves,path", SHAPES, ids=IDS)
def test_forward_inverse_against_float64(D, hidden, L, flip, waves, path, strict):
    BMAX = 16 * waves * 2 + 5
    x, _, _ = _sweep.inputs(BMAX, D, seed=1)
    flow, _, x = _sweep.conditioned_flow(D, L, hidden, x, flip=flip, sigma=_sigma(D))
    l64, l32 = _sweep.oracle_layers(flow, np.float64), _sweep.oracle_layers(flow, np.float32)
    zs64, ld64 = O.flow_forward(l64, x.numpy().astype(np.float64))
    zs64 = np.stack(zs64)
    z32 = zs64[-1].astype(np.float32)
    xs64, ild64 = O.flow_inverse(l64, z32.astype(np.float64))
    xs32, ild32 = O.flow_inverse(l32, z32)
    xs64, xs32 = np.stack(xs64), np.stack(xs32)
    fg = flow.to(DEV)
    fg.strict_nan = strict
    stack = fg._native_stack()
    assert stack.kernel_name() == "mfma-tile" and stack.strict_nan == strict
    xg, zg = x.to(DEV), torch.from_numpy(z32).to(DEV)
    worst_f = worst_i = worst_floor = 0.0
    for B in (1, BMAX):
        n0 = engine.stats["forward"] + engine.stats["inverse"]
        with torch.no_grad():
            z, ld = fg.transform(xg[:B])
            zs, lda = fg(xg[:B])
            xr, ild = fg.inverse_transform(zg[:B])
            xs, ilda = fg.backward(zg[:B])
        assert engine.stats["forward"] + engine.stats["inverse"] == n0 + 4, "native path did not run"
        e = [rel_err(_np(z), zs64[-1, :B]), rel_err(_np(ld).reshape(-1), ld64[:B]),
             rel_err(_np(torch.stack(zs)), zs64[:, :B]), rel_err(_np(lda).reshape(-1), ld64[:B])]
        floor = max(rel_err(xs32[:, :B], xs64[:, :B]), rel_err(ild32[:B], ild64[:B]))
        bar = max(TOL, 2 * floor)
        ei = [rel_err(_np(xr), xs64[-1, :B]), rel_err(_np(ild).reshape(-1), ild64[:B]),
              rel_err(_np(torch.stack(xs)), xs64[:, :B]),
              rel_err(_np(ilda).reshape(-1), ild64[:B])]
        print("%s strict=%d B=%d: fwd %s inv %s (fp32 oracle %.2e, bar %.2e)"
              % (_sweep.shape_id(D, hidden), strict, B, e, ei, floor, bar))
        assert max(e) <= TOL, (B, e)
        assert max(ei) <= bar, (B, ei, bar)
        worst_f, worst_i, worst_floor = max(worst_f, *e), max(worst_i, *ei), max(worst_floor, floor)
    _sweep.record({"test": "tile_forward", "D": D, "hidden": hidden, "strict": strict,
                   "kernel": "mfma-tile", "waves": tile_waves(D, hidden, strict),
                   "fwd_err": worst_f, "inv_err": worst_i, "inv_fp32_oracle_err": worst_floor})


@pytest.mark.parametrize("D,hidden,L,flip,waves,path", SHAPES, ids=IDS)
def test_reverse_mode(D, hidden, L, flip, waves, path):
    BMAX = 16 * waves * 2 + 5
    x, y, _ = _sweep.inputs(BMAX, D, seed=1)
    if path == "none":
        flow = _sweep.make_flow(D, L, hidden, _sigma(D), _sweep.SEED0, flip=flip)
        stack = flow.to(DEV)._native_stack()
        assert stack.vjp_kernel_name() == "none" and not stack.has_native_vjp()
        n = ctypes.c_size_t()
        assert _lib.lib().cnf_vjp_workspace_bytes(ctypes.byref(stack.desc), ctypes.c_int64(BMAX),
                                                  ctypes.byref(n)) == -3   # CNF_ERR_UNSUPPORTED
        return
    flow, seed, x = _sweep.guarded_flow(D, L, hidden, x, flip=flip, sigma=_sigma(D))
    f64 = _sweep.ref64(flow)
    fg = copy.deepcopy(flow).to(DEV)
    stack = fg._native_stack()
    assert stack.kernel_name() == "mfma-tile" and stack.vjp_kernel_name() == path
    params = lambda f: [(k, p) for k, p in f.named_parameters() if p.requires_grad]
    names = [k for k, _ in params(fg)]
    g = torch.Generator().manual_seed(2)
    w = torch.randn(L, BMAX, D, generator=g)
    wl = torch.randn(BMAX, generator=g)

    def worst(got, ref):
        e = [_sweep.grad_err(a, b) for a, b in zip(got, ref)]
        return max(e), names[int(np.argmax(e))]

    worst_all = 0.0
    for B in (1, BMAX):
        for every_layer in (True, False):
            f64.zero_grad()
            xc = x[:B].double().requires_grad_(True)
            zs, ld = f64(xc)
            obj = (ld.reshape(-1) * wl[:B].double()).sum()
            for l in (range(L) if every_layer else [L - 1]):
                obj = obj + (zs[l] * w[l, :B].double()).sum()
            obj.backward()
            ref_g = [p.grad.numpy().copy() for _, p in params(f64)]
            fg.zero_grad()
            xg = x[:B].to(DEV).requires_grad_(True)
            n0, t0 = engine.stats["vjp"], engine.stats["torch_ops"]
            if every_layer:
                zs, ld = fg(xg)
                obj = (ld.reshape(-1) * wl[:B].to(DEV)).sum()
                for l in range(L):
                    obj = obj + (zs[l] * w[l, :B].to(DEV)).sum()
            else:
                z, ld = fg.transform(xg)
                obj = (ld.reshape(-1) * wl[:B].to(DEV)).sum() + (z * w[-1, :B].to(DEV)).sum()
            obj.backward()
            assert engine.stats["vjp"] == n0 + 1 or engine.stats["torch_ops"] > t0
            wg, where = worst([_np(p.grad) for _, p in params(fg)], ref_g)
            wx = _sweep.grad_err(_np(xg.grad), xc.grad.numpy())
            print("%s B=%d every_layer=%d seed=%d: grads %.2e (%s) dx %.2e"
                  % (_sweep.shape_id(D, hidden), B, every_layer, seed, wg, where, wx))
            assert wg <= GRAD_TOL and wx <= GRAD_TOL, (B, every_layer, wg, where, wx)
            worst_all = max(worst_all, wg, wx)
        # the calibrator loss (kind cal)
        f64.zero_grad()
        xc = x[:B].double().requires_grad_(True)
        zs, ld = f64(xc)
        rows = _sweep.loss_rows64(zs[-1], ld.reshape(-1), y[:B], 0, 1.0)
        (rows[0].sum() / B).backward()
        ref_g = [p.grad.numpy().copy() for _, p in params(f64)]
        rows = rows.detach().numpy()
        terms, grads, dx = stack.loss_and_grads(x[:B].to(DEV), y[:B].to(DEV), kind=0, det=1.0,
                                                grad_scale=1.0 / B, need_dx=True)
        terr = np.abs(terms.double().cpu().numpy() - rows.sum(axis=1))
        bound = 1e-5 * np.abs(rows).sum(axis=1)
        wg, where = worst([_np(t) for t in stack.split(grads)], ref_g)
        wx = _sweep.grad_err(_np(dx), xc.grad.numpy())
        print("%s B=%d cal loss: terms err %s bound %s grads %.2e (%s) dx %.2e"
              % (_sweep.shape_id(D, hidden), B, terr, bound, wg, where, wx))
        assert np.all(terr <= bound), (B, terr, bound)
        assert wg <= GRAD_TOL and wx <= GRAD_TOL, (B, wg, where, wx)
        worst_all = max(worst_all, wg, wx)
    _sweep.record({"test": "tile_vjp", "D": D, "hidden": hidden, "path": path, "seed": seed,
                   "grad_err": worst_all})
