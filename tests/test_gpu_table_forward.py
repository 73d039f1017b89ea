"""Forward family of every narrow-table shape against a float64 reference.

For each of the 18 shapes of kTable (cnf_valu.hip; 15 also in kSTable,
cnf_sgpr.hip), four stacks at sigma 0.2:

  A  RealNVP, L=3            k_sgpr fn[2 nets][fwd, inv, loss, predict]
  B  RealNVP, L=4, flip      k_sgpr pfn[2 nets][fwd, inv, predict]
  C  NICE,    L=4            k_sgpr fn[1 net][fwd, inv, loss, predict]
  D  NICE,    L=3, flip      k_sgpr pfn[1 net][fwd, inv, predict]

each also with OPT_NO_SGPR (k_valu's `small` variant [fwd, inv][non-strict];
every-layer outputs always run there), stack A with strict_nan (k_valu
[.][strict]) and stack A past kLargeBatch rows (the `large` variant, strict
and not).  The three tanh rows of kLTable run through flows/legacy.py, small
and large variant.

Batches 1, 131 (one 128-row k_sgpr tile + 3 rows) and 517 (two 256-row tiles
+ 5 rows; past one 512-row block of k_valu's small variant).  The reference
is computed once per stack on 517 rows and sliced.

Bars: the project's 1e-5 under tests/_golden.rel_err against the float64
numpy oracle of the same weights and the same fp32 inputs; for the inverse
max(1e-5, 2 x the fp32 numpy oracle's own error against float64 on the same
case) (the rule tests/test_gpu_parity._check_inverse applies to g6_d10_h0);
loss sums within 1e-5 x the sum of the per-row magnitudes; predict within 1e-5
absolute of the float64 formula."""
import copy

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
BS = (1, 131, 517)
BMAX = max(BS)

# name -> (L, scale, flip)
STACKS = {"A": (3, True, False), "B": (4, True, True), "C": (4, False, False),
          "D": (3, False, True)}


class _Case:
    """One stack: the flow on the device, BMAX fp32 rows and the float64 /
    fp32 numpy-oracle results every check of the stack shares (never written
    after construction)."""

    def __init__(self, D, hidden, name, poison=False):
        L, scale, flip = STACKS[name]
        self.D, self.L, self.hidden, self.name = D, L, hidden, name
        x, y, prior = _sweep.inputs(BMAX, D, seed=1)
        x = x - x.mean(dim=1, keepdim=True)   # centred logits, as predict's input
        flow, self.seed, x = _sweep.conditioned_flow(D, L, hidden, x, scale, True, flip)
        if poison:
            x = torch.cat([x, _poison_rows(flow)])
        self.x, self.y, self.prior = x, y, prior
        self.l64 = _sweep.oracle_layers(flow, np.float64)
        self.l32 = _sweep.oracle_layers(flow, np.float32)
        xn = x.numpy()
        zs, ld = O.flow_forward(self.l64, xn.astype(np.float64))
        self.zs64, self.ld64 = np.stack(zs), np.asarray(ld)
        # the inverse's input: the float64 output rounded to fp32 (fixed, CPU)
        self.z32 = np.nan_to_num(self.zs64[-1], nan=0.0, posinf=0.0, neginf=0.0) \
            .astype(np.float32)
        xs, ild = O.flow_inverse(self.l64, self.z32.astype(np.float64))
        self.xs64, self.ild64 = np.stack(xs), np.asarray(ild)
        xs32, ild32 = O.flow_inverse(self.l32, self.z32)
        self.xs32, self.ild32 = np.stack(xs32), np.asarray(ild32)
        self.flow = flow.to(DEV)
        self.xg = x.to(DEV)
        self.yg = y.to(DEV)
        self.zg = torch.from_numpy(self.z32).to(DEV)

    def inv_bar(self, B):
        """max(1e-5, 2 x the fp32 oracle's own error) on these rows."""
        floor = max(rel_err(self.xs32[:, :B], self.xs64[:, :B]),
                    rel_err(self.ild32[:B], self.ild64[:B]))
        return max(TOL, 2 * floor), floor


_cases = {}


def _case(D, hidden, name):
    key = (D, tuple(hidden), name)
    if key not in _cases:
        _cases.clear()   # one stack alive at a time
        _cases[key] = _Case(D, hidden, name)
    return _cases[key]


def _np(t):
    return t.detach().cpu().numpy()


def _set_options(c, options, strict=None):
    c.flow.native_options = options
    c.flow.strict_nan = strict
    return c.flow._native_stack()


SHAPES = [(D, h) for D, h, _ in _sweep.NARROW]
CASES = [(D, h, s, o) for D, h in SHAPES for s in STACKS for o in ("fast", "valu")]
IDS = ["%s-%s-%s" % (_sweep.shape_id(D, h), s, o) for D, h, s, o in CASES]


def _stack_for(c, opt):
    no_sgpr = opt == "valu"
    stack = _set_options(c, _lib.OPT_NO_SGPR if no_sgpr else 0)
    want = _sweep.expected_kernel(c.D, c.hidden, no_sgpr=no_sgpr)
    assert stack.kernel_name() == want
    return stack, want


@pytest.mark.parametrize("D,hidden,name,opt", CASES, ids=IDS)
def test_forward_and_inverse_against_float64(D, hidden, name, opt):
    c = _case(D, hidden, name)
    stack, kernel = _stack_for(c, opt)
    worst_f = worst_i = worst_floor = 0.0
    for B in BS:
        x, zin = c.xg[:B], c.zg[:B]
        n0 = engine.stats["forward"] + engine.stats["inverse"]
        with torch.no_grad():
            z, ld = c.flow.transform(x)
            zs, ld_all = c.flow(x)
            xr, ild = c.flow.inverse_transform(zin)
            xs, ild_all = c.flow.backward(zin)
        assert engine.stats["forward"] + engine.stats["inverse"] == n0 + 4, "native path did not run"
        e = [rel_err(_np(z), c.zs64[-1, :B]), rel_err(_np(ld).reshape(-1), c.ld64[:B]),
             rel_err(_np(torch.stack(zs)), c.zs64[:, :B]),
             rel_err(_np(ld_all).reshape(-1), c.ld64[:B])]
        bar, floor = c.inv_bar(B)
        ei = [rel_err(_np(xr), c.xs64[-1, :B]), rel_err(_np(ild).reshape(-1), c.ild64[:B]),
              rel_err(_np(torch.stack(xs)), c.xs64[:, :B]),
              rel_err(_np(ild_all).reshape(-1), c.ild64[:B])]
        print("%s %s %s B=%d: fwd %s inv %s (fp32 oracle %.2e, bar %.2e)"
              % (_sweep.shape_id(D, hidden), name, kernel, B, e, ei, floor, bar))
        assert max(e) <= TOL, (B, e)
        assert max(ei) <= bar, (B, ei, bar)
        worst_f, worst_i, worst_floor = max(worst_f, *e), max(worst_i, *ei), max(worst_floor, floor)
    _sweep.record({"test": "forward", "D": D, "hidden": hidden, "stack": name, "kernel": kernel,
                   "fwd_err": worst_f, "inv_err": worst_i, "inv_fp32_oracle_err": worst_floor})


@pytest.mark.parametrize("D,hidden,name,opt", CASES, ids=IDS)
def test_loss_terms_and_predict_against_float64(D, hidden, name, opt):
    c = _case(D, hidden, name)
    stack, kernel = _stack_for(c, opt)
    z64, ld64 = torch.from_numpy(c.zs64[-1]), torch.from_numpy(c.ld64)
    p64 = _sweep.predict64(z64, c.prior).numpy()
    lp = torch.log(c.prior)
    worst_p = 0.0
    # k_sgpr has no permuted loss instantiation (cnf_sgpr.hip pick()): a
    # random_flip stack's fused eval runs on k_valu, so its z / ld are held
    # bitwise to k_valu's transform, every other stack's to its own
    via_valu = kernel == "sgpr-fused" and STACKS[name][2]
    for B in BS:
        x, y = c.xg[:B], c.yg[:B]
        with torch.no_grad():
            if via_valu:
                _set_options(c, _lib.OPT_NO_SGPR)
            z, ld = c.flow.transform(x)
            if via_valu:
                stack = _set_options(c, 0)
        assert rel_err(_np(z), c.zs64[-1, :B]) <= TOL
        for kind in (0, 1):
            rows = _sweep.loss_rows64(z64[:B], ld64[:B], c.y[:B], kind, 0.5).numpy()
            t, zo, ldo = stack.forward_loss(x, y, kind=kind, det=0.5, want_outputs=True)
            t2, _, _ = stack.forward_loss(x, y, kind=kind, det=0.5)
            assert torch.equal(t, t2), "two calls differ"
            assert torch.equal(zo, z) and torch.equal(ldo, ld.reshape(-1))
            got = t.double().cpu().numpy()
            err, bound = np.abs(got - rows.sum(axis=1)), 1e-5 * np.abs(rows).sum(axis=1)
            print("%s %s %s B=%d kind=%d: terms err %s bound %s"
                  % (_sweep.shape_id(D, hidden), name, kernel, B, kind, err, bound))
            assert np.all(err <= bound), (B, kind, got, rows.sum(axis=1), bound)
        n0 = engine.stats["predict"]
        probs = stack.predict(x, lp)
        if kernel == "sgpr-fused":
            assert engine.stats["predict"] == n0 + 1, "the fused predict launch did not run"
        ep = float(np.max(np.abs(_np(probs).astype(np.float64) - p64[:B])))
        print("%s %s %s B=%d: predict err %.2e" % (_sweep.shape_id(D, hidden), name, kernel, B, ep))
        assert ep <= TOL, (B, ep)
        worst_p = max(worst_p, ep)
    _sweep.record({"test": "loss_predict", "D": D, "hidden": hidden, "stack": name,
                   "kernel": kernel, "predict_err": worst_p})


def _same_nonfinite(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(np.isposinf(a), np.isposinf(b)) and \
        np.array_equal(np.isneginf(a), np.isneginf(b))


def _poison_rows(flow):
    """Four rows whose conditioning half (the last D - D//2 features) is
    +-scale x N(0,1) and whose transformed half holds exact zeros: exp(s)
    overflows there (inf, and inf x 0 = NaN).  The scale starts at 3e3 and
    grows until the fp32 and the float64 oracle agree on every non-finite
    entry (checked on the CPU; an input condition, not a result)."""
    D = flow.layers[0].dim
    l64, l32 = _sweep.oracle_layers(flow, np.float64), _sweep.oracle_layers(flow, np.float32)
    g = torch.Generator().manual_seed(9)
    base = torch.randn(4, D, generator=g)
    DT = D // 2
    scale = 3e3
    for _ in range(12):
        rows = base.clone()
        rows[:, DT:] *= scale
        rows[:, :DT] = 0.0
        rows[1::2, 0] = 1.0   # a non-zero transformed entry too: inf rather than NaN
        r = rows.numpy()
        zs64, ld64 = O.flow_forward(l64, r.astype(np.float64))
        zs32, ld32 = O.flow_forward(l32, r)
        bad = ~np.isfinite(np.stack(zs32))
        if bad.any() and _same_nonfinite(np.stack(zs32), np.stack(zs64)) and \
                _same_nonfinite(ld32, ld64):
            return rows
        scale *= 4
    raise AssertionError("no scale at which the fp32 and float64 oracles agree")


@pytest.mark.parametrize("D,hidden", SHAPES, ids=[_sweep.shape_id(D, h) for D, h in SHAPES])
def test_strict_nan_stack_a(D, hidden):
    """k_valu [fwd, inv][strict] (small variant): the finite rows at the usual
    bars; the poisoned rows' non-finite entries exactly where the fp32 numpy
    oracle has them."""
    _cases.clear()
    c = _Case(D, hidden, "A", poison=True)
    stack = _set_options(c, 0, strict=True)
    assert stack.kernel_name() == "valu-fused" and stack.strict_nan
    n = BMAX
    with torch.no_grad():
        z, ld = c.flow.transform(c.xg)
        zs, ld_all = c.flow(c.xg)
        xr, ild = c.flow.inverse_transform(c.zg[:n])
        xs, ild_all = c.flow.backward(c.zg[:n])
    e = [rel_err(_np(z)[:n], c.zs64[-1, :n]), rel_err(_np(ld)[:n], c.ld64[:n]),
         rel_err(_np(torch.stack(zs))[:, :n], c.zs64[:, :n]), rel_err(_np(ld_all)[:n], c.ld64[:n])]
    bar, floor = c.inv_bar(n)
    ei = [rel_err(_np(xr), c.xs64[-1, :n]), rel_err(_np(ild), c.ild64[:n]),
          rel_err(_np(torch.stack(xs)), c.xs64[:, :n]), rel_err(_np(ild_all), c.ild64[:n])]
    print("%s strict: fwd %s inv %s (bar %.2e)" % (_sweep.shape_id(D, hidden), e, ei, bar))
    assert max(e) <= TOL and max(ei) <= bar, (e, ei, bar)
    zs32, ld32 = O.flow_forward(c.l32, c.x.numpy()[n:])
    zs32 = np.stack(zs32)
    assert (~np.isfinite(zs32)).any()
    # rel_err is inf unless NaN and +-inf positions coincide; finite entries of
    # these rows (|x| ~ 1e4 and more through exp) are held to the positions only
    gz, gzs = _np(z)[n:], _np(torch.stack(zs))[:, n:]
    assert _same_nonfinite(gzs, zs32), (gzs, zs32)
    assert _same_nonfinite(gz, zs32[-1])
    assert _same_nonfinite(_np(ld)[n:], ld32) and _same_nonfinite(_np(ld_all)[n:], ld32)
    mask = lambda a: np.where(np.isfinite(a), 0.0, a)
    assert rel_err(mask(gzs), mask(zs32)) == 0.0
    _sweep.record({"test": "strict", "D": D, "hidden": hidden, "stack": "A",
                   "kernel": "valu-fused", "fwd_err": max(e), "inv_err": max(ei),
                   "inv_fp32_oracle_err": floor})


@pytest.mark.parametrize("strict", [False, True], ids=["fast", "strict"])
@pytest.mark.parametrize("D,hidden", SHAPES, ids=[_sweep.shape_id(D, h) for D, h in SHAPES])
def test_large_variant(D, hidden, strict):
    """k_valu's `large` variant [fwd, inv][strict?]: stack A with OPT_NO_SGPR at
    kLargeBatch + 259 rows, final outputs only.  Row i of the batch is row
    i mod 517 of the stack's base rows (517 is odd: no tile or block size
    divides the period), so the float64 reference of every row is known: the
    whole batch is compared on the device, and 2048 seeded sample rows plus
    the last 259 through rel_err; the round trip and ld + ild over the whole
    batch at twice the fp32 oracle's own residue on the base rows."""
    B = _sweep.LARGE_BATCH + 259
    c = _case(D, hidden, "A")
    stack = _set_options(c, _lib.OPT_NO_SGPR, strict=strict)
    assert stack.kernel_name() == "valu-fused" and stack.strict_nan == strict
    row = torch.arange(B, device=DEV) % BMAX
    x = c.xg[row]
    with torch.no_grad():
        z, ld = c.flow.transform(x)
        xr, ild = c.flow.inverse_transform(z)
    z64 = torch.from_numpy(c.zs64[-1]).to(DEV)[row]
    ld64 = torch.from_numpy(c.ld64).to(DEV)[row]
    assert torch.isfinite(z).all() and torch.isfinite(ld).all()
    whole = [((z.double() - z64).abs() / (z64.abs() + 1)).max().item(),
             ((ld.double() - ld64).abs() / (ld64.abs() + 1)).max().item()]
    del z64, ld64
    idx = torch.cat([torch.randperm(B, generator=torch.Generator().manual_seed(1))[:2048],
                     torch.arange(B - 259, B)]).to(DEV)
    base = _np(row[idx])
    ef = [rel_err(_np(z[idx]), c.zs64[-1, base]), rel_err(_np(ld[idx]), c.ld64[base])]
    # the inverse of the device's own z: float64 and fp32 oracle on the sample
    zi = _np(z[idx])
    xi64, ild64 = O.flow_inverse(c.l64, zi.astype(np.float64))
    xi32, ild32 = O.flow_inverse(c.l32, zi)
    floor = max(rel_err(xi32[-1], xi64[-1]), rel_err(ild32, ild64))
    bar = max(TOL, 2 * floor)
    ei = [rel_err(_np(xr[idx]), xi64[-1]), rel_err(_np(ild[idx]), ild64)]
    # the fp32 oracle's own round trip and ld + ild on the base rows
    xb = c.x.numpy()
    zo32, ldo32 = O.flow_forward(c.l32, xb)
    xo32, ildo32 = O.flow_inverse(c.l32, zo32[-1])
    rt_floor = rel_err(xo32[-1], xb)
    sym_floor = float(np.max(np.abs(ldo32 + ildo32) / (np.abs(ldo32) + 1)))
    rt_bar, sym_bar = max(TOL, 2 * rt_floor), max(TOL, 2 * sym_floor)
    rt = ((xr - x).abs() / (x.abs() + 1)).max().item()
    sym = ((ld + ild).abs() / (ld.abs() + 1)).max().item()
    print("%s large strict=%d: fwd whole %s sample %s inv %s (fp32 oracle %.2e) round trip %.2e "
          "(fp32 oracle %.2e) ld+ild %.2e (fp32 oracle %.2e)"
          % (_sweep.shape_id(D, hidden), strict, whole, ef, ei, floor, rt, rt_floor, sym,
             sym_floor))
    assert max(whole) <= TOL and max(ef) <= TOL, (whole, ef)
    assert max(ei) <= bar, (ei, bar)
    assert rt <= rt_bar and sym <= sym_bar, (rt, rt_bar, sym, sym_bar)
    _sweep.record({"test": "large", "D": D, "hidden": hidden, "stack": "A", "strict": strict,
                   "kernel": "valu-fused", "fwd_err": max(whole + ef), "inv_err": max(ei),
                   "round_trip": rt, "inv_fp32_oracle_err": floor})


@pytest.mark.parametrize("L", [3, 4])
@pytest.mark.parametrize("D,hidden", _sweep.TANH,
                         ids=[_sweep.shape_id(D, h) for D, h in _sweep.TANH])
def test_tanh_table_through_legacy_flow(D, hidden, L):
    """kLTable (tanh s-net, alternating mask): forward, inverse and every-layer
    outputs against flows/legacy.py's CPU path in float64, the `small` variant
    at 1, 131 and 517 rows and the `large` one past kLargeBatch.  (The strict
    instantiations of these rows are not launched: include/cnf.h declares the
    legacy options not combinable with strict_nan, and flows/legacy.py never
    sets it.)"""
    from flows.legacy import LegacyRealNvpFlow
    torch.manual_seed(0)
    f = LegacyRealNvpFlow(D, layers=L, hidden_size=hidden, s_activation="tanh")
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in f.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * _sweep.SIGMA)
    x, _, _ = _sweep.inputs(BMAX, D, seed=1)
    f64 = copy.deepcopy(f).double()
    with torch.no_grad():
        h, outs, ld64 = x.double(), [], torch.zeros(BMAX, dtype=torch.float64)
        for ly in f64.layers:
            h, l = ly(h)
            outs.append(h)
            ld64 = ld64 + l
        z32 = outs[-1].float()
        h, ins, ild64 = z32.double(), [], torch.zeros(BMAX, dtype=torch.float64)
        for ly in reversed(f64.layers):
            h, l = ly.backward(h)
            ins.append(h)
            ild64 = ild64 + l
        x32, ild32 = f.backward(z32)   # the fp32 CPU restatement's own error
    floor = max(rel_err(x32.numpy(), ins[-1].numpy()), rel_err(ild32.numpy(), ild64.numpy()))
    bar = max(TOL, 2 * floor)
    fg = f.to(DEV)
    stack = fg._native_stack()
    assert stack.kernel_name() == "valu-fused"
    # the `large` variant: row i of kLargeBatch + 259 rows is base row i mod 517
    # (test_large_variant's construction), the whole batch against float64
    row = torch.arange(_sweep.LARGE_BATCH + 259, device=DEV) % BMAX
    with torch.no_grad():
        yb, ldb = fg(x.to(DEV)[row])
        xbb, ildb = fg.backward(z32.to(DEV)[row])
    big = lambda got, ref: ((got.double() - ref.to(DEV)[row]).abs()
                            / (ref.to(DEV)[row].abs() + 1)).max().item()
    eb = [big(yb, outs[-1]), big(ldb, ld64)]
    eib = [big(xbb, ins[-1]), big(ildb, ild64)]
    print("tanh %s L=%d large: fwd %s inv %s (bar %.2e)" % (_sweep.shape_id(D, hidden), L, eb, eib, bar))
    assert torch.isfinite(yb).all() and torch.isfinite(xbb).all()
    assert max(eb) <= TOL and max(eib) <= bar, (eb, eib, bar)
    del yb, ldb, xbb, ildb
    for B in BS:
        xg, zg = x[:B].to(DEV), z32[:B].to(DEV)
        with torch.no_grad():
            y, ld = fg(xg)
            xb, ild = fg.backward(zg)
            _, lda, alls = stack.run(xg, want_all=True)
            _, ilda, ialls = stack.run(zg, inverse=True, want_all=True)
        e = [rel_err(_np(y), outs[-1][:B].numpy()), rel_err(_np(ld).reshape(-1), ld64[:B].numpy()),
             rel_err(_np(alls), torch.stack(outs)[:, :B].numpy()),
             rel_err(_np(lda).reshape(-1), ld64[:B].numpy())]
        ei = [rel_err(_np(xb), ins[-1][:B].numpy()),
              rel_err(_np(ild).reshape(-1), ild64[:B].numpy()),
              rel_err(_np(ialls), torch.stack(ins)[:, :B].numpy()),
              rel_err(_np(ilda).reshape(-1), ild64[:B].numpy())]
        print("tanh %s L=%d B=%d: fwd %s inv %s (bar %.2e)"
              % (_sweep.shape_id(D, hidden), L, B, e, ei, bar))
        assert max(e) <= TOL, (B, e)
        assert max(ei) <= bar, (B, ei, bar)
    _sweep.record({"test": "tanh", "D": D, "hidden": hidden, "L": L, "kernel": "valu-fused",
                   "fwd_err": max(e), "inv_err": max(ei), "inv_fp32_oracle_err": floor})
