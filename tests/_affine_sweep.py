"""The affine family's row-geometry sweep (tests/test_gpu_affine_sweep.py; the
plans also in tests/test_affine_cpu.py), in the discipline of tests/_rowsweep.py
whose constants, widths, depths, bars and admission rule it imports: every
geometry <lpr, cpl> of CNF_ROWFLOW_DISPATCH at a register-depth and a
checkpoint-depth stack, at a ragged multi-block batch and at one row, plus the
boundary shapes of csrc/cnf_affine.hip (ps = 2 D row sums per layer).

Admission.  The package's own fp32 torch-op CPU path must lie within a quarter
of each bar of the float64 restatement (tests/_affine_ref.py); it is decided on
the CPU from the references alone and moves the whole case to its next seed,
never a row.  The draw is damped with the depth -- x ~ 2 N, s ~ min(0.3, 1 / L)
N, t ~ min(0.5, 2 / L) N -- because an undamped s ~ 0.3 N at L = 64 grows the
rows until fp32 itself misses the quarter bar (1.7e-4 at D = 256).
"""
import numpy as np
import torch

import _affine_ref as A
import _rowsweep as S
from _golden import rel_err

DET = S.DET
BINS = S.BINS


class Case:
    def __init__(self, D, L, B, expect=None, why=""):
        self.family, self.D, self.L, self.B = "affine", D, L, B
        self.expect, self.why = dict(expect or {}), why
        self.id = "affine-d%d-l%d-b%d" % (D, L, B)

    def plan(self):
        p = A.expected_plan(self.D, self.L, self.B)
        for k, v in self.expect.items():
            assert p[k] == v, (self.id, k, p[k], v)
        return p

    def __repr__(self):
        return self.id


def _cases():
    rg = S.ragged
    out = [Case(D, L, B, why="main grid")
           for D in S.WIDTHS for L in S.DEPTHS for B in (rg(D), 1)]
    out += [
        Case(10, 10, rg(10), {"regt": 1, "rega": 1}, "full register depth, D = kAccD"),
        Case(11, 10, rg(11), {"regt": 1, "rega": 0}, "full register depth, D = kAccD + 1"),
        Case(12, 10, rg(12), {"regt": 1, "rega": 0}, "full register depth"),
        Case(10, 11, rg(10), {"regt": 0, "rega": 0}, "D = kAccD past the register depth"),
        Case(1, 64, rg(1), {"regt": 0, "gacc": 0}, "deepest stack, narrowest row"),
        Case(2, 64, rg(2), {"regt": 0, "gacc": 0}, "deepest stack, two columns"),
        Case(3, 64, rg(3), {"regt": 0, "gacc": 0}, "deepest stack, four full checkpoints"),
        Case(256, 64, 251, {"gacc": 1, "bwd_blocks": 31, "bwd_units": 124},
             "pw = 32772 caps the gacc grid at 31 blocks: three passes and a ragged row"),
        Case(23, 64, rg(23), {"gacc": 0}, "pw = 2948, deepest LDS record"),
        Case(24, 64, rg(24), {"gacc": 1}, "pw = 3076, gacc under checkpoints"),
        Case(153, 10, rg(153), {"gacc": 0, "regt": 1}, "pw = 3064, LDS record at 48 KB"),
        Case(154, 10, rg(154), {"gacc": 1, "regt": 1}, "pw = 3084, gacc with inputs in registers"),
        Case(17, 3, 16 * 1024 + 1, {"fwd_blocks": 1024, "bwd_blocks": 256},
             "one row past the forward cap, 16 lanes per row"),
        Case(65, 3, 4 * 1024 + 1, {"fwd_blocks": 1024, "bwd_blocks": 256},
             "one row past the forward cap, 64 lanes per row"),
        Case(65, 3, 4 * 37 + 1, {"bwd_blocks": 38, "bwd_units": 38},
             "38 records over 16 unit groups: chunk = 3, a partial and three empty groups"),
    ]
    return out


BY_ID = {}
for _c in _cases():      # a boundary shape that is also a main-grid cell keeps its literals
    BY_ID[_c.id] = _c
CASES = list(BY_ID.values())
IDS = [c.id for c in CASES]


def draw(case, attempt):
    D, L, B = case.D, case.L, case.B
    rs = np.random.RandomState([2, D, L, B, attempt])
    x = (2.0 * rs.standard_normal((B, D))).astype(np.float32)
    y = rs.randint(0, D, size=B).astype(np.int64)
    d = A.draw_params(rs, D, L)
    gz_all = rs.standard_normal((L, B, D)).astype(np.float32)
    gld = rs.standard_normal(1).astype(np.float32)
    return x, y, d, gz_all, gld


def _references(case, x, y, d, gz_all, gld):
    """Everything the GPU is compared with, float64."""
    B = case.B
    params = A.params_of(d)
    r = {}
    r["zs"], ld = A.forward(params, x)
    r["ld"] = np.array([ld])
    r["xs"], ild = A.inverse(params, r["zs"][-1])
    r["ild"] = np.array([ild])
    r["rt"] = x.astype(np.float64)          # inverse(forward(x))
    r["probs"] = A.predict(params, x, S.log_priors(case.D))
    for kind, det in (("cal", 1.0), ("ce", DET)):
        r["terms_" + kind], r["g_" + kind], r["dx_" + kind] = \
            A.loss_vjp(params, x, y, kind, det, 1.0 / B)
    r["g_all"], r["dx_all"] = A.vjp(params, x, gz_all=gz_all, gld=gld)
    r["g_fin"], r["dx_fin"] = A.vjp(params, x, gz=gz_all[-1])
    return r


def _flat(grads):
    return torch.cat([g.reshape(-1) for g in grads]).numpy()


def _fp32_cpu(case, x, y, d, gz_all, gld, ref):
    """The same quantities from the package's torch-op CPU path in fp32.  The
    inverse starts from the float64 reference's z rounded to fp32, as the GPU
    test's does, so it is judged on its own."""
    B = case.B
    flow = A.build_flow(d)
    ps_ = list(flow.parameters())
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    lp = torch.from_numpy(S.log_priors(case.D)).float()
    o = {}
    with torch.no_grad():
        zs, ld = flow(xt)
        o["zs"], o["ld"] = torch.stack(zs).numpy(), ld.numpy()
        xs, ild = flow.backward(torch.from_numpy(ref["zs"][-1].astype(np.float32)))
        o["xs"], o["ild"] = torch.stack(xs).numpy(), ild.numpy()
        o["rt"] = flow.inverse_transform(zs[-1])[0].numpy()
        z, _ = flow.transform(xt - xt.mean(dim=1, keepdim=True))
        q = torch.log(torch.softmax(z, dim=1) + 1e-7) - lp
        o["probs"] = torch.softmax(q, dim=1).numpy()

    def grads(objective):
        xg = xt.clone().requires_grad_(True)
        res = torch.autograd.grad(objective(xg), ps_ + [xg], allow_unused=True)
        res = [torch.zeros_like(t) if g is None else g for g, t in zip(res, ps_ + [xg])]
        return _flat(res[:-1]), res[-1].numpy()

    def loss(kind, det):
        def f(xg):
            z, ld = flow.transform(xg)
            if kind == "cal":
                ce = -torch.log(torch.softmax(z, dim=1).gather(1, yt.view(-1, 1)).squeeze(1) + 1e-7)
            else:
                ce = -torch.log_softmax(z, dim=1).gather(1, yt.view(-1, 1)).squeeze(1)
            return torch.sum(ce - det * ld) / B
        return f

    def generic(xg):
        zs, ld = flow(xg)
        return (torch.stack(zs) * torch.from_numpy(gz_all)).sum() + (ld * torch.from_numpy(gld)).sum()

    o["g_cal"], o["dx_cal"] = grads(loss("cal", 1.0))
    o["g_ce"], o["dx_ce"] = grads(loss("ce", DET))
    o["g_all"], o["dx_all"] = grads(generic)
    o["g_fin"], o["dx_fin"] = grads(
        lambda xg: (flow.transform(xg)[0] * torch.from_numpy(gz_all[-1])).sum())
    return o


OUT_KEYS = ("zs", "ld", "xs", "ild", "rt", "probs")
GRAD_KEYS = S.GRAD_KEYS

_prepared = {}


def prepare(case):
    """The admitted case (cached for the session): the first of S.MAX_SEEDS
    seed attempts at which the fp32 CPU path is within S.OUT_COND (outputs,
    log-dets, predict) and S.GRAD_COND (every gradient) of the float64
    restatement."""
    if case.id in _prepared:
        return _prepared[case.id]
    tried = []
    for attempt in range(S.MAX_SEEDS):
        inputs = draw(case, attempt)
        ref = _references(case, *inputs)
        cpu = _fp32_cpu(case, *inputs, ref)
        fo = max(rel_err(cpu[k], ref[k]) for k in OUT_KEYS)
        fg = max(S.grad_err(cpu[k], ref[k]) for k in GRAD_KEYS)
        tried.append((fo, fg))
        if fo <= S.OUT_COND and fg <= S.GRAD_COND:
            p = S.Prepared()
            p.floor_probs_d = S.probs_err(cpu["probs"], ref["probs"])
            p.probs_bar = max(S.OUT_BAR, 2.0 * p.floor_probs_d)
            p.case, p.attempt, p.floor_out, p.floor_grad, p.ref = case, attempt, fo, fg, ref
            p.x, p.y, p.d, p.gz_all, p.gld = inputs
            p.lp = S.log_priors(case.D)
            _prepared[case.id] = p
            return p
    raise AssertionError("no admissible seed for %s: %r" % (case.id, tried))
