"""The mixed family's row-geometry sweep (tests/test_gpu_mixed_sweep.py; the
plans also in tests/test_mixed_sync_cpu.py), in the discipline of
tests/_rowsweep.py whose constants, widths, bars and admission rule it
imports: every geometry <lpr, cpl> of CNF_ROWFLOW_DISPATCH at a register-depth
and a checkpoint-depth stack, at a ragged multi-block batch and at one row,
plus the shapes on each side of every switch csrc/cnf_mixed.hip has: register
resident / checkpointed (L = 10 | 11, and D = 10 | 11 for a one-lane row), one
checkpoint segment / two (L = 16 | 17) up to four (L = 64), wave records in LDS
/ in the workspace (pw = L (2 D + 2) + 4 on each side of kLdsWords).

The layers are cyclic P, R, A from a planar first layer.  The cases call the
stack directly (the ABI takes any order at any batch); the flow's own dispatch
rule is tests/test_mixed_cpu.py's and tests/test_gpu_mixed.py's.

Admission.  The package's own fp32 torch-op CPU path -- its layers applied one
after another, the log-det summed out of place, since the loop's in-place sum
rejects this order at one row -- must lie within a quarter of each bar of the
float64 restatement (tests/_mixed_ref.py); it is decided on the CPU from the
references alone and moves the whole case to its next seed, never a row.
"""
import numpy as np
import torch

import _mixed_ref as M
import _rowsweep as S
from _golden import rel_err

DET = S.DET
BINS = S.BINS


def order(L):
    return ("PRA" * (L // 3 + 1))[:L]


class Case:
    def __init__(self, D, L, B, expect=None, why=""):
        self.family, self.D, self.L, self.B = "mixed", D, L, B
        self.expect, self.why = dict(expect or {}), why
        self.order = order(L)
        self.kinds = [M.KIND[c] for c in self.order]
        self.id = "mixed-d%d-l%d-b%d" % (D, L, B)

    def plan(self):
        p = M.expected_plan(self.D, self.L, self.B)
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
        Case(10, 11, rg(10), {"regt": 0, "rega": 0}, "D = kAccD past the register depth"),
        Case(11, 10, rg(11), {"regt": 0, "rega": 0},
             "D = kAccD + 1: a one-lane row that wide is checkpointed at every depth"),
        Case(17, 10, rg(17), {"regt": 1, "rega": 0}, "full register depth, 16 lanes per row"),
        Case(65, 10, rg(65), {"regt": 1, "rega": 0}, "full register depth, 64 lanes per row"),
        Case(3, 16, rg(3), {"regt": 0, "gacc": 0}, "one full checkpoint segment"),
        Case(3, 17, rg(3), {"regt": 0, "gacc": 0}, "one layer into the second segment"),
        Case(33, 17, rg(33), {"regt": 0, "gacc": 0}, "two segments, 16 lanes per row"),
        Case(1, 64, rg(1), {"regt": 0, "gacc": 0}, "deepest stack, narrowest row"),
        Case(3, 64, rg(3), {"regt": 0, "gacc": 0}, "deepest stack, four full segments"),
        Case(22, 64, rg(22), {"gacc": 0}, "pw = 2948, deepest LDS record"),
        Case(23, 64, rg(23), {"gacc": 1}, "pw = 3076, workspace records under checkpoints"),
        Case(152, 10, rg(152), {"gacc": 0, "regt": 1}, "pw = 3064, LDS record at 48 KB"),
        Case(153, 10, rg(153), {"gacc": 1, "regt": 1},
             "pw = 3084, workspace records with inputs in registers"),
        Case(256, 64, 251, {"gacc": 1, "bwd_blocks": 31, "bwd_units": 124},
             "pw = 32900 caps the gacc grid at 31 blocks: passes and a ragged row"),
        Case(17, 3, 16 * 1024 + 1, {"fwd_blocks": 1024, "bwd_blocks": 256},
             "one row past the forward cap, 16 lanes per row"),
        Case(65, 3, 4 * 1024 + 1, {"fwd_blocks": 1024, "bwd_blocks": 256},
             "one row past the forward cap, 64 lanes per row"),
        Case(65, 3, 4 * 37 + 1, {"bwd_blocks": 38, "bwd_units": 38},
             "38 records over 16 unit groups: chunk = 3, a partial and three empty groups"),
    ]
    return out


MAIN = [c for c in _cases() if c.why == "main grid"]
BY_ID = {}
for _c in _cases():      # a boundary shape that is also a main-grid cell keeps its literals
    BY_ID[_c.id] = _c
CASES = list(BY_ID.values())
IDS = [c.id for c in CASES]
# the pairs on each side of kLdsWords
BOUNDARY_PAIRS = [("mixed-d22-l64-b35", "mixed-d23-l64-b35", 2948, 3076),
                  ("mixed-d152-l10-b11", "mixed-d153-l10-b11", 3064, 3084)]


def variant_name(plan):
    return "rega" if plan["rega"] else "regt" if plan["regt"] else "ckpt"


def draw(case, attempt):
    D, L, B = case.D, case.L, case.B
    rs = np.random.RandomState([3, D, L, B, attempt])
    x = (2.0 * rs.standard_normal((B, D))).astype(np.float32)
    y = rs.randint(0, D, size=B).astype(np.int64)
    ps = M.draw_params(rs, D, case.order)
    gz_all = rs.standard_normal((L, B, D)).astype(np.float32)
    gld = rs.standard_normal(B).astype(np.float32)
    return x, y, ps, gz_all, gld


def _references(case, x, y, ps, gz_all, gld):
    """Everything the GPU is compared with, float64."""
    B = case.B
    r = {}
    r["zs"], r["ld"] = M.forward(ps, x)
    r["probs"] = M.predict(ps, x, S.log_priors(case.D))
    for kind, det in (("cal", 1.0), ("ce", DET)):
        r["terms_" + kind], r["g_" + kind], r["dx_" + kind] = \
            M.loss_vjp(ps, x, y, kind, det, 1.0 / B)
    r["g_all"], r["dx_all"] = M.vjp(ps, x, gz_all=gz_all, gld=gld)
    r["g_fin"], r["dx_fin"] = M.vjp(ps, x, gz=gz_all[-1])
    return r


def _flat(grads):
    return torch.cat([g.reshape(-1) for g in grads]).numpy()


def cpu_forward(flow, x):
    """(zs list, per-row log-det [B]) of the package's layers on the CPU, one
    after another, the log-det summed out of place."""
    B = x.shape[0]
    zs, ld = [], torch.zeros(B, dtype=x.dtype)
    for ly in flow.layers:
        x, l = ly(x)
        zs.append(x)
        ld = ld + l.reshape(-1) * torch.ones(B, dtype=x.dtype)
    return zs, ld


def _fp32_cpu(case, x, y, ps, gz_all, gld):
    """The same quantities from the package's torch-op CPU path in fp32."""
    B = case.B
    flow = M.build_flow(ps)
    ps_ = list(flow.parameters())
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    lp = torch.from_numpy(S.log_priors(case.D)).float()
    o = {}
    with torch.no_grad():
        zs, ld = cpu_forward(flow, xt)
        o["zs"], o["ld"] = torch.stack(zs).numpy(), ld.numpy()
        zc, _ = cpu_forward(flow, xt - xt.mean(dim=1, keepdim=True))
        q = torch.log(torch.softmax(zc[-1], dim=1) + 1e-7) - lp
        o["probs"] = torch.softmax(q, dim=1).numpy()

    def grads(objective):
        xg = xt.clone().requires_grad_(True)
        res = torch.autograd.grad(objective(xg), ps_ + [xg], allow_unused=True)
        res = [torch.zeros_like(t) if g is None else g for g, t in zip(res, ps_ + [xg])]
        return _flat(res[:-1]), res[-1].numpy()

    def loss(kind, det):
        def f(xg):
            zs, ld = cpu_forward(flow, xg)
            z = zs[-1]
            if kind == "cal":
                ce = -torch.log(torch.softmax(z, dim=1).gather(1, yt.view(-1, 1)).squeeze(1) + 1e-7)
            else:
                ce = -torch.log_softmax(z, dim=1).gather(1, yt.view(-1, 1)).squeeze(1)
            return torch.sum(ce - det * ld) / B
        return f

    def generic(xg):
        zs, ld = cpu_forward(flow, xg)
        return (torch.stack(zs) * torch.from_numpy(gz_all)).sum() + (ld * torch.from_numpy(gld)).sum()

    o["g_cal"], o["dx_cal"] = grads(loss("cal", 1.0))
    o["g_ce"], o["dx_ce"] = grads(loss("ce", DET))
    o["g_all"], o["dx_all"] = grads(generic)
    o["g_fin"], o["dx_fin"] = grads(
        lambda xg: (cpu_forward(flow, xg)[0][-1] * torch.from_numpy(gz_all[-1])).sum())
    return o


OUT_KEYS = S.OUT_KEYS
GRAD_KEYS = S.GRAD_KEYS

_prepared = {}


def prepare(case):
    """The admitted case (cached for the session): the first of S.MAX_SEEDS
    seed attempts at which the fp32 CPU path is within S.OUT_COND (outputs,
    log-det, predict) and S.GRAD_COND (every gradient) of the float64
    restatement."""
    if case.id in _prepared:
        return _prepared[case.id]
    tried = []
    for attempt in range(S.MAX_SEEDS):
        inputs = draw(case, attempt)
        ref = _references(case, *inputs)
        cpu = _fp32_cpu(case, *inputs)
        fo = max(rel_err(cpu[k], ref[k]) for k in OUT_KEYS)
        fg = max(S.grad_err(cpu[k], ref[k]) for k in GRAD_KEYS)
        tried.append((fo, fg))
        if fo <= S.OUT_COND and fg <= S.GRAD_COND:
            p = S.Prepared()
            p.floor_probs_d = S.probs_err(cpu["probs"], ref["probs"])
            p.probs_bar = max(S.OUT_BAR, 2.0 * p.floor_probs_d)
            p.case, p.attempt, p.floor_out, p.floor_grad, p.ref = case, attempt, fo, fg, ref
            p.x, p.y, p.ps, p.gz_all, p.gld = inputs
            p.lp = S.log_priors(case.D)
            _prepared[case.id] = p
            return p
    raise AssertionError("no admissible seed for %s: %r" % (case.id, tried))


_rows = {}


def record(case, **fields):
    """One row per case in conftest.RECORDS["mixed_sweep"]."""
    import conftest
    row = _rows.get(case.id)
    if row is None:
        plan = case.plan()
        row = _rows[case.id] = {"case": case.id, "D": case.D, "L": case.L, "B": case.B,
                                "lpr": plan["lpr"], "cpl": plan["cpl"], "bwd": variant_name(plan),
                                "gacc": plan["gacc"]}
        conftest.RECORDS.setdefault("mixed_sweep", []).append(row)
    row.update(fields)
    return row
