"""Shared helper of the row-geometry sweeps (tests/test_rowflow_sync_cpu.py,
test_gpu_rowflow_forward.py, test_gpu_rowflow_vjp.py): the case list of the
planar and radial families (csrc/cnf_planar.hip, cnf_radial.hip, the shared
host code of cnf_rowflow.h), the launch plan each case must take, seeded
inputs, their float64 references and the admission rule.

The families pick their kernels by shape: CNF_ROWFLOW_DISPATCH instantiates
forward, predict, score and reverse mode for 22 row geometries <lpr, cpl>, and
launch_bwd splits the reverse mode by (regt, rega); the wave records move from
LDS to the workspace (gacc) past LDS_WORDS.  WIDTHS holds every geometry, both
ends of each multi-lane one; CASES runs each at a register-tape and a
workspace-tape depth, and adds the boundary shapes.  The constants restate
cnf_rowflow.h / cnf_planar.hip; tests/test_rowflow_sync_cpu.py parses the
sources and fails when they and this list disagree.

Admission.  A case can tell a wrong kernel from rounding only while plain fp32
arithmetic leaves most of the bar unused, so the package's own fp32 torch-op
CPU path must lie within a quarter of each bar of the float64 restatement.  It
is decided on the CPU from the references alone and moves the whole case to its
next seed, never a row.
"""
import numpy as np
import torch

import _planar_predict_ref as PR
import _planar_ref as R
import _radial_ref as RR
from _golden import rel_err

REG_L = 10          # kRegL: tape in registers up to this depth
ACC_D = 11          # kAccD (cnf_planar.hip): per-lane accumulators up to this width
LDS_WORDS = 3072    # kLdsWords: a wave's record in LDS up to this many floats
FWD_CAP = 1024      # kFwdCap, kBwdCap: grid caps in blocks
BWD_CAP = 256
THREADS = 256       # kThreads; kWaves = THREADS / 64
WAVES = 4
FIN_GROUPS = 16     # k_*_finish: kFinThreads / 64 unit groups once pw >= 64

FAMILIES = ("planar", "radial")
WIDTHS = list(range(1, 17)) + [17, 32, 33, 48, 49, 64, 65, 128, 129, 192, 193, 256]
DEPTHS = (3, 11)    # REGT, !REGT
DET = 0.7           # the CE loss's log-det weight (planar)
BINS = 15

OUT_BAR, GRAD_BAR = 1e-5, 1e-4
OUT_COND, GRAD_COND = OUT_BAR / 4, GRAD_BAR / 4
MAX_SEEDS = 20


def grad_err(got, ref):
    from test_gpu_vjp import _grad_err
    return _grad_err(got, ref)


# ---- the launch plan, restated ------------------------------------------------

def lanes(D):
    return 1 if D <= 16 else 16 if D <= 64 else 64


def geometry(D):
    lpr = lanes(D)
    return lpr, -(-D // lpr)


GEOMETRIES = sorted({geometry(D) for D in WIDTHS})


def rows_per_block(D):
    return THREADS // lanes(D)


def ps(family, D):
    return 2 * D + 2 if family == "planar" else D + 2


def pw(family, D, L):
    return L * ps(family, D) + 4


def variant(family, D, L):
    """(regt, rega) of launch_bwd."""
    lpr, cpl = geometry(D)
    regt = L <= REG_L
    rega = regt and lpr == 1 and (cpl <= ACC_D if family == "planar" else True)
    return regt, rega


def expected_plan(family, D, L, B):
    """cnf_<family>_launch_plan, restated from the constants above."""
    lpr, cpl = geometry(D)
    regt, rega = variant(family, D, L)
    w = pw(family, D, L)
    gacc = w > LDS_WORDS
    n = max(1, -(-B // (THREADS // lpr)))
    cap = max(4, min(BWD_CAP, (1 << 20) // w)) if gacc else BWD_CAP
    bwd = min(n, cap)
    return {"lpr": lpr, "cpl": cpl, "regt": int(regt), "rega": int(rega), "gacc": int(gacc),
            "fwd_blocks": min(n, FWD_CAP), "bwd_blocks": bwd,
            "bwd_units": bwd * (WAVES if gacc else 1)}


def _r64(n):
    return (n + 63) // 64 * 64


def workspace_floats(family, D, L, B):
    """The workspace formula of include/cnf.h from the restated plan."""
    p = expected_plan(family, D, L, B)
    dp = p["lpr"] * p["cpl"]
    cs = (2 * dp if family == "planar" else dp) + 8
    w = pw(family, D, L)
    tape = _r64(L * B) if L > REG_L else 0
    return _r64(L * cs) + _r64(w) + _r64(max(p["bwd_units"] * w, 4 * p["fwd_blocks"])) + tape


def finish_chunk(units):
    """k_*_finish: units per unit group (pw >= 64 in every case here)."""
    return -(-units // FIN_GROUPS)


# ---- the cases ------------------------------------------------------------------

class Case:
    """One (family, D, L, B).  `expect`: the plan fields the case is about, as
    literals on top of expected_plan(); `why`: what it exercises."""

    def __init__(self, family, D, L, B, expect=None, why=""):
        self.family, self.D, self.L, self.B = family, D, L, B
        self.expect, self.why = dict(expect or {}), why
        self.id = "%s-d%d-l%d-b%d" % (family, D, L, B)

    def plan(self):
        p = expected_plan(self.family, self.D, self.L, self.B)
        for k, v in self.expect.items():
            assert p[k] == v, (self.id, k, p[k], v)
        return p

    def __repr__(self):
        return self.id


def ragged(D):
    """More than one block and a ragged last one: 515, 35 or 11 rows."""
    return 2 * rows_per_block(D) + 3


def _cases():
    out = []
    for fam in FAMILIES:
        for D in WIDTHS:
            for L in DEPTHS:
                for B in (ragged(D), 1):
                    out.append(Case(fam, D, L, B, why="main grid"))
    for fam in FAMILIES:
        acc = fam == "planar"
        out += [
            Case(fam, 11, 10, ragged(11), {"regt": 1, "rega": 1}, "full register depth, D = kAccD"),
            Case(fam, 12, 10, ragged(12), {"regt": 1, "rega": 0 if acc else 1},
                 "full register depth, D = kAccD + 1"),
            Case(fam, 3, 64, ragged(3), {"regt": 0, "gacc": 0},
                 "deepest tape, full pointer table, one lane per row"),
            # the narrowest rows contract most under 64 radial layers: the reverse
            # mode's rebuilt inputs are the worst conditioned here
            Case(fam, 1, 64, ragged(1), {"regt": 0, "gacc": 0}, "deepest stack, narrowest row"),
            Case(fam, 2, 64, ragged(2), {"regt": 0, "gacc": 0}, "deepest stack, two columns"),
        ]
    lds = {"gacc": 0}
    ws = {"gacc": 1}
    out += [
        Case("planar", 22, 64, ragged(22), lds, "pw = 2948, deepest LDS record"),
        Case("planar", 23, 64, ragged(23), ws, "pw = 3076, gacc with the tape in the workspace"),
        Case("planar", 152, 10, ragged(152), dict(lds, regt=1), "pw = 3064, LDS record at 48 KB"),
        Case("planar", 153, 10, ragged(153), dict(ws, regt=1),
             "pw = 3084, gacc with the tape in registers"),
        Case("radial", 45, 64, ragged(45), lds, "pw = 3012"),
        Case("radial", 46, 64, ragged(46), ws, "pw = 3076"),
        Case("radial", 256, 11, ragged(256), lds, "pw = 2842"),
        Case("radial", 256, 12, ragged(256), ws, "pw = 3100"),
        Case("planar", 256, 64, 251, {"gacc": 1, "bwd_blocks": 31, "bwd_units": 124},
             "pw = 32900 caps the gacc grid at 31 blocks: two passes and a ragged row; "
             "finish chunk = 8"),
        Case("radial", 256, 64, 251, {"gacc": 1, "bwd_blocks": 63, "bwd_units": 252},
             "pw = 16516: 63 blocks of the 63-block gacc cap, 252 units, finish chunk = 16"),
    ]
    for fam in FAMILIES:
        out += [
            Case(fam, 17, 3, 16 * 1024 + 1, {"fwd_blocks": 1024, "bwd_blocks": 256},
                 "one row past the forward cap, 16 lanes per row"),
            Case(fam, 65, 3, 4 * 1024 + 1, {"fwd_blocks": 1024, "bwd_blocks": 256},
                 "one row past the forward cap, 64 lanes per row"),
            Case(fam, 65, 3, 4 * 37 + 1, {"bwd_blocks": 38, "bwd_units": 38},
                 "38 records over 16 unit groups: chunk = 3, a partial and three empty groups"),
        ]
    return out


MAIN = [c for c in _cases() if c.why == "main grid"]
BY_ID = {}
for _c in _cases():      # a boundary shape that is also a main-grid cell keeps its literals
    BY_ID[_c.id] = _c
CASES = list(BY_ID.values())
IDS = [c.id for c in CASES]

# one case per reverse-mode variant and record placement (the bounds tests)
BOUNDS = ["planar-d3-l3-b515", "radial-d3-l3-b515", "planar-d14-l3-b515",
          "planar-d33-l11-b35", "radial-d33-l11-b35", "planar-d129-l11-b11",
          "radial-d129-l11-b11", "planar-d23-l64-b35", "planar-d153-l10-b11",
          "radial-d46-l64-b35", "radial-d256-l12-b11"]


def variant_name(plan):
    return "rega" if plan["rega"] else "regt" if plan["regt"] else "tape"


# ---- inputs and references ---------------------------------------------------------

def log_priors(D):
    return np.log(np.arange(1, D + 1) / (D * (D + 1) / 2.0))


def draw(case, attempt):
    """The case's seeded inputs: rows, labels, parameters (the fixture dict of
    _planar_ref / _radial_ref .build_flow), upstream weights."""
    fam, D, L, B = case.family, case.D, case.L, case.B
    rs = np.random.RandomState([FAMILIES.index(fam), D, L, B, attempt])
    x = (2.0 * rs.standard_normal((B, D))).astype(np.float32)
    y = rs.randint(0, D, size=B).astype(np.int64)
    if fam == "planar":
        # w.u_hat grows like sqrt(D) at a fixed scale and 1 + h' w.u_hat then
        # comes close to 0, where fp32 itself loses the log-det: scale by 1 / sqrt(D)
        s = min(0.5, 1.0 / np.sqrt(D))
        d = {"W": (s * rs.standard_normal((L, D))).astype(np.float32),
             "U": (s * rs.standard_normal((L, D))).astype(np.float32),
             "Bv": (0.5 * rs.standard_normal(L)).astype(np.float32)}
    else:
        d = {"Z0": (0.5 * rs.standard_normal((L, D))).astype(np.float32),
             "A": np.abs(1.0 + 0.5 * rs.standard_normal(L)).astype(np.float32),
             "Bv": (0.5 * rs.standard_normal(L)).astype(np.float32)}
    gz_all = rs.standard_normal((L, B, D)).astype(np.float32)
    gld = rs.standard_normal(B).astype(np.float32)
    return x, y, d, gz_all, gld


def ref_module(family):
    return R if family == "planar" else RR


class Prepared:
    """An admitted case: inputs, float64 references, the fp32 CPU path's own
    error (floor_out, floor_grad) and the seed attempt it was admitted at."""


def _references(case, x, y, d, gz_all, gld):
    """Everything the GPU is compared with, float64."""
    fam, B = case.family, case.B
    M = ref_module(fam)
    params = M.params_of(d)
    lp = log_priors(case.D)
    r = {}
    if fam == "planar":
        r["zs"], r["ld"], _ = R.forward(params, x)
        r["probs"], _ = PR.predict(params, x, lp)
        for kind, det in (("cal", 1.0), ("ce", DET)):
            r["terms_" + kind], r["g_" + kind], r["dx_" + kind] = \
                R.loss_vjp(params, x, y, kind, det, 1.0 / B)
        r["g_all"], r["dx_all"] = R.vjp(params, x, gz_all=gz_all, gld=gld)
        r["g_fin"], r["dx_fin"] = R.vjp(params, x, gz=gz_all[-1])
    else:
        r["zs"], _ = RR.forward(params, x)
        r["ld"] = np.zeros(B)
        r["probs"] = RR.predict(params, x, lp)
        for kind in ("cal", "ce"):
            r["terms_" + kind], r["g_" + kind], r["dx_" + kind] = \
                RR.loss_vjp(params, x, y, kind, 1.0 / B)
        r["g_all"], r["dx_all"] = RR.vjp(params, x, gz_all=gz_all)
        r["g_fin"], r["dx_fin"] = RR.vjp(params, x, gz=gz_all[-1])
    return r


def _flat(grads):
    return torch.cat([g.reshape(-1) for g in grads]).numpy()


def _fp32_cpu(case, x, y, d, gz_all, gld):
    """The same quantities from the package's torch-op CPU path in fp32."""
    fam, B = case.family, case.B
    flow = ref_module(fam).build_flow(d)
    ps_ = list(flow.parameters())
    xt = torch.from_numpy(x)
    yt = torch.from_numpy(y)
    lp = torch.from_numpy(log_priors(case.D)).float()
    o = {}
    with torch.no_grad():
        zs, ld = flow(xt)
        o["zs"] = torch.stack(zs).numpy()
        o["ld"] = (ld * torch.ones(B)).reshape(-1).numpy()
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
        obj = (torch.stack(zs) * torch.from_numpy(gz_all)).sum()
        return obj + (ld * torch.from_numpy(gld)).sum() if fam == "planar" else obj

    o["g_cal"], o["dx_cal"] = grads(loss("cal", 1.0))
    o["g_ce"], o["dx_ce"] = grads(loss("ce", DET))
    o["g_all"], o["dx_all"] = grads(generic)
    o["g_fin"], o["dx_fin"] = grads(
        lambda xg: (flow.transform(xg)[0] * torch.from_numpy(gz_all[-1])).sum())
    return o


OUT_KEYS = ("zs", "ld", "probs")
GRAD_KEYS = ("g_cal", "dx_cal", "g_ce", "dx_ce", "g_all", "dx_all", "g_fin", "dx_fin")


def probs_err(got, ref):
    """The probabilities in units of the uniform one, D * p, under rel_err.
    rel_err's |b| + 1 makes the plain comparison absolute for values far below
    1: one term too many in a D-wide softmax moves p ~ 1 / D by ~ 1 / D^2,
    under the 1e-5 bar from D = 65 on (tried: the predict kernels' last sum
    over one padding column passed the plain comparison at every D >= 65).
    Scaled, the same defect is ~ 1 / (2 D).  D * p reaches D, so fp32's own
    error grows with the width (4e-6 at D = 256, L = 64): this figure is no
    part of the admission and is held to the project's rule, max(1e-5, twice
    the fp32 CPU path's own error) -- Prepared.probs_bar."""
    D = np.asarray(ref).shape[-1]
    return rel_err(np.asarray(got, dtype=np.float64) * D, np.asarray(ref, dtype=np.float64) * D)


def floors(ref, got):
    fo = max(rel_err(got[k], ref[k]) for k in OUT_KEYS)
    fg = max(grad_err(got[k], ref[k]) for k in GRAD_KEYS)
    return fo, fg


_prepared = {}


def prepare(case):
    """The admitted case (cached for the session): the first of MAX_SEEDS seed
    attempts at which the fp32 CPU path is within OUT_COND (outputs, log-det,
    predict; _golden.rel_err) and GRAD_COND (every gradient; _grad_err) of the
    float64 restatement."""
    if case.id in _prepared:
        return _prepared[case.id]
    tried = []
    for attempt in range(MAX_SEEDS):
        inputs = draw(case, attempt)
        ref = _references(case, *inputs)
        cpu = _fp32_cpu(case, *inputs)
        fo, fg = floors(ref, cpu)
        tried.append((fo, fg))
        if fo <= OUT_COND and fg <= GRAD_COND:
            p = Prepared()
            p.floor_probs_d = probs_err(cpu["probs"], ref["probs"])
            p.probs_bar = max(OUT_BAR, 2.0 * p.floor_probs_d)
            p.case, p.attempt, p.floor_out, p.floor_grad, p.ref = case, attempt, fo, fg, ref
            p.x, p.y, p.d, p.gz_all, p.gld = inputs
            p.lp = log_priors(case.D)
            _prepared[case.id] = p
            return p
    raise AssertionError("no admissible seed for %s: %r" % (case.id, tried))


def build_flow(p, device):
    return ref_module(p.case.family).build_flow(p.d, device)


# ---- records --------------------------------------------------------------------------

_rows = {}


def record(case, **fields):
    """One row per case in conftest.RECORDS["rowflow_sweep"], filled by both
    GPU files."""
    import conftest
    row = _rows.get(case.id)
    if row is None:
        plan = case.plan()
        row = _rows[case.id] = {"case": case.id, "family": case.family, "D": case.D, "L": case.L,
                                "B": case.B, "lpr": plan["lpr"], "cpl": plan["cpl"],
                                "bwd": variant_name(plan), "gacc": plan["gacc"]}
        conftest.RECORDS.setdefault("rowflow_sweep", []).append(row)
    row.update(fields)
    return row
