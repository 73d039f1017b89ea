"""Shared helper of the MFMA-family sweep (tests/test_widesweep_sync_cpu.py,
test_gpu_widesweep_layerwise.py, test_gpu_widesweep_fused.py): the constants
the reverse mode's dispatch reads (csrc/cnf_wvjp.hip, cnf_wide16.hip), the
launch plan restated from them, the list of cases with the classes each one is
there for, and the admitted inputs and float64 references the GPU files share.

cnf_vjp_launch_plan (CouplingStack.vjp_launch_plan) reports what the library
would launch; expected_plan() below says what this file believes it launches.
tests/test_widesweep_sync_cpu.py parses the sources, holds the constants here
to them, holds expected_plan to the library over a grid of descriptors, and
shows that the cases reach every class that grid can select.
"""
import collections
import copy

import numpy as np
import torch

import _sweep
from _golden import rel_err

# ---- csrc/cnf_wvjp.hip, cnf_wide16.hip (checked by test_widesweep_sync_cpu.py) --------
NJ_MAX = (64, 128, 192)     # pick_nj: kNJ = 1, 2, 3 up to these widths, else 4
KBN = 64                    # kBN: output columns per k_wgemm block
KKC = 128                   # kKC: reduction chunk
DW16_CT = 7                 # kDw16CT: 16-column tiles per k_wdw16 wave
LDS_BYTES = 160 * 1024      # wvjp_ok's kLds
WAVE_BLOCKS_CAP = 16384     # wave_grid
NSEED_CAP = 4096            # make_plan / plan16: k_wseed's blocks
KB_RECORDS = 256            # row blocks of the weight gradients at most
KB_ROWS_MIN = 256           # ... of at least this many rows
KEEP_ACTS_BYTES = 8 * 2 ** 30   # kKeepActsBytes
W16_TABLE = [(100, [100, 100]), (100, [100]), (100, []), (32, [64, 64])]   # kW16Table
DWG_CLASSES = [(7, 4), (7, 7), (4, 7), (4, 4), (4, 2), (4, 5), (1, 5)]     # CNF_DWG_CLASSES

SIGMA = 0.05                # as tests/test_gpu_tile_envelope.py above D = 24
DET = 0.7                   # the CE loss's log-det weight
OUT_BAR, GRAD_BAR = 1e-5, 1e-4          # tests/_golden.py, DESIGN section 5
OUT_COND, GRAD_COND = OUT_BAR / 4, GRAD_BAR / 4
MAX_SEEDS = 64


def r8(n):
    return (n + 7) & ~7


def al64(n):
    return (n + 63) // 64 * 64


class Shape:
    """Shape of cnf_internal.h for a descriptor of the tile family."""

    def __init__(self, D, hidden, L, scale=True, shift=True, strict=False):
        self.D, self.hidden, self.L, self.strict = D, list(hidden), L, bool(strict)
        self.scale, self.shift = bool(scale), bool(shift)
        self.DT, self.DC = D // 2, D - D // 2
        self.nets = int(self.scale) + int(self.shift)
        self.units = [D] + self.hidden + [D]
        self.n_lin = len(self.hidden) + 1
        self.net_floats = sum(self.units[i + 1] * self.units[i] + self.units[i + 1]
                              for i in range(self.n_lin))
        self.layer_floats = self.net_floats * self.nets

    def lin_out(self, k):
        return (self.D if self.strict else self.DT) if k == self.n_lin - 1 else self.units[k + 1]

    def lin_in(self, k):
        return (self.D if self.strict else self.DC) if k == 0 else self.units[k]

    def hp(self, k):
        return r8(self.units[k + 1] + 1)

    def gp(self, k):
        return r8(self.lin_out(k))


def gemm_nc(cols):
    return min(KBN // 32, (cols + 31) // 32)


def gemm_lds(cols, K, pair):
    return r8(K) * (32 * gemm_nc(cols) + 8) * 4 * (2 if pair else 1)


def gemm_calls(s):
    """(cols, K, BT, EPI, PAIR) of every k_wgemm launch of one layer's sweeps."""
    last = s.n_lin - 1
    calls = [(s.lin_out(k) if k == last else s.hp(k), s.lin_in(k), True,
              "bias" if k == last else "bias_relu", False) for k in range(s.n_lin)]
    calls += [(s.gp(k - 1), s.lin_out(k), False, "mask", False) for k in range(1, s.n_lin)]
    calls.append((s.D if s.strict else s.DC, s.lin_out(0), False, "add", s.nets == 2))
    return calls


def wvjp_ok(s):
    """wvjp_ok (cnf_wvjp.hip) without legacy options: every launch's weight
    slice within one CU's LDS."""
    return all(gemm_lds(cols, K, pair) <= LDS_BYTES for cols, K, _, _, pair in gemm_calls(s))


def table_row(s):
    """The shape's row of kW16Table when wide_ok (a shift net, not strict), else -1."""
    if (s.D, s.hidden) in W16_TABLE and s.shift and not s.strict:
        return W16_TABLE.index((s.D, s.hidden))
    return -1


def kb_blocks(B):
    rows = max(KB_ROWS_MIN, ((B + KB_RECORDS - 1) // KB_RECORDS + 31) // 32 * 32)
    return rows, (B + rows - 1) // rows


def dw16_subs(N, K):
    return ((N + 127) // 128) * ((((K + 1 + 15) // 16) + DW16_CT - 1) // DW16_CT)


def expected_plan(s, B, inverse=False):
    """cnf_vjp_launch_plan restated, for D > 16 (the tile family) without
    legacy options, in CouplingStack.vjp_launch_plan's form.  (plan16's 96 GB
    tape limit is not restated: no batch here comes near it.)"""
    B = max(B, 1)
    if not wvjp_ok(s):
        return {"path": "none"}
    rows, nkb = kb_blocks(B)
    nseed = min(NSEED_CAP, (B + 15) // 16)
    row = table_row(s)
    if row >= 0 and not inverse:
        last = s.n_lin - 1
        classes = {((s.lin_out(k) + 15) // 16, (s.lin_in(k) + 1 + 15) // 16)
                   for k in range(s.n_lin)}
        wdwg = classes <= set(DWG_CLASSES)
        z = max(dw16_subs(s.lin_out(k), s.lin_in(k)) for k in range(last + 1))
        return {"path": "wide-fused", "row": row, "nets": s.nets, "nkb": nkb, "rows_kb": rows,
                "nseed": nseed, "wdwg": wdwg, "dw16_z": 0 if wdwg else z,
                "classes": classes & set(DWG_CLASSES)}
    acts = s.nets * (sum(al64(B * s.hp(k)) for k in range(s.n_lin - 1))
                     + al64(B * r8(s.D if s.strict else s.DT)))
    calls = gemm_calls(s)
    return {"path": "layerwise",
            "kNJ": 0 if inverse else 1 + sum(s.D > m for m in NJ_MAX),
            "keep_acts": s.L > 1 and acts * s.L * 4 <= KEEP_ACTS_BYTES,
            "nkb": nkb, "rows_kb": rows, "nseed": nseed,
            "wave_blocks": min((B + 3) // 4, WAVE_BLOCKS_CAP),
            "dw16_z": max(dw16_subs(s.lin_out(k), s.lin_in(k)) for k in range(s.n_lin)),
            "gemms": {(bt, epi, pair, gemm_nc(cols)) for cols, _, bt, epi, pair in calls},
            "ny": max((cols + KBN - 1) // KBN for cols, *_ in calls),
            "chunks": max((r8(K) + KKC - 1) // KKC for _, K, *_ in calls)}


def classes_of(plan):
    """The dispatch classes a plan is in, as hashable tags: what the sync test
    counts over the library's grid and over the cases."""
    p = plan["path"]
    if p == "none":
        return {("path", "none")}
    out = {("path", p), (p, "nkb>1", plan["nkb"] > 1), (p, "rows_kb>256", plan["rows_kb"] > 256),
           (p, "nseed capped", plan["nseed"] == NSEED_CAP)}
    if p == "layerwise":
        out |= {("kNJ", plan["kNJ"]), ("keep_acts", plan["keep_acts"]),
                ("wave_blocks capped", plan["wave_blocks"] == WAVE_BLOCKS_CAP),
                ("dw16_z>1", plan["dw16_z"] > 1), ("ny>1", plan["ny"] > 1),
                ("chunks", plan["chunks"])}
        out |= {("gemm",) + g for g in plan["gemms"]}
    else:
        out |= {("row x nets", plan["row"], plan["nets"]), ("wdwg", plan["wdwg"])}
        out |= {("wdwg class",) + c for c in plan["classes"]}
    return out


# ---- the cases ------------------------------------------------------------------------
# expect: the plan fields the case is there for, at its largest batch (literals; the sync
# test holds them, and expected_plan's every field, to cnf_vjp_launch_plan)
Case = collections.namedtuple(
    "Case", "id group D hidden L scale shift flip strict inverse batches expect")


def _c(group, D, hidden, L=2, scale=True, shift=True, flip=False, strict=False, inverse=False,
       batches=(1, 133), **expect):
    tag = "%s-%s-l%d%s%s%s%s%s-b%d" % (
        group, _sweep.shape_id(D, hidden), L, "" if scale else "-nice", "" if shift else "-noshift",
        "-flip" if flip else "", "-strict" if strict else "", "-inv" if inverse else "",
        batches[-1])
    return Case(tag, group, D, list(hidden), L, scale, shift, flip, strict, inverse,
                tuple(batches), expect)


LAYERWISE = [
    # width classes: both sides of every pick_nj threshold, and CNF_MAX_DIM
    _c("width", 64, [24], kNJ=1), _c("width", 65, [24], kNJ=2),
    _c("width", 128, [24], kNJ=2), _c("width", 129, [24], kNJ=3),
    _c("width", 192, [24], kNJ=3), _c("width", 193, [24], kNJ=4),
    _c("width", 256, [24], kNJ=4),
    # L = 1: keep_acts off, the backward sweep recomputes the hidden activations
    _c("width", 65, [33], L=1, kNJ=2, keep_acts=False),
    _c("width", 130, [24], strict=True, kNJ=3), _c("width", 256, [24], strict=True, kNJ=4),
    _c("width", 130, [24], inverse=True, kNJ=0), _c("width", 256, [24], inverse=True, kNJ=0),
    # GEMM classes
    _c("gemm", 64, [130], scale=False, ny=3, chunks=2),       # kEpiAdd without PAIR (NICE)
    _c("gemm", 64, [130], shift=False, ny=3, chunks=2),       # ... and the s-net alone
    _c("gemm", 130, [24], scale=False, kNJ=3),                # ... with NC = 2 (DC > 32)
    _c("gemm", 200, [136, 120], dw16_z=2, chunks=2),          # z > 1 from N > 128 and K + 1 > 112
    _c("gemm", 256, [280], batches=(1, 69), chunks=3, ny=5),  # the last width wvjp_ok admits
    _c("gemm", 256, [130, 40], batches=(1, 69), chunks=2),
    # four chunks: a narrow flow's wide hidden layer passes wvjp_ok (NC = 1 slices) up to
    # CNF_MAX_WIDTH; 390 is the narrowest-but-ragged K past 384 (r8: 392, a last chunk of 8)
    _c("gemm", 17, [390], batches=(1, 37), chunks=4, ny=7),
    # row blocks: nkb = 2 with a ragged second block (5 rows)
    _c("rows", 130, [136], batches=(261,), nkb=2, rows_kb=256),
    _c("rows", 40, [64], batches=(261,), nkb=2, rows_kb=256),
    # Batch caps.  No hidden layer, so no ReLU kink: the guard cannot admit a stack with
    # hidden units at this many rows (the expected number of pre-activations inside
    # KINK_MIN grows with rows x units; see the 517-row note in test_gpu_widesweep_fused).
    _c("caps", 17, [], flip=True, batches=(65541,), wave_blocks=16384, nseed=4096,
       rows_kb=288, nkb=228),
]
# the shape just past wvjp_ok's LDS bound: r8(281) * 72 * 4 * 2 > 160 KB
PAST_LDS = (256, [281])

_fused = []
for _row, (_D, _h) in enumerate(W16_TABLE):
    for _nets in (2, 1):
        for _L in (1, 3):
            _fused.append(_c("fused", _D, _h, L=_L, scale=_nets == 2, flip=_L == 3,
                             batches=(1, 131), row=_row, nets=_nets, wdwg=True))
        # two row-block records for k_wdw16g to sum
        _fused.append(_c("fused", _D, _h, L=2, scale=_nets == 2, batches=(261,), row=_row,
                         nets=_nets, wdwg=True, nkb=2))
# both sides of plan16's batch caps (nseed, rows_kb, many row-block records) on the one
# table row without hidden units (no kink; see the caps case above)
_fused.append(_c("fused", 100, [], L=2, flip=True, batches=(65541,), row=2, nets=2, wdwg=True,
                 nseed=4096, rows_kb=288, nkb=228))
FUSED = _fused
FUSED_FORWARD_BATCHES = (1, 131, 517)   # 131: one block plus a wave with three rows
CASES = LAYERWISE + FUSED
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def shape_of(case):
    return Shape(case.D, case.hidden, case.L, case.scale, case.shift, case.strict)


def case_plan(case, B=None):
    return expected_plan(shape_of(case), case.batches[-1] if B is None else B, case.inverse)


def assert_plan(case, stack, B):
    """The library's plan for this call is the restated one, and at the
    case's largest batch it has the fields the case is there for."""
    got = stack.vjp_launch_plan(B, case.inverse)
    assert got == case_plan(case, B), (case.id, B, got)
    if B == case.batches[-1]:
        assert {k: got[k] for k in case.expect} == case.expect, (case.id, got)
    return got


# ---- admitted inputs and float64 references -------------------------------------------

def hidden_margin(flow64, run):
    """kink_margin of _sweep for whatever `run` evaluates (the inverse too):
    min over every hidden Linear call of |a| / (sum |W||h| + |b| + 1)."""
    worst = [float("inf")]
    hooks = []

    def hook(lin, args, out):
        m = args[0].abs() @ lin.weight.abs().t() + lin.bias.abs()
        worst[0] = min(worst[0], float((out.abs() / (m + 1)).min()))

    for ly in flow64.layers:
        for net, on in ((ly.s, ly.scale), (ly.t, ly.shift)):
            if on:
                hooks += [lin.register_forward_hook(hook) for lin in list(net.layers)[:-1]]
    try:
        with torch.no_grad():
            run()
    finally:
        for h in hooks:
            h.remove()
    return worst[0]


def params(flow):
    return [p for p in flow.parameters() if p.requires_grad]


def objective(flow, name, xin, y, w, wl, inverse):
    """The scalar a gradient case differentiates, on any Flow (float64 CPU,
    fp32 CPU, device): "all" weights every layer's output and the log-det,
    "fin" the final output and the log-det (Flow.transform /
    inverse_transform), "cal" / "ce" the calibrator losses' mean."""
    B = xin.shape[0]
    if name == "all":
        outs, ld = flow.backward(xin) if inverse else flow(xin)
        return (torch.stack(list(outs)) * w).sum() + (ld.reshape(-1) * wl).sum()
    if name == "fin":
        out, ld = flow.inverse_transform(xin) if inverse else flow.transform(xin)
        return (out * w[-1]).sum() + (ld.reshape(-1) * wl).sum()
    z, ld = flow.transform(xin)
    kind = 0 if name == "cal" else 1
    return _sweep.loss_rows64(z, ld.reshape(-1), y, kind, 1.0 if kind == 0 else DET)[0].sum() / B


def objectives(case):
    return ("all", "fin") if case.inverse else ("all", "fin", "cal", "ce")


def cpu_grads(flow, case, x, y, w, wl):
    """{objective: (flat parameter gradient, input gradient)} by CPU autograd in
    the flow's dtype."""
    dt = next(flow.parameters()).dtype
    out = {}
    for name in objectives(case):
        xin = x.to(dt).clone().requires_grad_(True)
        obj = objective(flow, name, xin, y, w.to(dt), wl.to(dt), case.inverse)
        ps = params(flow)
        gs = torch.autograd.grad(obj, ps + [xin], allow_unused=True)
        gs = [torch.zeros_like(t) if g is None else g for g, t in zip(gs, ps + [xin])]
        out[name] = ([g.numpy().astype(np.float64) for g in gs[:-1]],
                     gs[-1].numpy().astype(np.float64))
    return out


def worst_grad(got, ref):
    """max grad_err over the parameter tensors and the input gradient."""
    return max([_sweep.grad_err(a, b) for a, b in zip(got[0], ref[0])]
               + [_sweep.grad_err(got[1], ref[1])])


def _rows_of(flow, x, y, name):
    kind = 0 if name == "cal" else 1
    with torch.no_grad():
        z, ld = flow.transform(x)
        return _sweep.loss_rows64(z, ld.reshape(-1), y, kind, 1.0 if kind == 0 else DET)


def terms_ratio(err, bound):
    """max err / bound; a zero bound (NICE: the log-det is exactly 0) takes a
    zero error."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(np.max(r))


def _terms_floor(flow, f64, x, y, name):
    """The fp32 CPU path's own loss-term error on these rows over the terms'
    bar (OUT_BAR x the sum of the per-row magnitudes), worst of the three."""
    rows = _rows_of(f64, x.double(), y, name).numpy()
    got = _rows_of(flow, x, y, name).sum(dim=1).double().numpy()
    return terms_ratio(np.abs(got - rows.sum(axis=1)), OUT_BAR * np.abs(rows).sum(axis=1))


class Prepared:
    pass


_prepared = {}


def prepare_grad(case):
    """The admitted gradient case (cached for the session).  Decided on the CPU
    from the references alone, at the case's largest batch (smaller ones are
    its first rows): the first seed from _sweep.SEED0 on at which
      * _sweep.guarded_flow's conditions hold (the fp32 numpy oracle within
        FP32_COND of float64, every hidden pre-activation KINK_MIN away from
        the ReLU kink -- for an inverse case those of the inverse steps too),
      * the package's fp32 torch-op CPU path gives every gradient within
        GRAD_COND (a quarter of the bar) of float64 CPU autograd, and the loss
        terms of every batch the case runs within a quarter of theirs (one
        row's log-det can cancel to ~1e-3, where fp32's own rounding of the
        sum passes 1e-5 of it).
    The whole case moves to the next seed; no row is dropped or rescaled."""
    if case.id in _prepared:
        return _prepared[case.id]
    BMAX = case.batches[-1]
    x, y, _ = _sweep.inputs(BMAX, case.D, seed=1)
    g = torch.Generator().manual_seed(2)
    w = torch.randn(case.L, BMAX, case.D, generator=g)
    wl = torch.randn(BMAX, generator=g)
    tried = []
    for seed in range(_sweep.SEED0, _sweep.SEED0 + MAX_SEEDS):
        flow = _sweep.make_flow(case.D, case.L, case.hidden, SIGMA, seed, case.scale, case.shift,
                                case.flip)
        f64 = _sweep.ref64(flow)
        if _sweep.fp32_oracle_error(flow, x) > _sweep.FP32_COND or \
                _sweep.kink_margin(flow, x) < _sweep.KINK_MIN:
            tried.append((seed, "guard"))
            continue
        xin = x
        if case.inverse:   # the inverse runs on the forward output, rounded to fp32
            with torch.no_grad():
                xin = f64.transform(x.double())[0].float()
            if hidden_margin(f64, lambda: f64.backward(xin.double())) < _sweep.KINK_MIN:
                tried.append((seed, "inverse guard"))
                continue
        ref = cpu_grads(f64, case, xin, y, w, wl)
        cpu = cpu_grads(flow, case, xin, y, w, wl)
        floor = max(worst_grad(cpu[k], ref[k]) for k in ref)
        if floor > GRAD_COND:
            tried.append((seed, floor))
            continue
        tfloor = 0.0 if case.inverse else max(
            _terms_floor(flow, f64, xin[:B], y[:B], name) for B in case.batches
            for name in ("cal", "ce"))
        if tfloor > 0.25:
            tried.append((seed, "terms", tfloor))
            continue
        p = Prepared()
        p.case, p.seed, p.flow, p.f64, p.floor = case, seed, flow, f64, floor
        p.terms_floor = tfloor
        p.x, p.y, p.w, p.wl = xin, y, w, wl
        p.refs = {BMAX: ref}
        _prepared[case.id] = p
        return p
    raise AssertionError("no admissible seed for %s: %r" % (case.id, tried))


def grad_refs(p, B):
    """float64 CPU autograd of the case's objectives on its first B rows."""
    if B not in p.refs:
        p.refs[B] = cpu_grads(p.f64, p.case, p.x[:B], p.y[:B], p.w[:, :B], p.wl[:B])
    return p.refs[B]


def loss_rows(p, B, name):
    """Per-row (loss, ce, ld) in float64 for "cal" / "ce"."""
    return _rows_of(p.f64, p.x[:B].double(), p.y[:B], name).numpy()


def probs_err(got, ref):
    """_rowsweep.probs_err: the probabilities in units of the uniform one."""
    D = np.asarray(ref).shape[-1]
    return rel_err(np.asarray(got, dtype=np.float64) * D, np.asarray(ref, dtype=np.float64) * D)


def prepare_forward(case):
    """The admitted forward case at max(FUSED_FORWARD_BATCHES) centred rows
    (_sweep.conditioned_flow) with its float64 oracle outputs, the fp32
    oracle's inverse, float64 predict and the fp32 CPU path's own D * p error."""
    key = ("fwd", case.id)
    if key in _prepared:
        return _prepared[key]
    from oracle import cnf_oracle as O
    BMAX = max(FUSED_FORWARD_BATCHES)
    x, _, prior = _sweep.inputs(BMAX, case.D, seed=1)
    x = x - x.mean(dim=1, keepdim=True)
    flow, seed, x = _sweep.conditioned_flow(case.D, case.L, case.hidden, x, case.scale,
                                            case.shift, case.flip, sigma=SIGMA)
    l64, l32 = _sweep.oracle_layers(flow, np.float64), _sweep.oracle_layers(flow, np.float32)
    p = Prepared()
    p.case, p.seed, p.flow, p.x, p.prior = case, seed, flow, x, prior
    zs64, p.ld64 = O.flow_forward(l64, x.numpy().astype(np.float64))
    p.z64 = zs64[-1]
    p.zin = p.z64.astype(np.float32)
    xs64, p.ild64 = O.flow_inverse(l64, p.zin.astype(np.float64))
    xs32, p.ild32 = O.flow_inverse(l32, p.zin)
    p.x64, p.x32 = xs64[-1], xs32[-1]
    p.p64 = _sweep.predict64(torch.from_numpy(p.z64), prior).numpy()
    with torch.no_grad():
        q = torch.log(torch.softmax(flow.transform(x)[0], dim=1) + 1e-7) - torch.log(prior)
        p.p32 = torch.softmax(q, dim=1).numpy()
    _prepared[key] = p
    return p


def to_device(flow, dev, strict=False):
    fg = copy.deepcopy(flow).to(dev)
    fg.strict_nan = strict
    return fg


# ---- exact workspace, sentinels, repeatability (GPU) -----------------------------------
DEV = "cuda:0"
SENT = 12345.0
PAD = 64     # sentinel floats on each side of every buffer


class Fenced:
    """A float buffer of n elements between two runs of sentinels."""

    def __init__(self, n, fill=None):
        self.buf = torch.full((n + 2 * PAD,), SENT, dtype=torch.float32, device=DEV)
        self.view = self.buf[PAD:PAD + n]
        if fill is not None:
            self.view.copy_(fill.reshape(-1))

    def intact(self):
        return bool((self.buf[:PAD] == SENT).all()) and bool((self.buf[-PAD:] == SENT).all())


def run_fenced(stack, case, p, B, entry):
    """One cnf_vjp / cnf_vjp_inverse / cnf_loss_vjp call with an exact
    workspace and fenced outputs; returns the outputs' bytes."""
    import ctypes
    from cnf_hip import _lib
    from cnf_hip.stack import _ptr, _stream
    lib = _lib.lib()
    blob = stack.prepared(torch.device(DEV))
    n = ctypes.c_size_t()
    q = "cnf_vjp_inverse_workspace_bytes" if entry == "cnf_vjp_inverse" else "cnf_vjp_workspace_bytes"
    _lib.check(q, getattr(lib, q)(ctypes.byref(stack.desc), ctypes.c_int64(B), ctypes.byref(n)))
    assert n.value % 4 == 0
    ws = Fenced(n.value // 4)
    x = p.x[:B].to(DEV).contiguous()
    grads, dx, terms = Fenced(stack.param_count()), Fenced(B * case.D), Fenced(3)
    if entry == "cnf_loss_vjp":
        y = p.y[:B].to(DEV)
        st = lib.cnf_loss_vjp(ctypes.byref(stack.desc), _ptr(blob), _ptr(x), _ptr(y),
                              ctypes.c_int32(0), ctypes.c_float(1.0), ctypes.c_float(1.0 / B),
                              _ptr(terms.view), _ptr(grads.view), _ptr(dx.view), ctypes.c_int64(B),
                              _ptr(ws.view), ctypes.c_size_t(n.value), _stream(torch.device(DEV)))
    else:
        gza = p.w[:, :B].to(DEV).contiguous()
        gld = p.wl[:B].to(DEV).contiguous()
        st = getattr(lib, entry)(ctypes.byref(stack.desc), _ptr(blob), _ptr(x), None, _ptr(gza),
                                 _ptr(gld), _ptr(grads.view), _ptr(dx.view), ctypes.c_int64(B),
                                 _ptr(ws.view), ctypes.c_size_t(n.value),
                                 _stream(torch.device(DEV)))
    _lib.check(entry, st)
    torch.cuda.synchronize()
    for name, f in (("workspace", ws), ("grads", grads), ("dx", dx), ("terms", terms)):
        assert f.intact(), "%s: %s written outside its bounds" % (entry, name)
    out = [grads.view.clone(), dx.view.clone()]
    if entry == "cnf_loss_vjp":
        out.append(terms.view.clone())
    else:
        assert bool((terms.view == SENT).all())
    return out


def check_fenced(stack, case, p, B, entry, ref):
    a = run_fenced(stack, case, p, B, entry)
    b = run_fenced(stack, case, p, B, entry)
    for u, v in zip(a, b):
        assert torch.equal(u, v), "%s: a repeated call differs" % entry
    got = ([t.cpu().numpy() for t in stack.split(a[0])], a[1].cpu().numpy().reshape(B, case.D))
    e = worst_grad(got, ref)
    assert e <= GRAD_BAR, (entry, e)
    return e


# ---- records --------------------------------------------------------------------------
_rows = {}


def record(case, **fields):
    """One row per case in conftest.RECORDS["wide_sweep"]; fields merge, errors
    keep their worst."""
    import conftest
    row = _rows.get(case.id)
    if row is None:
        row = _rows[case.id] = {"case": case.id, "group": case.group}
        conftest.RECORDS.setdefault("wide_sweep", []).append(row)
    for k, v in fields.items():
        row[k] = max(row[k], v) if isinstance(v, float) and k in row else v
