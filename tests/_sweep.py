"""Shared helper of the narrow-table sweeps (tests/test_table_sync_cpu.py,
test_gpu_table_forward.py, test_gpu_table_vjp.py, test_gpu_tile_envelope.py):
the shapes of the compile-time kernel tables, seeded flows, their float64
references and the ReLU-kink guard of the gradient tests.

NARROW mirrors kTable of csrc/cnf_valu.hip (k_valu, and k_vjp's kVTable); the
third field says whether the shape is also in kSTable (k_sgpr, cnf_sgpr.hip)
and kV2Part{A,B,C} (k_vjp2, cnf_vjp2_*.hip).  tests/test_table_sync_cpu.py
parses the five sources and fails when a table and this list disagree.
"""
import copy

import numpy as np
import torch

from flows.flows import Flow, NvpCouplingLayer
from oracle import cnf_oracle as O

# (D, hidden, in kSTable and kV2Part*)
NARROW = [
    (2, [5, 5], True), (3, [5, 5], True), (4, [5, 5], True), (5, [5, 5], True),
    (6, [5, 5], True), (8, [5, 5], True), (10, [5, 5], True),
    (3, [3, 3], True), (8, [3, 3], True), (10, [3, 3], True),
    (3, [3], True), (10, [10], False), (10, [10, 10], False),
    (3, [], True), (10, [], True),
    (10, [7], False), (10, [5], True), (3, [5], True),
]
# kLTable (CNF_OPT_S_TANH): the legacy tanh s-net shapes of k_valu
TANH = [(3, [3]), (10, [10]), (10, [5, 5])]

LARGE_BATCH = 4 << 20   # kLargeBatch (cnf_valu.hip): beyond it the `large` variant
V2_LMAX = 8             # kV2LMax (cnf_vjp2.h): layers k_vjp2's accumulators hold
VJP_ROWS = 64           # kVRows (cnf_vjp.hip)
VJP_GP = 65             # kGP
SIGMA = 0.2
SEED0 = 3               # the kink guard's search starts here


def shape_id(D, hidden):
    return "d%d_h%s" % (D, "x".join(map(str, hidden)) or "0")


def in_v2(D, hidden):
    return any(d == D and h == list(hidden) and s for d, h, s in NARROW)


def in_narrow(D, hidden):
    return any(d == D and h == list(hidden) for d, h, _ in NARROW)


def vjp_rows_lds_bytes(D, hidden, L, nets):
    """lds_bytes() of cnf_vjp.hip: k_vjp's stash, staging and accumulators."""
    h1 = hidden[0] if len(hidden) > 0 else 0
    h2 = hidden[1] if len(hidden) > 1 else 0
    DT, DC = D // 2, D - D // 2
    GS, HS = h1 + h2 + DT, DC + h1 + h2 + 1
    TG, TH = (GS + 15) // 16, (HS + 15) // 16
    ACC = TG * TH * 256
    return 4 * (L * DT * VJP_ROWS + 16 * (TG + TH) * VJP_GP + L * nets * ACC)


def expected_vjp_path(D, hidden, L, scale=True, shift=True, strict=False):
    """vjp_path() of cnf_vjp.hip for a narrow shape without legacy options:
    k_vjp2 for its table's shapes with a shift net, not strict, L <= kV2LMax;
    else k_vjp while not strict and its LDS estimate is <= 64 KB; else the
    layer-at-a-time sweeps."""
    assert in_narrow(D, hidden)
    if in_v2(D, hidden) and shift and not strict and L <= V2_LMAX:
        return "vjp2"
    nets = int(bool(scale)) + int(bool(shift))
    if not strict and vjp_rows_lds_bytes(D, hidden, L, nets) <= 64 * 1024:
        return "vjp-rows"
    return "layerwise"


def expected_kernel(D, hidden, shift=True, strict=False, no_sgpr=False):
    """cnf_kernel_name for a narrow shape without legacy options."""
    assert in_narrow(D, hidden)
    return "sgpr-fused" if in_v2(D, hidden) and shift and not strict and not no_sgpr \
        else "valu-fused"


def make_flow(D, L, hidden, sigma=SIGMA, seed=SEED0, scale=True, shift=True, flip=False):
    """A CPU flow with N(0, sigma) parameters (tests/test_gpu_parity._make_flow)."""
    torch.manual_seed(seed)
    np.random.seed(seed)
    f = Flow([NvpCouplingLayer(D, hidden, scale=scale, shift=shift, random_flip=flip)
              for _ in range(L)])
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in f.parameters():
            if p.requires_grad:
                p.copy_(torch.randn(p.shape, generator=g) * sigma)
    return f


def ref64(flow):
    """The float64 CPU reference of the same weights (plain torch ops)."""
    return copy.deepcopy(flow).cpu().double()


def oracle_layers(flow, dtype=np.float64):
    """The numpy oracle's layers (permutations included) in `dtype`."""
    l0 = flow.layers[0]
    st = {k: v.detach().cpu().numpy() for k, v in flow.state_dict().items()}
    ly = O.layers_from_state(st, len(flow.layers), l0.dim, len(l0.hidden_size) + 1,
                             l0.scale, l0.shift)
    return O.cast_layers(ly, dtype)


def inputs(B, D, seed=1):
    """Seeded fp32 rows, labels, and a non-uniform prior."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=g)
    y = torch.randint(0, D, (B,), generator=g)
    pri = torch.rand(D, generator=g) + 0.2
    return x, y, pri / pri.sum()


def kink_margin(flow, x):
    """min over every layer, net, hidden unit and row of |a| / (m + 1) in
    float64: a the hidden pre-activation, m = sum |W||h| + |b| its magnitude
    scale.  inf for a flow without hidden layers."""
    f = ref64(flow)
    h = x.detach().cpu().double()
    worst = float("inf")
    with torch.no_grad():
        for ly in f.layers:
            keep = ly.mask * h
            for net, on in ((ly.s, ly.scale), (ly.t, ly.shift)):
                if not on:
                    continue
                a_in = keep
                for lin in list(net.layers)[:-1]:
                    a = lin(a_in)
                    m = a_in.abs() @ lin.weight.abs().t() + lin.bias.abs()
                    worst = min(worst, float((a.abs() / (m + 1)).min()))
                    a_in = torch.relu(a)
            h, _ = ly(h)
    return worst


KINK_MIN = 2e-6   # ~32 fp32 ulps: a 10-term dot product's bound plus upstream forward error
# A case can tell a wrong kernel from rounding only while plain fp32 arithmetic
# leaves most of the 1e-5 bar unused: the fp32 numpy oracle's own error against
# float64 must stay within a quarter of it.  (At sigma 0.2 a stack without
# hidden layers can grow double-exponentially -- |z| ~ 1e16 after three layers,
# NaN in float64 after nine -- and the oracle's own error then passes 1e-5.)
FP32_COND = 2.5e-6


def fp32_oracle_error(flow, x):
    """rel_err (tests/_golden.py) of the fp32 numpy oracle's every-layer
    outputs and log-det against the float64 oracle on the rows x; inf when
    either has a non-finite entry."""
    from _golden import rel_err
    xn = x.detach().cpu().numpy().astype(np.float32)
    z64, ld64 = O.flow_forward(oracle_layers(flow, np.float64), xn.astype(np.float64))
    z32, ld32 = O.flow_forward(oracle_layers(flow, np.float32), xn)
    z64, z32 = np.stack(z64), np.stack(z32)
    if not (np.isfinite(z64).all() and np.isfinite(z32).all() and np.isfinite(ld64).all()
            and np.isfinite(ld32).all()):
        return float("inf")
    return max(rel_err(z32, z64), rel_err(ld32, ld64))


# The inverse is held to twice the fp32 oracle's own error; past 1e-4 (ten
# times the flat bar) that bar no longer tells a wrong kernel from rounding,
# and a non-finite oracle result makes it vacuous.
INV_COND = 1e-4


def fp32_oracle_inverse_error(flow, x):
    """As fp32_oracle_error, for the every-step inverse of the float64 forward
    output rounded to fp32 (the inverse checks' input)."""
    from _golden import rel_err
    l64, l32 = oracle_layers(flow, np.float64), oracle_layers(flow, np.float32)
    z64, _ = O.flow_forward(l64, x.detach().cpu().numpy().astype(np.float64))
    z32 = z64[-1].astype(np.float32)
    x64, ild64 = O.flow_inverse(l64, z32.astype(np.float64))
    x32, ild32 = O.flow_inverse(l32, z32)
    return max(rel_err(np.stack(x32), np.stack(x64)), rel_err(ild32, ild64))


def _search(D, L, hidden, x, scale, shift, flip, sigma, kink):
    # the rows as given, then halved (exactly, a power of two) up to three
    # times: the nine-layer stack without hidden layers has no admissible seed
    # on unit-variance rows at sigma 0.2
    for k in range(4):
        xs = x * 0.5 ** k
        for seed in range(SEED0, SEED0 + 64):
            f = make_flow(D, L, hidden, sigma, seed, scale, shift, flip)
            if fp32_oracle_error(f, xs) > FP32_COND:
                continue
            if kink_margin(f, xs) >= KINK_MIN if kink else \
                    fp32_oracle_inverse_error(f, xs) <= INV_COND:
                return f, seed, xs
    raise AssertionError("no admissible case for %r" % ((D, L, hidden, scale, shift, flip),))


def conditioned_flow(D, L, hidden, x, scale=True, shift=True, flip=False, sigma=SIGMA):
    """(flow, seed, rows): the first seed from SEED0 on (and, failing all 64,
    the rows x halved) at which the fp32 numpy oracle's own forward error on
    the rows is within FP32_COND and its inverse error within INV_COND.  An
    input condition, decided on the CPU from the oracles alone; the whole case
    moves, no row is ever dropped."""
    return _search(D, L, hidden, x, scale, shift, flip, sigma, False)


def guarded_flow(D, L, hidden, x, scale=True, shift=True, flip=False, sigma=SIGMA):
    """(flow, seed, rows) with the fp32 oracle's forward error within FP32_COND
    and every hidden pre-activation of the rows at least KINK_MIN (relative)
    away from the ReLU kink, so relu' is the same in every fp32 evaluation
    order (the gradient tests' guard; they run no inverse)."""
    return _search(D, L, hidden, x, scale, shift, flip, sigma, True)


def grad_err(got, ref):
    """tests/test_gpu_vjp._grad_err: max |got - ref| / (max |ref| + 1e-3)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref))) / (float(np.max(np.abs(ref))) + 1e-3)


def loss_rows64(z, ld, y, kind, det):
    """Per-row (loss, ce, ld) in float64 (calibrators.py:287-291; the CE kind:
    run_experiment3D.py:107), z / ld float64 torch tensors (autograd kept)."""
    lsm = torch.log_softmax(z, dim=1)
    lpy = lsm.gather(1, y.view(-1, 1)).squeeze(1)
    if kind == 0:
        ce = -torch.log(torch.exp(lpy) + 1e-7)
        loss = ce - ld
    else:
        ce = -lpy
        loss = ce - det * ld
    return torch.stack([loss, ce, ld.expand_as(ce)])


def predict64(z, prior):
    """calibrators.py:40-44 in float64 for the flow output z of centred rows."""
    p = torch.softmax(z, dim=1)
    return torch.softmax(torch.log(p + 1e-7) - torch.log(prior.double()), dim=1)


def record(row):
    import conftest
    conftest.RECORDS.setdefault("table_sweep", []).append(row)
