"""float64 restatement of one k_adam step (csrc/cnf_adam.hip) with a running
rounding bound, an fp32 op-by-op restatement, deliberately wrong variants, and
the case lists of the Adam sweep (tests/test_adam_ref_cpu.py,
tests/test_gpu_adam_sweep.py).  NumPy only.

The update, as adam_tensors / k_adam state it (torch.optim.Adam, amsgrad off,
coupled weight decay):

    g' = g + wd * p                       (only when wd != 0)
    m' = m + (1 - b1) * (g' - m)
    v' = v * b2 + (g' * g') * (1 - b2)
    p' = p - step_size * (m' / (sqrt(v') / bc2_sqrt + eps))

with 1 - b1, b2, 1 - b2, eps, wd, step_size = lr / (1 - b1^t) and
bc2_sqrt = sqrt(1 - b2^t) each formed in double and rounded to fp32 once
(`scalars`).

The bound.  `step_ref` evaluates the formula in float64 from the fp32 inputs
and carries, per element and per intermediate, a bound on what an fp32
evaluation of the same operations can be off by: every fp32 operation adds
U * |result| + TINY (U = 2^-24, half an ulp of a normal result; TINY = 2^-149
covers a subnormal one), and the bounds of its inputs pass through with the
operation's derivative:

    a +- b     e_a + e_b
    c * a      |c| e_a                      (c one of the exact fp32 scalars)
    a * a      (2 |a| + e_a) e_a            (the square term kept: g' can cancel
                                             to the size of its own bound)
    sqrt(a)    the larger of sqrt(a + e) - sqrt(a) and sqrt(a) - sqrt(max(a - e, 0))
               (the derivative's closed form; finite at a = 0)
    a / d      e_a / d_lo + |a| e_d / (d d_lo),  d_lo = max(d - e_d, eps / 2)

A fused multiply-add rounds once where the separate form rounds twice, so the
bound covers both.  Nothing in it is fitted to a device result; the tests hold
the fp32 restatements (fused and not) to 1 x bound on the CPU and every device
evaluation to 2 x bound (second-order terms of the other operations, and the
difference between the two forms).
"""
import math
import re
from collections import namedtuple

import numpy as np

F = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -149

# ---- the launch constants of csrc/cnf_adam.hip (test_adam_ref_cpu holds them to the source)
CHUNK = 128          # kAdamTensors: tensors per launch
BLOCK = 256          # threads per block, elements per block and pass
GRID_BLOCKS = 64     # blocks per tensor at most
CAP = GRID_BLOCKS * BLOCK   # elements of one tensor per grid-stride pass


def parse_source(text):
    """(chunk, block, grid_blocks) as cnf_adam.hip states them; every place the
    block size appears must agree."""
    chunk = re.search(r"constexpr int kAdamTensors = (\d+);", text)
    bounds = re.search(r"__launch_bounds__\((\d+)\) void k_adam\b", text)
    grid = re.search(r"std::min<int64_t>\(\(maxn \+ (\d+)\) / (\d+), (\d+)\)", text)
    first = re.search(r"\(int64_t\)blockIdx\.x \* (\d+) \+ threadIdx\.x", text)
    stride = re.search(r"i \+= \(int64_t\)gridDim\.x \* (\d+)\)", text)
    launch = re.search(r"dim3\(gx, \(unsigned\)n_here\), dim3\((\d+)\)", text)
    assert chunk and bounds and grid and first and stride and launch
    block = int(bounds.group(1))
    assert int(grid.group(1)) == block - 1 and int(grid.group(2)) == block
    assert int(first.group(1)) == block and int(stride.group(1)) == block
    assert int(launch.group(1)) == block
    assert "std::min(kAdamTensors, nt - first)" in text and "first += kAdamTensors" in text
    return int(chunk.group(1)), block, int(grid.group(3))


# ---- scalars ----------------------------------------------------------------------
# hp = (lr, beta1, beta2, eps, weight_decay), Python floats
HPARAMS = {
    "default": (1e-3, 0.9, 0.999, 1e-8, 0.0),
    "wd": (1e-3, 0.9, 0.999, 1e-8, 0.01),
    "fast": (1e-2, 0.8, 0.99, 1e-6, 0.0),
    "slow_wd": (1e-3, 0.95, 0.9999, 1e-8, 0.1),
    "beta1_0": (1e-3, 0.0, 0.999, 1e-8, 0.0),
}
STEPS = (1, 2, 7, 1000, 100000)

Scalars = namedtuple("Scalars", "omb1 beta2 omb2 eps wd step_size bc2_sqrt")


def _f(x):
    return float(F(x))


def scalars(hp, t):
    """adam_tensors' seven kernel scalars: doubles rounded to fp32 once."""
    lr, b1, b2, eps, wd = hp
    return Scalars(_f(1.0 - b1), _f(b2), _f(1.0 - b2), _f(eps), _f(wd),
                   _f(lr / (1.0 - math.pow(b1, float(t)))),
                   _f(math.sqrt(1.0 - math.pow(b2, float(t)))))


def double_scalars(hp, t):
    """The same seven left in double: what torch.optim.Adam uses on float64
    parameters (test_adam_ref_cpu anchors the formula to torch with these)."""
    lr, b1, b2, eps, wd = hp
    return Scalars(1.0 - b1, b2, 1.0 - b2, eps, wd, lr / (1.0 - b1 ** t), (1.0 - b2 ** t) ** 0.5)


def sched_scalars(hp, sched):
    """The scalars of a sched-form step: step_size and bc2_sqrt are the two
    fp32 values the kernel reads from device memory."""
    s = scalars(hp, 1)
    return s._replace(step_size=_f(sched[0]), bc2_sqrt=_f(sched[1]))


# ---- float64 restatement with the running bound ------------------------------------
Ref = namedtuple("Ref", "p m v ep em ev")


def _rnd(x):
    return U * np.abs(x) + TINY


def step_ref(p, g, m, v, s):
    """One step from fp32 (or float64) inputs and Scalars `s`: float64 p', m',
    v' and the bound of each (module docstring)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    if s.wd != 0.0:
        t1 = s.wd * p
        gd = g + t1
        eg = _rnd(t1) + _rnd(gd)
    else:
        gd, eg = g, np.zeros_like(g)
    d = gd - m
    ed = eg + _rnd(d)
    sm = s.omb1 * d
    es = s.omb1 * ed + _rnd(sm)
    m1 = m + sm
    em = es + _rnd(m1)
    gg = gd * gd
    egg = (2.0 * np.abs(gd) + eg) * eg + _rnd(gg)
    a = v * s.beta2
    ea = _rnd(a)
    b = gg * s.omb2
    eb = s.omb2 * egg + _rnd(b)
    v1 = a + b
    ev = ea + eb + _rnd(v1)
    r = np.sqrt(v1)
    er = np.maximum(np.sqrt(v1 + ev) - r, r - np.sqrt(np.maximum(v1 - ev, 0.0))) + _rnd(r)
    q = r / s.bc2_sqrt
    eq = er / s.bc2_sqrt + _rnd(q)
    den = q + s.eps
    eden = eq + _rnd(den)
    lo = np.maximum(den - eden, s.eps / 2)
    w = m1 / den
    ew = em / lo + np.abs(m1) * eden / (den * lo) + _rnd(w)
    u = s.step_size * w
    eu = s.step_size * ew + _rnd(u)
    p1 = p - u
    ep = eu + _rnd(p1)
    return Ref(p1, m1, v1, ep, em, ev)


def ratios(ref, p, m, v):
    """Worst |got - ref| / bound of p, m, v; inf for a non-finite element."""
    out = {}
    for k, got, want, e in (("p", p, ref.p, ref.ep), ("m", m, ref.m, ref.em),
                            ("v", v, ref.v, ref.ev)):
        got = np.asarray(got, np.float64).reshape(-1)
        if got.size == 0:
            out[k] = 0.0
            continue
        r = np.abs(got - want) / e
        out[k] = float(np.max(np.where(np.isfinite(got), r, np.inf)))
    return out


# ---- fp32 restatement, operation by operation ----------------------------------------
def _fma(a, b, c):
    # the 24 x 24-bit product is exact in double; one rounding to fp32 at the end
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64)
            + np.asarray(c, np.float64)).astype(F)


def step_f32(p, g, m, v, s, fused=False):
    """The kernel's operations on fp32 arrays, each rounded to fp32.  fused:
    g + wd * p and p - step_size * (m' / denom) as one FMA each, the two the
    gfx950 code object contracts; the other three products stay separate."""
    p, g, m, v = (np.asarray(a, F) for a in (p, g, m, v))
    omb1, beta2, omb2, eps, wd, step, bc2 = (F(x) for x in s)
    if wd != 0:
        g = _fma(wd, p, g) if fused else g + wd * p
    m1 = m + omb1 * (g - m)
    v1 = v * beta2 + (g * g) * omb2
    den = np.sqrt(v1) / bc2 + eps
    w = m1 / den
    p1 = _fma(-step, w, p) if fused else p + (-step) * w
    assert p1.dtype == F and m1.dtype == F and v1.dtype == F
    return p1, m1, v1


# ---- deliberately wrong variants (float64) -------------------------------------------
# name -> what it gets wrong
WRONG = {
    "adamw": "decoupled weight decay: p scaled by 1 - lr wd, the gradient left alone",
    "beta1_for_omb1": "m' = m + beta1 (g' - m)",
    "v_from_raw_g": "v' built from g, not g + wd p",
    "no_bc2": "denominator sqrt(v') + eps, the second bias correction dropped",
    "eps_before_bc2": "denominator (sqrt(v') + eps) / bc2_sqrt",
    "eps_in_sqrt": "denominator sqrt(v' + eps) / bc2_sqrt",
}


def step_wrong(name, p, g, m, v, hp, t):
    s = scalars(hp, t)
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    gd = g + s.wd * p if name != "adamw" else g
    if name == "adamw":
        p = p * (1.0 - hp[0] * hp[4])
    m1 = m + (_f(hp[1]) if name == "beta1_for_omb1" else s.omb1) * (gd - m)
    gv = g if name == "v_from_raw_g" else gd
    v1 = v * s.beta2 + gv * gv * s.omb2
    if name == "no_bc2":
        den = np.sqrt(v1) + s.eps
    elif name == "eps_before_bc2":
        den = (np.sqrt(v1) + s.eps) / s.bc2_sqrt
    elif name == "eps_in_sqrt":
        den = np.sqrt(v1 + s.eps) / s.bc2_sqrt
    else:
        den = np.sqrt(v1) / s.bc2_sqrt + s.eps
    return p - s.step_size * (m1 / den), m1, v1


def must_catch(name, regime, hp_name, t):
    """Whether the sweep case (regime, hyper-parameters, t), at either moment
    state, has to expose wrong variant `name` past 2 x bound.

    adamw, v_from_raw_g: wherever wd != 0 -- m' (v') moves by (1 - b) wd p
      terms, 1e-4 and more of its size, in every regime.
    beta1_for_omb1: every case of the unit regime (b1 != 1 - b1 in all sets).
    no_bc2: t <= 7 in the unit, small and eps regimes: bc2_sqrt <= 0.27 there
      and sqrt(v') / bc2_sqrt is not under eps.  (At t = 100000 bc2_sqrt is 1
      to fp32 for three of the five sets, and in the subnormal regime eps is
      the whole denominator: neither can see it.)
    eps_before_bc2: t <= 7 in the eps regime, where eps / bc2_sqrt against eps
      is a change of the order of the denominator itself.
    eps_in_sqrt: the small and eps regimes at every t: v' is of eps's size
      (g^2 ~ 1e-8) or far under it.
    """
    wd = HPARAMS[hp_name][4]
    if name in ("adamw", "v_from_raw_g"):
        return wd != 0.0
    if name == "beta1_for_omb1":
        return regime == "unit"
    if name == "no_bc2":
        return t <= 7 and regime in ("unit", "small", "eps")
    if name == "eps_before_bc2":
        return t <= 7 and regime == "eps"
    if name == "eps_in_sqrt":
        return regime in ("small", "eps")
    raise KeyError(name)


# ---- gradient regimes -------------------------------------------------------------------
REGIMES = ("unit", "small", "eps", "subnormal", "loguniform", "cancel")
_SCALE = {"unit": 1.0, "small": 1e-4, "eps": 3e-8, "subnormal": 1e-20}


def _grad(regime, p, wd, rng):
    n = p.size
    if regime in _SCALE:
        return (rng.standard_normal(n) * _SCALE[regime]).astype(F)
    if regime == "loguniform":
        return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-10, 1, n)).astype(F)
    if regime == "cancel":   # g + wd p cancels to 2^-12 of its terms
        return (-_f(wd) * p.astype(np.float64)
                * (1.0 + rng.choice([-1.0, 1.0], n) * 2.0 ** -12)).astype(F)
    raise KeyError(regime)


def make_state(regime, hp_name, n, carried, seed=0):
    """fp32 (p, g, m, v) of n elements: p ~ N(0, 1), g of the regime; moments
    zero, or carried from one earlier gradient g0 of the same regime
    (m = (1 - b1) g0', v = (1 - b2) g0'^2, g0' = g0 + wd p, rounded to fp32)."""
    hp = HPARAMS[hp_name]
    rng = np.random.default_rng([seed, REGIMES.index(regime), list(HPARAMS).index(hp_name),
                                 int(carried)])
    p = rng.standard_normal(n).astype(F)
    g = _grad(regime, p, hp[4], rng)
    if carried:
        g0 = _grad(regime, p, hp[4], rng).astype(np.float64) + _f(hp[4]) * p
        m = ((1.0 - hp[1]) * g0).astype(F)
        v = ((1.0 - hp[2]) * g0 * g0).astype(F)
    else:
        m, v = np.zeros(n, F), np.zeros(n, F)
    return p, g, m, v


SWEEP = [(r, h, t, c) for r in REGIMES for h in HPARAMS for t in STEPS for c in (False, True)]


def is_zero_case(regime, hp_name, carried):
    """cancel with wd = 0 is g = 0: with zero moments the step must be exact."""
    return regime == "cancel" and HPARAMS[hp_name][4] == 0.0 and not carried


# ---- geometry lists (from the launch constants) --------------------------------------------
SIZES = (0, 1, BLOCK - 1, BLOCK, BLOCK + 1, CAP - 1, CAP, CAP + 1, 2 * CAP + 1, 40000)
COUNTS = (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)


def _count_sizes(k):
    # small, all different in a run, one past a block now and then
    return [(i * 37) % 300 + 1 + (BLOCK if i % 50 == 49 else 0) for i in range(k)]


def geometries():
    """name -> tensor sizes of one cnf_adam_step_tensors call."""
    geo = {"n=%d" % n: [n] for n in SIZES}
    # one chunk: small tensors under the gx of a large one, on both sides of it
    geo["mixed"] = [1, BLOCK + 1, 2 * CAP + 1, 0, BLOCK - 1, CAP, 40000, BLOCK, CAP - 1, CAP + 1, 1]
    for k in COUNTS:
        geo["count=%d" % k] = _count_sizes(k)
    geo["empty_first"] = [0, 300, CAP + 1]
    geo["empty_middle"] = [300, 0, 0, CAP + 1]
    geo["empty_last"] = [300, CAP + 1, 0]
    geo["empty_chunk_then_two"] = [0] * CHUNK + [1000, CAP + 1]
    geo["empty_chunk_between"] = [700] + [0] * (2 * CHUNK - 1) + [CAP + 1, 3]
    return geo


def split(flat, sizes):
    out, off = [], 0
    for n in sizes:
        out.append(flat[off:off + n])
        off += n
    assert off == flat.size
    return out
