"""k_adam (csrc/cnf_adam.hip) on the GPU against the float64 restatement of
tests/_adam_ref.py, at its launch edges and gradient regimes.

Every device value of p, m and v is held to 2 x the restatement's derived
rounding bound (the bound itself holds, at 1 x, for an fp32 NumPy evaluation:
tests/test_adam_ref_cpu.py).  Indexing properties are bitwise: guard bands
around every parameter and around the three flat buffers stay untouched in
every call this file makes, a flat state gives the same bits however it is cut
into tensors, a raised skip flag moves nothing, and a non-finite gradient
element spoils its own element only.  torch.optim.Adam's own device steps
(single-tensor, foreach, fused) are held to the same bound, and their bit
mismatches against the kernel are recorded (conftest.RECORDS ->
adam_sweep.jsonl; the counts carry no bar).

All calls go through ctypes on cnf_adam_step_tensors except where a test names
StackAdam or a cnf_desc entry point.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import _adam_ref as A
from cnf_hip import _lib
from cnf_hip.adam import StackAdam
from cnf_hip.stack import Stack, _ptr, _stream
from conftest import RECORDS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64                         # sentinel floats on each side of every tensor
SENTINEL = np.uint32(0xDEADBEEF)
LIB = os.path.basename(_lib.LIB_PATH)


def _record(**row):
    row["lib"] = LIB
    RECORDS.setdefault("adam_sweep", []).append(row)
    print("adam_sweep", row)


class Arena:
    """fp32 arrays inside one sentinel-filled device buffer, PAD sentinels
    before, between and after them.  misalign: every array starts at an odd
    float (4-byte aligned, nothing more); otherwise at a multiple of four."""

    def __init__(self, arrays, misalign=False):
        self.pos, cur = [], 0
        for a in arrays:
            at = cur + PAD
            at = at | 1 if misalign else (at + 3) // 4 * 4
            self.pos.append((at, a.size))
            cur = at + a.size
        self.host = np.full(cur + PAD + 1, SENTINEL, np.uint32)
        self.inside = np.zeros(self.host.size, bool)
        for (at, n), a in zip(self.pos, arrays):
            self.host[at:at + n] = np.ascontiguousarray(a, np.float32).view(np.uint32)
            self.inside[at:at + n] = True
        self.dev = torch.from_numpy(self.host.view(np.int32)).to(DEV)
        assert self.dev.data_ptr() % 16 == 0

    def ptrs(self):
        # an empty tensor's pointer lands on a sentinel: non-null, never dereferenced
        return [self.dev.data_ptr() + 4 * at for at, _ in self.pos]

    def read(self, untouched=False):
        """The arrays after the call; the sentinels (or, for a read-only
        buffer, everything) must hold their bits."""
        back = self.dev.cpu().numpy().view(np.uint32)
        keep = np.ones(back.size, bool) if untouched else ~self.inside
        bad = np.flatnonzero(back[keep] != self.host[keep])
        assert bad.size == 0, "guard band written: %d words, first at %d" % (bad.size, bad[0])
        return [back[at:at + n].view(np.float32).copy() for at, n in self.pos]


def step(sizes, p, g, m, v, hp, t, sched=None, skip=None, misalign=False):
    """One cnf_adam_step_tensors call on guarded copies of the flat fp32 state,
    p cut into `sizes`.  Returns flat (p', m', v')."""
    sizes = list(sizes)
    pa = Arena(A.split(p, sizes), misalign)
    ga, ma, va = Arena([g]), Arena([m]), Arena([v])
    nt = len(sizes)
    numel = (ctypes.c_int64 * nt)(*sizes)
    arr = (ctypes.c_void_p * nt)(*pa.ptrs())
    if misalign:
        assert all(q % 8 == 4 for q in pa.ptrs())
    lr, b1, b2, eps, wd = hp
    st = _lib.lib().cnf_adam_step_tensors(nt, numel, arr, ga.ptrs()[0], ma.ptrs()[0], va.ptrs()[0],
                                          t, lr, _ptr(sched), b1, b2, eps, wd, _ptr(skip),
                                          _stream(torch.device(DEV)))
    _lib.check("cnf_adam_step_tensors", st)
    torch.cuda.synchronize()
    ga.read(untouched=True)
    ps = pa.read()
    return (np.concatenate(ps) if ps else np.zeros(0, np.float32)), ma.read()[0], va.read()[0]


def _held(ref, p, m, v, what):
    r = A.ratios(ref, p, m, v)
    assert max(r.values()) <= 2.0, (what, r)
    return r


# ---- regimes ---------------------------------------------------------------------------------
REGIME_SIZES = [A.CAP + 1, A.BLOCK + 1, 0, 1, 3000]     # ~20k elements, two passes in the first


@pytest.mark.parametrize("hp_name", list(A.HPARAMS))
@pytest.mark.parametrize("regime", A.REGIMES)
def test_regime(regime, hp_name):
    """Every t and both moment states of one (regime, hyper-parameter set)."""
    hp = A.HPARAMS[hp_name]
    n = sum(REGIME_SIZES)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for t in A.STEPS:
        for carried in (False, True):
            p, g, m, v = A.make_state(regime, hp_name, n, carried)
            got = step(REGIME_SIZES, p, g, m, v, hp, t)
            ref = A.step_ref(p, g, m, v, A.scalars(hp, t))
            r = _held(ref, *got, what=(t, carried))
            worst = {k: max(worst[k], r[k]) for k in worst}
            if A.is_zero_case(regime, hp_name, carried):
                # zero gradient, zero moments, no decay: exact
                assert np.array_equal(got[0].view(np.uint32), p.view(np.uint32))
                assert not got[1].any() and not got[2].any()
    _record(test="regime", regime=regime, hp=hp_name, **worst)


# ---- geometry -----------------------------------------------------------------------------------
GEO = A.geometries()
GEO_HP, GEO_T = "wd", 7


def _geo_state(n, seed=0):
    return A.make_state("unit", GEO_HP, n, True, seed)


@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "4byte"])
@pytest.mark.parametrize("name", list(GEO))
def test_geometry(name, misalign):
    sizes = GEO[name]
    hp = A.HPARAMS[GEO_HP]
    p, g, m, v = _geo_state(sum(sizes))
    got = step(sizes, p, g, m, v, hp, GEO_T, misalign=misalign)
    ref = A.step_ref(p, g, m, v, A.scalars(hp, GEO_T))
    _held(ref, *got, what=name)
    if sum(sizes):
        assert not np.array_equal(got[0], p)


def test_partition_invariance():
    """One flat state cut as 1, 3 and 300 tensors: the same bits."""
    n = 2 * A.CAP + 777
    hp = A.HPARAMS[GEO_HP]
    p, g, m, v = _geo_state(n, seed=1)
    rng = np.random.default_rng(5)
    cuts = np.sort(rng.choice(np.arange(1, n), 299, replace=False))
    many = np.diff(np.concatenate([[0], cuts, [n]])).tolist()
    assert len(many) == 300 and sum(many) == n
    one = step([n], p, g, m, v, hp, GEO_T)
    for sizes in ([A.CAP + 5, 300, n - A.CAP - 305], many):
        got = step(sizes, p, g, m, v, hp, GEO_T)
        for a, b in zip(one, got):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), len(sizes)
    _held(A.step_ref(p, g, m, v, A.scalars(hp, GEO_T)), *one, what="one tensor")


# ---- skip flag, non-finite gradients ----------------------------------------------------------------
def test_skip_flag():
    sizes = [300, A.CAP + 1, 0, 5]
    hp = A.HPARAMS[GEO_HP]
    p, g, m, v = _geo_state(sum(sizes), seed=2)
    plain = step(sizes, p, g, m, v, hp, GEO_T)
    assert not np.array_equal(plain[0], p)
    for flag in (1, 2, 3, -1):
        got = step(sizes, p, g, m, v, hp, GEO_T,
                   skip=torch.tensor([flag], dtype=torch.int32, device=DEV))
        for a, b in zip(got, (p, m, v)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), flag
    got = step(sizes, p, g, m, v, hp, GEO_T, skip=torch.zeros(1, dtype=torch.int32, device=DEV))
    for a, b in zip(got, plain):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_nonfinite_gradient_stays_in_its_element(bad):
    sizes = [300, 2 * A.CAP + 1, 5]
    at = 300 + A.CAP + 17            # the big tensor's second pass
    hp = A.HPARAMS[GEO_HP]
    p, g, m, v = _geo_state(sum(sizes), seed=3)
    clean = step(sizes, p, g, m, v, hp, GEO_T)
    g = g.copy()
    g[at] = bad
    got = step(sizes, p, g, m, v, hp, GEO_T)
    others = np.arange(g.size) != at
    for a, b in zip(got, clean):
        assert not np.isfinite(a[at]) and np.isfinite(b[at])
        assert np.array_equal(a[others].view(np.uint32), b[others].view(np.uint32))


# ---- StackAdam: a trajectory, one step ahead ----------------------------------------------------------
class ListStack(Stack):
    """A bare list of 1-d device parameters: all StackAdam asks of a stack."""
    family = "list"

    def __init__(self, arrays):
        self._params = [torch.nn.Parameter(torch.from_numpy(np.array(a, np.float32)).to(DEV))
                        for a in arrays]

    def param_count(self):
        return sum(p.numel() for p in self._params)

    def flat(self):
        return torch.cat([p.detach().reshape(-1) for p in self._params]).cpu().numpy()


def _state_of(adam):
    return adam.stack.flat(), adam._m.cpu().numpy(), adam._v.cpu().numpy()


def _traj_sizes():
    sizes = [(i * 53) % 400 + 1 for i in range(300)]
    sizes[140] = A.CAP + 1           # a second pass inside the second chunk
    return sizes


@pytest.mark.parametrize("hp_name", ["wd", "fast"])
def test_trajectory_one_step_ahead(hp_name):
    """12 consecutive StackAdam steps over 300 tensors, then t = 999 and
    t = 99999: each step's result against the restatement applied to the
    device's own previous state, so no error accumulates and every step is
    held to 2 x bound.  The sched form runs alongside on its own copy and must
    stay bitwise equal."""
    hp = A.HPARAMS[hp_name]
    lr, b1, b2, eps, wd = hp
    sizes = _traj_sizes()
    n = sum(sizes)
    rng = np.random.default_rng(9)
    p0 = rng.standard_normal(n).astype(np.float32)
    a1 = StackAdam(ListStack(A.split(p0, sizes)), lr, (b1, b2), eps, wd)
    a2 = StackAdam(ListStack(A.split(p0, sizes)), lr, (b1, b2), eps, wd)
    scales = [1.0, 1.0, 1e-4, 3e-8, 1.0, 1e-2, 1e-20, 1.0, 3e-8, 3e-8, 1e-4, 1.0, 1.0, 1.0]
    jumps = {12: 998, 13: 99998}     # the step count set before steps 13 and 14
    prev = (p0, np.zeros(n, np.float32), np.zeros(n, np.float32))
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for k, scale in enumerate(scales):
        if k in jumps:
            a1.t = a2.t = jumps[k]
        t = a1.t + 1
        g = (rng.standard_normal(n) * scale).astype(np.float32)
        gd = torch.from_numpy(g).to(DEV)
        a1.step(gd)
        sv = a2.sched_values(t)
        a2.step_sched(gd, torch.tensor(sv, dtype=torch.float32, device=DEV))
        assert a1.t == a2.t == t
        got, got2 = _state_of(a1), _state_of(a2)
        for x, y in zip(got, got2):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), ("sched", t)
        assert A.sched_scalars(hp, sv) == A.scalars(hp, t)
        r = _held(A.step_ref(prev[0], g, prev[1], prev[2], A.scalars(hp, t)), *got, what=t)
        worst = {q: max(worst[q], r[q]) for q in worst}
        prev = got
    assert a1.t == 99999
    _record(test="trajectory", hp=hp_name, **worst)


def test_desc_entry_points_against_restatement():
    """cnf_adam_step, _sched and _guarded, one step each on a small coupling
    stack (they derive the tensor list from the descriptor)."""
    from flows.flows import Flow, NvpCouplingLayer
    torch.manual_seed(0)
    stack = Flow([NvpCouplingLayer(3, [3, 3]) for _ in range(2)]).to(DEV)._native_stack()
    n = stack.param_count()
    hp = A.HPARAMS[GEO_HP]
    lr, b1, b2, eps, wd = hp
    p, g, m, v = _geo_state(n, seed=4)
    ref = A.step_ref(p, g, m, v, A.scalars(hp, GEO_T))
    lib, desc, st = _lib.lib(), ctypes.byref(stack.desc), _stream(torch.device(DEV))
    a = StackAdam.__new__(StackAdam)
    a.lr, a.betas = lr, (b1, b2)
    sched = torch.tensor(a.sched_values(GEO_T), dtype=torch.float32, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    gd = torch.from_numpy(g).to(DEV)
    calls = {
        "cnf_adam_step": lambda arr, md, vd: lib.cnf_adam_step(
            desc, arr, _ptr(gd), _ptr(md), _ptr(vd), GEO_T, lr, b1, b2, eps, wd, st),
        "cnf_adam_step_sched": lambda arr, md, vd: lib.cnf_adam_step_sched(
            desc, arr, _ptr(gd), _ptr(md), _ptr(vd), _ptr(sched), b1, b2, eps, wd, st),
        "cnf_adam_step_guarded": lambda arr, md, vd: lib.cnf_adam_step_guarded(
            desc, arr, _ptr(gd), _ptr(md), _ptr(vd), GEO_T, lr, None, b1, b2, eps, wd,
            _ptr(flag), st),
    }
    sizes = [q.numel() for q in stack.param_tensors()]
    assert sum(sizes) == n
    for name, call in calls.items():
        ps = [torch.from_numpy(x.copy()).to(DEV) for x in A.split(p, sizes)]
        md, vd = torch.from_numpy(m).to(DEV), torch.from_numpy(v).to(DEV)
        arr = (ctypes.c_void_p * len(ps))(*[q.data_ptr() for q in ps])
        _lib.check(name, call(arr, md, vd))
        torch.cuda.synchronize()
        _held(ref, torch.cat(ps).cpu().numpy(), md.cpu().numpy(), vd.cpu().numpy(), what=name)


# ---- torch on the device, as a second witness ---------------------------------------------------------
WITNESS_SIZES = [A.CAP + 1, A.BLOCK + 1, 1, 3000]
TORCH_FORMS = (("single", {"foreach": False}), ("foreach", {"foreach": True}),
               ("fused", {"fused": True}))


@pytest.mark.parametrize("hp_name", ["default", "wd"])
@pytest.mark.parametrize("regime", A.REGIMES)
def test_torch_device_steps_within_the_same_bound(regime, hp_name):
    """Step 7 from carried moments: the kernel (StackAdam.like, resuming from
    a torch optimizer's state) and torch.optim.Adam's three device forms (state
    handed over by store_into), each within 2 x bound of the restatement.  The
    count of elements whose bits differ between the kernel and each torch form
    is recorded, not judged."""
    hp = A.HPARAMS[hp_name]
    lr, b1, b2, eps, wd = hp
    n = sum(WITNESS_SIZES)
    p, g, m, v = A.make_state(regime, hp_name, n, True)
    ref = A.step_ref(p, g, m, v, A.scalars(hp, GEO_T))
    gd = torch.from_numpy(g).to(DEV)

    def seeded(**kw):
        stack = ListStack(A.split(p, WITNESS_SIZES))
        seed = StackAdam(stack, lr, (b1, b2), eps, wd)
        seed.t = GEO_T - 1
        seed._m, seed._v = torch.from_numpy(m).to(DEV), torch.from_numpy(v).to(DEV)
        opt = torch.optim.Adam(stack.param_tensors(), lr=lr, betas=(b1, b2), eps=eps,
                               weight_decay=wd, **kw)
        seed.store_into(opt)
        return stack, opt

    stack, opt = seeded()
    na = StackAdam.like(stack, opt)
    assert na.t == GEO_T - 1 and (na.lr, na.betas, na.eps, na.weight_decay) == (lr, (b1, b2), eps, wd)
    na.step(gd)
    mine = _state_of(na)
    row = {"test": "torch_witness", "regime": regime, "hp": hp_name, "n": n}
    row.update({"kernel_" + k: x for k, x in _held(ref, *mine, what="kernel").items()})
    for form, kw in TORCH_FORMS:
        try:
            stack, opt = seeded(**kw)
        except RuntimeError as e:      # this torch build has no fused Adam for the device
            assert form == "fused", e
            row[form] = None
            continue
        ps = stack.param_tensors()
        if form == "fused":            # the fused kernel reads the step count on the device
            for q in ps:
                opt.state[q]["step"] = opt.state[q]["step"].to(DEV)
        for q, gq in zip(ps, stack.split(gd)):
            q.grad = gq.clone()
        opt.step()
        torch.cuda.synchronize()
        assert all(int(opt.state[q]["step"]) == GEO_T for q in ps)
        theirs = (stack.flat(),
                  torch.cat([opt.state[q]["exp_avg"].reshape(-1) for q in ps]).cpu().numpy(),
                  torch.cat([opt.state[q]["exp_avg_sq"].reshape(-1) for q in ps]).cpu().numpy())
        r = _held(ref, *theirs, what=form)
        row.update({"%s_%s" % (form, k): x for k, x in r.items()})
        for k, a, b in zip("pmv", mine, theirs):
            row["%s_bits_differ_%s" % (form, k)] = int(np.count_nonzero(
                a.view(np.uint32) != b.view(np.uint32)))
    _record(**row)
