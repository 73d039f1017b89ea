"""The mixed planar / radial / affine family without a GPU: the C ABI
(symbols, parameter counts, every argument error and the order of the checks,
the workspace and the launch plan), the float64 restatement against the
reference's record, the dispatch rule of flows.flows, the log-det shape rule
against the CPU layer loop, MixedFlow and pickling.

Every launching call below carries at least one fault, so it returns before
any HIP call; the pointers are fake (the fault table is
tests/test_rowflow_args_cpu.py's, of which mixed is the fourth family)."""
import ctypes
import itertools
import os
import pickle

import numpy as np
import pytest
import torch

import _mixed_ref as M
import _rowsweep as S
import test_rowflow_args_cpu as T
from _golden import rel_err
from cnf_hip import _lib, engine, mixed
from cnf_hip.mixed import MixedStack
from flows import flows as FL
from flows.flows import AffineConstantLayer, Flow, NvpCouplingLayer, PlanarLayer, RadialLayer
from test_gpu_vjp import _grad_err

P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_NAMES = ("forward", "forward_loss", "predict", "score", "vjp", "loss_vjp")
LAYER = {"P": PlanarLayer, "R": RadialLayer, "A": AffineConstantLayer}


def make(order, D=3):
    return [LAYER[c](D) for c in order]


# ---- C ABI: symbols and counts ----------------------------------------------------------

def test_exports_match_header():
    names = [n for n in _lib.EXPORTS if n.startswith("cnf_mixed_")]
    assert sorted(names) == sorted("cnf_mixed_" + s for s in (
        "param_count", "workspace_bytes", "launch_plan") + ENTRY_NAMES)
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in names)
    src = open(os.path.join(ROOT, "include", "cnf.h")).read()
    for line in ("#define CNF_LAYER_PLANAR 0", "#define CNF_LAYER_RADIAL 1",
                 "#define CNF_LAYER_AFFINE 2", "#define CNF_MIXED_MAX_LAYERS 64",
                 "#define CNF_ABI_VERSION 2"):
        assert line in src
    assert all("int %s(" % n in src for n in names)
    assert (_lib.LAYER_PLANAR, _lib.LAYER_RADIAL, _lib.LAYER_AFFINE) == (0, 1, 2)
    assert _lib.MIXED_MAX_LAYERS == 64 and lib.cnf_abi_version() == 2
    assert M.KIND == {"P": 0, "R": 1, "A": 2} and mixed.KIND == {M.FAMILY[k]: v
                                                                for k, v in M.KIND.items()}
    assert all("mixed_" + k in engine.stats
               for k in ("forward", "vjp", "loss_vjp", "predict", "score"))


@pytest.mark.parametrize("order,D", [("PRA", 3), ("PRPRPRPRPA", 10), ("AP", 2), ("P", 5), ("RR", 7),
                                     ("A" * 64, 256), ("PAR" * 21, 1)])
def test_param_count_matches_state_dict(order, D):
    flow = Flow(make(order, D))
    kinds = [M.KIND[c] for c in order]
    want = sum(M.grad_floats(c, D) for c in order)
    assert mixed.param_count(D, kinds) == sum(p.numel() for p in flow.parameters()) == want
    st = MixedStack(list(flow.layers))
    assert st.param_count() == want and st.kinds == kinds and st.dim == D and st.L == len(order)
    # ABI order = state_dict order
    assert [id(p) for p in st.param_tensors()] == [id(p) for p in flow.parameters()]


def _kinds(vals):
    return (I32 * len(vals))(*vals)


@pytest.mark.parametrize("D,L,status", [(0, 1, -2), (3, 0, -2), (-1, 1, -2), (257, 1, -3),
                                        (3, 65, -3), (256, 64, 0), (1, 1, 0)])
def test_envelope(D, L, status):
    lib = _lib.lib()
    n, b = I64(), ctypes.c_size_t()
    out = (I32 * 8)()
    k = _kinds([i % 3 for i in range(max(L, 1))])
    assert lib.cnf_mixed_param_count(I32(D), I32(L), k, ctypes.byref(n)) == status
    assert lib.cnf_mixed_workspace_bytes(I32(D), I32(L), k, I64(8), ctypes.byref(b)) == status
    assert lib.cnf_mixed_launch_plan(I32(D), I32(L), k, I64(8), out) == status


def test_query_argument_errors():
    lib = _lib.lib()
    n, b = I64(), ctypes.c_size_t()
    out = (I32 * 8)()
    good = _kinds([0, 1, 2])
    d, l = I32(3), I32(3)
    assert lib.cnf_mixed_param_count(d, l, good, None) == -1
    assert lib.cnf_mixed_workspace_bytes(d, l, good, I64(8), None) == -1
    assert lib.cnf_mixed_launch_plan(d, l, good, I64(8), None) == -1
    for fn, tail in ((lib.cnf_mixed_param_count, (ctypes.byref(n),)),
                     (lib.cnf_mixed_workspace_bytes, (I64(8), ctypes.byref(b))),
                     (lib.cnf_mixed_launch_plan, (I64(8), out))):
        assert fn(d, l, None, *tail) == -1
        assert fn(d, l, _kinds([0, 1, 3]), *tail) == -2
        assert fn(d, l, _kinds([-1, 1, 2]), *tail) == -2
        assert fn(I32(300), l, None, *tail) == -3            # the shape first
        assert fn(d, l, _kinds([2, 2, 2]), *tail) == 0       # a single kind is valid
    for fn, tail in ((lib.cnf_mixed_workspace_bytes, (ctypes.byref(b),)),
                     (lib.cnf_mixed_launch_plan, (out,))):
        assert fn(d, l, good, I64(-1), *tail) == -4
        assert fn(d, l, good, I64((1 << 31) + 1), *tail) == -4
        assert fn(d, l, _kinds([0, 9, 0]), I64(-1), *tail) == -2   # kinds before the batch
        assert fn(d, l, good, I64(1 << 31), *tail) == 0
    assert lib.cnf_mixed_launch_plan(d, l, good, I64(0), out) == 0 and list(out)[5:] == [1, 1, 1]


# ---- C ABI: every argument error of every entry point, and their order -----------------------

# The table is tests/test_rowflow_args_cpu.py's, where mixed is the fourth family
# (its head carries `kinds`, its packed table has 3 + 2 entries); its mixed rows
# run here under the ids they have always had.
KINDS = T.KINDS
CASES = [(entry, fs, st) for fam, entry, fs, st in T.CASES if fam == "mixed"]
IDS = ["%s-%s" % (entry, "+".join(fs)) for entry, fs, _ in CASES]


@pytest.mark.parametrize("entry,faults,status", CASES, ids=IDS)
def test_status_and_precedence(entry, faults, status):
    assert T.L == len(KINDS) and T.call("mixed", entry, faults) == status


def test_table_covers_every_entry_point_and_fault():
    assert len(IDS) == len(set(IDS))
    assert {f for _, fs, _ in CASES for f in fs} == set(T.FAULTS)
    assert {fs for _, fs, _ in CASES if len(fs) == 2} == set(T.PAIRS)
    for entry in ENTRY_NAMES:
        mine = {fs for e, fs, _ in CASES if e == entry}
        assert {("kinds_null",), ("kinds_bad_first",), ("kinds_bad_last",), ("dim_big", "kinds_null"),
                ("kinds_null", "batch_neg"), ("kinds_bad_last", "batch_neg"), ("table_null",),
                ("entry_null_last",), ("entry_mis_last",), ("ws_short",), ("x_mis",)} <= mine
        assert (("kinds_null", "bins_zero") in mine) == (entry == "score")
        assert (("grads_null",) in mine) == ("vjp" in entry)


def test_packed_table_is_read_to_its_last_entry():
    """3 + 2 entries for planar + affine: a fault in entry 4 is seen, and the
    same table under kinds = [2, 2] (4 entries) is not read past entry 3."""
    lib = _lib.lib()
    ws = mixed.workspace_bytes(T.D, KINDS, T.B)

    def fwd(kinds, table, x=16):
        return lib.cnf_mixed_forward(I32(T.D), I32(2), _kinds(kinds), (P * len(table))(*table),
                                     P(x), P(16), P(16), P(0), I64(T.B), P(16),
                                     ctypes.c_size_t(ws), P(0))
    good = [4096 + 64 * i for i in range(5)]
    assert fwd([0, 2], good[:4] + [0]) == -1 and fwd([2, 0], good[:4] + [4098]) == -6
    # entry 4 unread under 2 + 2 entries: the later fault (x null) shows instead
    assert fwd([2, 2], good[:4] + [4098], x=0) == -1 and fwd([0, 2], good[:4] + [4098], x=0) == -6
    assert fwd([0, 1], good + [4098]) == -6              # 3 + 3 entries


@pytest.mark.parametrize("entry", ["forward", "predict", "score"])
def test_empty_batch_without_outputs_needs_no_device(entry):
    names, nt = T.names("mixed", entry), T.N_TABLE["mixed"]
    vals = dict(T.GOOD, B=0, wb=0, record=16, kinds=_kinds(KINDS),
                params=(P * nt)(*[4096 + 64 * i for i in range(nt)]))
    args = [vals[n] if n in ("params", "kinds") else T.CTYPES.get(n, P)(vals.get(n, 0))
            for n in names]
    assert getattr(_lib.lib(), "cnf_mixed_" + entry)(*args) == 0


# ---- workspace and launch plan ---------------------------------------------------------------

@pytest.mark.parametrize("D,L", [(1, 1), (3, 3), (3, 18), (10, 10), (10, 11), (11, 10), (16, 64),
                                 (17, 3), (23, 64), (64, 48), (100, 4), (153, 10), (256, 64)])
@pytest.mark.parametrize("B", [0, 1, 63, 256, 257, 777, 65537, 1 << 20])
def test_workspace_and_plan_match_the_restated_plan(D, L, B):
    kinds = [i % 3 for i in range(L)]
    assert mixed.workspace_bytes(D, kinds, B) == 4 * M.workspace_floats(D, L, B)
    assert mixed.launch_plan(D, kinds, B) == M.expected_plan(D, L, max(B, 1))
    # neither depends on the kinds
    assert mixed.launch_plan(D, [2] * L, B) == mixed.launch_plan(D, kinds, B)
    assert mixed.workspace_bytes(D, [1] * L, B) == mixed.workspace_bytes(D, kinds, B)


def test_constants_the_restated_plan_mirrors():
    src = open(os.path.join(ROOT, "calibration-normalizing-flows_amd", "csrc",
                            "cnf_mixed.hip")).read()
    assert "constexpr int kAccD = %d;" % M.ACC_D in src
    assert "constexpr int kSeg = %d;" % M.SEG in src
    assert "geometry(D, L, 2 * padded_dim(D) + 8, 2 * D + 2, 0)" in src
    assert "const bool regt = L <= kRegL && (lpr != 1 || cpl <= kAccD);" in src
    assert "return {regt, regt && lpr == 1};" in src


# ---- the restatement and the record ----------------------------------------------------------

@pytest.mark.parametrize("name", M.FIXTURES)
def test_restatement_matches_the_reference_record(name):
    d = M.load(name)
    ps = M.params_of(d)
    B = d["x"].shape[0]
    zs, ld = M.forward(ps, d["x"])
    assert rel_err(zs, d["zs64"]) <= 1e-12
    assert rel_err(ld, np.asarray(d["ld64"]).reshape(-1) * np.ones(B)) <= 1e-12
    assert rel_err(M.predict(ps, d["x"], d["log_priors"]), d["probs64"]) <= 1e-12
    for kind, det in (("cal", 1.0), ("ce", float(d["det"]))):
        t, g, _ = M.loss_vjp(ps, d["x"], d["y"], kind, det, 1.0 / B)
        ref = float(d["loss_%s_64" % kind])
        assert abs(t[0] / B - ref) <= 1e-12 * (abs(ref) + 1)
        assert _grad_err(g, d["g_%s_64" % kind]) <= 1e-10
    # the recorded floors leave three quarters of each bar
    assert max(float(d["floor_zs"]), float(d["floor_ld"]), float(d["floor_probs"])) <= S.OUT_COND
    assert max(float(d["floor_g_cal"]), float(d["floor_g_ce"])) <= S.GRAD_COND


def test_fixture_shapes():
    want = {"pra": ("PRA", 3, 777), "d10": ("PRPRPRPRPA", 10, 777), "deep": ("PRA" * 6, 3, 300),
            "contract": ("PAPR", 10, 300), "d17": ("PAR", 17, 130), "d100": ("PRAP", 100, 70),
            "ar": ("ARA", 4, 50), "one": ("AP", 2, 1)}
    assert sorted(want) == sorted(M.FIXTURES)
    for name, (order, D, B) in want.items():
        d = M.load(name)
        assert M.order_of(d) == order and d["x"].shape == (B, D)
        assert tuple(d["ld"].shape) == ((1,) if name in ("ar", "one") else (B,))
    c = M.params_of(M.load("contract"))
    assert (c[1][1][0] == -6).all() and (c[1][1][1] == 3).all()
    assert len(M.order_of(M.load("deep"))) == M.SEG + 2


def test_restatement_upstream_gradients_match_autograd():
    d = M.load("d17")
    ps = M.params_of(d)
    flow = M.build_flow(ps).double()
    rs = np.random.RandomState(5)
    L, B, D = d["zs"].shape
    gz_all, gld = rs.standard_normal((L, B, D)), rs.standard_normal(B)
    x = torch.from_numpy(d["x"]).double().requires_grad_(True)
    zs, ld = flow(x)
    obj = (torch.stack(zs) * torch.from_numpy(gz_all)).sum() + (ld * torch.from_numpy(gld)).sum()
    res = torch.autograd.grad(obj, list(flow.parameters()) + [x])
    ref = torch.cat([g.reshape(-1) for g in res[:-1]]).numpy()
    grads, dx = M.vjp(ps, d["x"], gz_all=gz_all, gld=gld)
    assert _grad_err(grads, ref) <= 1e-10 and _grad_err(dx, res[-1].numpy()) <= 1e-10


@pytest.mark.parametrize("name", M.FIXTURES)
def test_cpu_flow_matches_reference(name):
    d = M.load(name)
    flow = M.build_flow(M.params_of(d))
    n0 = dict(engine.stats)
    with torch.no_grad():
        zs, ld = flow(torch.from_numpy(d["x"]))
    assert engine.stats == n0                         # host tensors stay on torch ops
    assert tuple(ld.shape) == tuple(d["ld"].shape)
    assert rel_err(torch.stack(zs).numpy(), d["zs"]) <= 1e-6
    assert rel_err(ld.numpy(), d["ld"]) <= 1e-6


# ---- dispatch --------------------------------------------------------------------------------

def test_family_switch_and_binding():
    assert FL.MIXED_NATIVE is True and "_mstack" in FL.Flow._BINDINGS
    assert MixedStack.family == "mixed" and MixedStack.slot == "_mstack"
    assert MixedStack.squeeze_logdet is False and not MixedStack.has_inverse


def test_host_tensors_stay_on_the_loop():
    layers = make("PRA")
    x = torch.randn(5, 3)
    assert FL._row_class(layers, x) is None
    n0 = dict(engine.stats)
    with torch.no_grad():
        Flow(layers)(x)
    assert engine.stats == n0


def test_dispatch_rule(monkeypatch):
    """With the device test answered yes for host rows (there is no GPU here)
    and host parameters, everything else of the rule runs as on a device."""
    monkeypatch.setattr(FL, "_device_rows", lambda x: torch.is_tensor(x) and x.dim() == 2
                        and x.dtype == torch.float32)
    x = torch.randn(5, 3)
    pick = lambda layers, rows=x: FL._row_class(layers, rows)
    assert pick(make("PRA")) is MixedStack and pick(make("PA")) is MixedStack
    assert pick(make("PRPRPRPRPA")) is MixedStack
    # a single family still takes its own stack
    assert pick(make("PPP")).family == "planar" and pick(make("RR")).family == "radial"
    assert pick(make("AA")).family == "affine" and pick(make("P")).family == "planar"
    # ineligible layers
    assert pick(make("PR") + [AffineConstantLayer(3, scale=False)]) is None
    assert pick(make("PR") + [AffineConstantLayer(3, shift=False)]) is None
    assert pick(make("PR") + [NvpCouplingLayer(3)]) is None
    assert pick(make("P") + [RadialLayer(4)]) is None                      # widths differ
    assert pick(make("PRA"), torch.randn(5, 4)) is None                    # not the input's width
    assert pick(make("PRA"), torch.randn(5, 3).double()) is None
    assert pick([PlanarLayer(3), RadialLayer(3).double()]) is None
    # orders the loop rejects, and the radial first layer (a host log-det)
    assert pick(make("AP")) is None and pick(make("AP"), x[:1]) is MixedStack
    assert pick(make("PA"), x[:1]) is None
    assert pick(make("RP")) is None and pick(make("RP"), x[:1]) is None
    assert pick(make("AR")) is MixedStack and pick(make("AR"), x[:0]) is None
    assert pick(make("PA"), x[:0]) is MixedStack
    # the switches: the mixed one, and each family present
    monkeypatch.setattr(FL, "MIXED_NATIVE", False)
    assert pick(make("PRA")) is None and pick(make("PPP")).family == "planar"
    monkeypatch.setattr(FL, "MIXED_NATIVE", True)
    for name, order in (("PLANAR_NATIVE", "PR"), ("RADIAL_NATIVE", "PR"), ("AFFINE_NATIVE", "PA")):
        monkeypatch.setattr(FL, name, False)
        assert pick(make(order)) is None
        monkeypatch.setattr(FL, name, True)
    monkeypatch.setattr(FL, "RADIAL_NATIVE", False)
    assert pick(make("PA")) is MixedStack                                   # no radial layer in it


def test_compatible():
    ok = make("PRA", 5)
    assert MixedStack.compatible(ok) and MixedStack.compatible(ok, "cpu")
    assert not MixedStack.compatible(ok, "cuda:0")            # parameters sit on the host
    assert not MixedStack.compatible([])
    assert not MixedStack.compatible(ok + [PlanarLayer(4)])
    assert not MixedStack.compatible(ok + [NvpCouplingLayer(5)])
    assert not MixedStack.compatible(ok + [AffineConstantLayer(5, scale=False)])
    assert not MixedStack.compatible(ok + [RadialLayer(5).double()])
    assert MixedStack.compatible(make("PP", 5))               # a single kind is a valid stack


ORDERS = ["".join(o) for n in (2, 3) for o in itertools.product("PRA", repeat=n)
          if len(set(o)) > 1]


@pytest.mark.parametrize("B", [0, 1, 2])
@pytest.mark.parametrize("order", ORDERS)
def test_logdet_shape_rule_is_the_loops(order, B):
    """eligible <=> the CPU layer loop does not raise, and then with its shape."""
    torch.manual_seed(1)
    layers = make(order)
    x = torch.randn(B, 3)
    want = FL.mixed_logdet_shape(layers, B)
    try:
        with torch.no_grad():
            _, ld = Flow(layers)(x)
        got = tuple(ld.shape)
    except RuntimeError:
        got = None
    assert want == got, (order, B, want, got)


def test_logdet_shape_examples():
    shape = lambda o, B: FL.mixed_logdet_shape(make(o), B)
    assert shape("PA", 2) == (2,) and shape("PA", 1) is None
    assert shape("AP", 1) == (1,) and shape("AP", 2) is None
    assert shape("AR", 2) == (1,) and shape("AR", 1) == (1,)
    assert shape("RA", 2) is None and shape("RP", 2) is None
    assert shape("PRA", 777) == (777,)
    assert len(ORDERS) == 6 + 24


# ---- the factory and pickling ----------------------------------------------------------------

def test_mixed_flow_spec():
    from flows.normalizing_flows_torch import MixedFlow
    flow = MixedFlow(4)
    assert flow.spec == "PRPRA" and flow.dim == 4
    assert [type(ly) for ly in flow.layers] == [LAYER[c] for c in "PRPRA"]
    assert [type(ly) for ly in MixedFlow(2, layers="arp").layers] == [LAYER[c] for c in "ARP"]
    assert MixedFlow(3, layers="PA", epochs=5, dev="cpu").spec == "PA"     # the calibrator's kwargs
    for bad in ("", "PX", "P R", 3):
        with pytest.raises(ValueError):
            MixedFlow(3, layers=bad)
    x = torch.randn(6, 4)
    with torch.no_grad():
        z, ld = flow(x)
        zs, ld2 = flow.forward_all(x)
    assert z.shape == (6, 4) and ld.shape == (6,) and torch.equal(z, zs[-1]) and len(zs) == 5
    assert list(flow.state_dict())[:6] == ["layers.0.w", "layers.0.u", "layers.0.b",
                                           "layers.1.z0", "layers.1.a", "layers.1.b"]
    assert list(flow.state_dict())[-2:] == ["layers.4.s", "layers.4.t"]


def test_pickle_round_trip():
    from flows.normalizing_flows_torch import MixedFlow
    flow = MixedFlow(4, layers="PRA")
    x = torch.randn(5, 4)
    with torch.no_grad():
        z, ld = flow(x)
    flow._mstack = object()                           # a binding must not travel
    flow._mstack_key = [1]
    back = pickle.loads(pickle.dumps(flow))
    assert back._mstack is None and back._mstack_key is None and back.spec == "PRA"
    with torch.no_grad():
        z2, ld2 = back(x)
    assert torch.equal(z, z2) and torch.equal(ld, ld2)


def test_cpu_calibrator_fit_matches_reference_run():
    """The CPU loop (the reference's own, on torch ops) around MixedFlow from
    the same seed: the reference's init draw, history, parameters and predict."""
    import calibrators as C
    from flows.normalizing_flows_torch import MixedFlow
    for name in ("full", "mb128"):
        d = M.load_cal(name)
        tol = 1e-5
        assert str(d["order"]) == "PRPRA" and d["logits"].shape == (300, 3)
        torch.manual_seed(int(d["seed"]))
        n0 = dict(engine.stats)
        cal = C.TorchFlowCalibrator(MixedFlow, d["logits"], np.eye(3)[d["labels"]],
                                    layers=str(d["order"]), epochs=int(d["epochs"]),
                                    batch_size=int(d["batch_size"]), dev=torch.device("cpu"))
        assert engine.stats == n0
        for k in ("loss", "ce", "log_det"):
            got = np.array([float(v) for v in cal.history[k]])
            assert np.max(np.abs(got - d[k]) / (np.abs(d[k]) + 1)) <= tol, k
        got = torch.cat([p.detach().reshape(-1) for p in cal.flow.parameters()]).numpy()
        assert np.max(np.abs(got - d["P"])) <= tol
        steps = int(d["epochs"]) * -(-300 // int(d["batch_size"]))
        assert np.max(np.abs(d["P"] - d["P64"])) <= steps * 1e-3 * 2e-2 / 4
        assert np.max(np.abs(cal.predict(d["held"]) - d["pred"])) <= tol
