"""k_sgpr's tile loop at the shapes where its prologue, epilogue and argument
handling can go wrong: the fused eval call (cnf_forward_loss through the C ABI,
as bench.Runner.step makes it) at D=10, hidden [5,5], L in {5, 6} (5: the odd
stack's lone layer runs first, on a row read reversed) and batches that are
ragged only, one full 128-row tile, a full tile plus a ragged one, several
tiles, and one batch long enough that a wave owns more than one tile (the
kernel reads out / ld / y / kind / det and the next tile's input pointer from
the argument block at each tile boundary).

References: k_valu (the same call with OPT_NO_SGPR) at the tolerance
tests/test_gpu_parity.py holds the two paths to; the fp64 oracle on z and the
log-det at 1e-5; an fp64 restatement of the reference's loss terms
(calibrators.py:287-291; the CE kind: run_experiment3D.py:107) over the rows,
each sum bounded by 1e-5 * sum of the per-row magnitudes of that term."""
import ctypes

import numpy as np
import pytest
import torch

import bench
from _golden import rel_err
from cnf_hip import _lib
from oracle import cnf_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5
DEV = "cuda:0"
D = 10
BS = (1, 2, 127, 128, 129, 256, 128 * 9 + 5)
BMAX = max(BS)
CAL, CE = 0, 1


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    yield


class _Case:
    """One flow (both kernel families over the same weights), BMAX rows of
    synthetic logits and labels, and their fp64 references."""

    def __init__(self, L):
        w = {"D": D, "hidden": [5, 5], "scale": True, "L": L}
        self.flow = bench.make_flow(w, torch.device(DEV))
        self.sgpr = self.flow._native_stack()
        assert self.sgpr.kernel_name() == "sgpr-fused"
        valu_flow = bench.make_flow(w, torch.device(DEV))
        valu_flow.native_options = _lib.OPT_NO_SGPR
        self.valu = valu_flow._native_stack()
        assert self.valu.kernel_name() == "valu-fused"
        self._keep = valu_flow
        self.x, self.y = bench.synthetic_logits(BMAX, D, torch.device(DEV), 77 + L)
        st = {k: v.detach().cpu().numpy() for k, v in self.flow.state_dict().items()}
        layers = O.layers_from_state(st, L, D, 3, True, True)
        zs, ld = O.flow_forward(layers, self.x.cpu().numpy().astype(np.float64))
        self.z64 = np.asarray(zs[-1], dtype=np.float64)
        self.ld64 = np.asarray(ld, dtype=np.float64).reshape(-1)

    def ref_terms(self, B, kind, det):
        """Per-row (loss, ce, ld) in fp64, calibrators.py:287-291 restated."""
        z, ld = self.z64[:B], self.ld64[:B]
        y = self.y[:B].cpu().numpy()
        zs = z - z.max(axis=1, keepdims=True)
        lsm = zs - np.log(np.exp(zs).sum(axis=1, keepdims=True))
        lpy = lsm[np.arange(B), y]
        if kind == CAL:
            ce = -np.log(np.exp(lpy) + 1e-7)
            loss = ce - ld
        else:
            ce = -lpy
            loss = ce - det * ld
        return np.stack([loss, ce, ld])


_cases = {}


def _case(L):
    if L not in _cases:
        _cases[L] = _Case(L)
    return _cases[L]


def _ptr(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset if t is not None else 0)


def _call(stack, x, y, kind, det, want=True, ld_off=0, y_off=0):
    """cnf_forward_loss through the C ABI.  ld_off / y_off: byte offsets of the
    log-det / label pointers from a 16-B aligned allocation."""
    B = x.shape[0]
    dev = x.device
    lib = _lib.lib()
    desc = ctypes.byref(stack.desc)
    n = ctypes.c_size_t()
    assert lib.cnf_forward_loss_workspace_bytes(desc, ctypes.c_int64(B), ctypes.byref(n)) == 0
    ws = torch.zeros(max(n.value, 16), dtype=torch.uint8, device=dev)
    terms = torch.full((3,), 7.0, device=dev)
    z = torch.full((B, D), 7.0, device=dev) if want else None
    ldbuf = torch.full((B + 4,), 7.0, device=dev) if want else None
    ybuf = torch.zeros(B + 2, dtype=torch.int64, device=dev)
    assert ybuf.data_ptr() % 16 == 0 and (ldbuf is None or ldbuf.data_ptr() % 16 == 0)
    ybuf[y_off // 8:y_off // 8 + B] = y
    blob = stack.prepared(dev)
    st = lib.cnf_forward_loss(desc, _ptr(blob), _ptr(x), _ptr(ybuf, y_off), ctypes.c_int32(kind),
                              ctypes.c_float(det), _ptr(z), _ptr(ldbuf, ld_off), _ptr(terms),
                              ctypes.c_int64(B), _ptr(ws), ctypes.c_size_t(n.value),
                              ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert st == 0, st
    torch.cuda.synchronize(dev)
    ld = ldbuf[ld_off // 4:ld_off // 4 + B] if want else None
    if want:  # nothing written past the rows
        assert torch.all(ldbuf[ld_off // 4 + B:] == 7.0) and torch.all(ldbuf[:ld_off // 4] == 7.0)
    return terms, z, ld


def _check_sums(got, rows, what):
    """Each sum within 1e-5 * sum of its per-row magnitudes of the fp64 sum."""
    got = got.double().cpu().numpy()
    ref = rows.sum(axis=1)
    bound = 1e-5 * np.abs(rows).sum(axis=1)
    print(what, "sums", got, "ref", ref, "err", np.abs(got - ref), "bound", bound)
    assert np.all(np.abs(got - ref) <= bound), (what, got, ref, bound)


@pytest.mark.parametrize("L", [5, 6])
@pytest.mark.parametrize("B", BS)
def test_loss_call_matches_valu_oracle_and_fp64_terms(L, B):
    c = _case(L)
    x, y = c.x[:B], c.y[:B]
    for kind, det in ((CAL, 1.0), (CE, 0.5)):
        t, z, ld = _call(c.sgpr, x, y, kind, det)
        # the k_valu path: the tolerance test_gpu_parity.py holds the two paths to
        tv, zv, ldv = _call(c.valu, x, y, kind, det)
        assert rel_err(z.cpu().numpy(), zv.cpu().numpy()) <= TOL
        assert rel_err(ld.cpu().numpy(), ldv.cpu().numpy()) <= TOL
        # the fp64 oracle
        assert rel_err(z.cpu().numpy(), c.z64[:B]) <= TOL
        assert rel_err(ld.cpu().numpy(), c.ld64[:B]) <= TOL
        rows = c.ref_terms(B, kind, det)
        _check_sums(t, rows, "sgpr L=%d B=%d kind=%d" % (L, B, kind))
        _check_sums(tv, rows, "valu L=%d B=%d kind=%d" % (L, B, kind))
        # out and ld null: the same sums (the loss never depends on the stores)
        tn, _, _ = _call(c.sgpr, x, y, kind, det, want=False)
        assert torch.equal(tn, t)
        # repeatable to the bit
        t2, z2, ld2 = _call(c.sgpr, x, y, kind, det)
        assert torch.equal(t2, t) and torch.equal(z2, z) and torch.equal(ld2, ld)


@pytest.mark.parametrize("L", [5, 6])
@pytest.mark.parametrize("row", [5, 128])  # B = 129: in the full tile / in the ragged tile
def test_invalid_label_poisons_the_sums_only(L, row):
    """y = D: the loss and ce sums are NaN; the log-det sum, which no label
    enters, keeps its bits (tests/test_gpu_parity.py pins it finite), and so do
    z and the log-det."""
    c = _case(L)
    B = 129
    x, y = c.x[:B], c.y[:B].clone()
    t0, z0, ld0 = _call(c.sgpr, x, y, CAL, 1.0)
    assert torch.isfinite(t0).all()
    y[row] = D
    for kind in (CAL, CE):
        t, z, ld = _call(c.sgpr, x, y, kind, 0.5)
        assert torch.isnan(t[0]) and torch.isnan(t[1]), t
        assert torch.equal(t[2], t0[2])
        assert torch.equal(z, z0) and torch.equal(ld, ld0)


@pytest.mark.parametrize("L", [5, 6])
def test_misaligned_logdet_and_label_pointers(L):
    c = _case(L)
    B = 2 * 128 + 5  # full tiles and a ragged one
    x, y = c.x[:B], c.y[:B]
    t0, z0, ld0 = _call(c.sgpr, x, y, CAL, 1.0)
    t1, z1, ld1 = _call(c.sgpr, x, y, CAL, 1.0, ld_off=4)
    assert torch.equal(t1, t0) and torch.equal(z1, z0) and torch.equal(ld1, ld0)
    t2, z2, ld2 = _call(c.sgpr, x, y, CAL, 1.0, y_off=8)
    assert torch.equal(t2, t0) and torch.equal(z2, z0) and torch.equal(ld2, ld0)


def test_waves_that_own_several_tiles():
    """2^20 + 130 rows: every wave of the persistent grid walks two tiles or
    more (next-tile DMA, per-tile argument reads) and the last tile is ragged.
    Against k_valu on the device; sums against fp64 sums of k_valu's z / ld."""
    c = _case(6)
    B = (1 << 20) + 130
    x, y = bench.synthetic_logits(B, D, torch.device(DEV), 5)
    t, z, ld = _call(c.sgpr, x, y, CAL, 1.0)
    tv, zv, ldv = _call(c.valu, x, y, CAL, 1.0)
    assert ((z - zv).abs() / (zv.abs() + 1)).max().item() <= TOL
    assert ((ld - ldv).abs() / (ldv.abs() + 1)).max().item() <= TOL
    lsm = torch.log_softmax(zv.double(), dim=1)
    ce = -torch.log(torch.exp(lsm.gather(1, y.view(-1, 1)).squeeze(1)) + 1e-7)
    # (k_valu's fp32 z, ld carry up to TOL * (|v| + 1) per row themselves)
    rows = torch.stack([ce - ldv.double(), ce, ldv.double()]).cpu().numpy()
    got = t.double().cpu().numpy()
    bound = 1e-5 * (np.abs(rows) + 1).sum(axis=1)
    assert np.all(np.abs(got - rows.sum(axis=1)) <= bound), (got, rows.sum(axis=1), bound)
    t2, z2, ld2 = _call(c.sgpr, x, y, CAL, 1.0)
    assert torch.equal(t2, t) and torch.equal(z2, z) and torch.equal(ld2, ld)
    tn, _, _ = _call(c.sgpr, x, y, CAL, 1.0, want=False)
    assert torch.equal(tn, t)
