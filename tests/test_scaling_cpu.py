"""The scaling calibrators without a GPU: the drop-in signatures, the float64
restatement (tests/_scaling_ref.py) and the host path against the reference's
own recorded objective / gradient values and predictions
(tests/golden/scaling/*.npz, written by gen_golden_scaling.py), the host fits,
and the argument validation of the four cnf_scaling_* entry points."""
import ctypes
import inspect

import numpy as np
import pytest

import _scaling_ref as R
from cnf_hip import _lib

CLS = {"temp": "TempScalingCalibrator", "mlr": "MLRCalibrator",
       "vec": "VectorScalingCalibrator", "mat": "MatrixScalingCalibrator"}
GTOL = 1e-5 + 1e-10  # SciPy CG's gtol, the criterion the reference's own successful fit meets


@pytest.fixture(scope="module")
def fx():
    return {n: R.load(n) for n in R.FIXTURES}


def test_dropin_signatures():
    import calibrators as C
    from utils.ops import optim_temperature
    for name in CLS.values():
        cls = getattr(C, name)
        assert issubclass(cls, C.Calibrator)
        assert list(inspect.signature(cls.__init__).parameters) == ["self", "logits", "target"]
    sig = inspect.signature(optim_temperature)
    assert list(sig.parameters) == ["logits", "target", "method", "min_diff", "step"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == ["newton", 1e-6, 0.01]


def _ref_sums_fn(f):
    return lambda kind, a, b: R.sums(f["x"], f["y"], kind, a, b)


def _host_sums_fn(f):
    from utils.ops import scaling_sums_host
    onehot = np.eye(f["x"].shape[1])[f["y"]]

    def fn(kind, a, b):
        s = scaling_sums_host(f["x"].astype(np.float64), onehot, kind, a, b)
        return s, R.sums(f["x"], f["y"], kind, a, b)[1]
    return fn


@pytest.mark.parametrize("path", ["restatement", "host"])
@pytest.mark.parametrize("name", R.CLASSES)
@pytest.mark.parametrize("fixture", R.FIXTURES)
def test_recorded_probes(fx, fixture, name, path):
    """Every recorded `fun` / `jac` value of the reference, rebuilt from the
    raw sums, within EVAL_TOL * sum|terms|."""
    f = fx[fixture]
    B, D = f["x"].shape
    fn = _ref_sums_fn(f) if path == "restatement" else _host_sums_fn(f)
    fun, jac, fun_s, jac_s = R.forms(name, fn, B, D)
    for i, x in enumerate(f[name + "_probe_x"]):
        R.assert_close(fun(x), f[name + "_probe_fun"][i], fun_s(x), B, (fixture, name, i, "fun"))
        R.assert_close(jac(x), f[name + "_probe_jac"][i], jac_s(x), B, (fixture, name, i, "jac"))


def _inject(cal, name, x, D):
    if name == "temp":
        cal.T = float(x[0])
    elif name == "mlr":
        cal.alpha, cal.gamma = float(x[0]), x[1:].copy()
    elif name == "vec":
        cal.b, cal.W = x[:D].copy(), x[D:].copy()
    else:
        cal.b, cal.W = x[:D].copy(), x[D:].reshape(D, D).copy()


def _bare(name, f):
    """An instance with the base state of (x, y) and no fit."""
    import calibrators as C
    cls = getattr(C, CLS[name])
    cal = cls.__new__(cls)
    C.Calibrator.__init__(cal, f["x"].astype(np.float64), f["y"])
    return cal


# s3 records no matrix fit (10,100 parameters): probes only
FITTED = [(fixture, name) for fixture in R.FIXTURES for name in R.CLASSES
          if (fixture, name) != ("s3", "mat")]


@pytest.mark.parametrize("fixture,name", FITTED)
def test_host_predict_with_recorded_parameters(fx, fixture, name):
    f = fx[fixture]
    D = f["x"].shape[1]
    cal = _bare(name, f)
    _inject(cal, name, f[name + "_x"], D)
    got = cal.predict(f["held"].astype(np.float64))
    assert got.dtype == np.float64
    assert np.max(np.abs(got - f[name + "_pred"])) <= 1e-12
    a, b = R.unpack(name, f[name + "_x"], D)
    ref = R.predict(f["held"], R.KIND[name], a, b, R.log_priors(f["y"], D))
    assert np.max(np.abs(ref - f[name + "_pred"])) <= 1e-12


@pytest.mark.parametrize("name", ["temp", "mlr", "vec"])
@pytest.mark.parametrize("fixture", R.FIXTURES)
def test_host_fits(fx, fixture, name):
    """`success` as the reference recorded it.  CG fits (MLR, vector): the
    restatement's reference-formula gradient at the fitted parameters meets
    SciPy CG's gtol.  Temperature: Newton-CG stops on its step (xtol = 1e-5),
    not on the gradient -- the reference's own successful s3 fit ends at
    |jac| = 4.9e-5 -- so its criterion is the distance |T - T_ref| <= 2e-5."""
    import calibrators as C
    f = fx[fixture]
    B, D = f["x"].shape
    cal = getattr(C, CLS[name])(f["x"].astype(np.float64), f["y"])
    assert bool(cal.optim.success) == bool(f[name + "_success"])
    _, jac, _, _ = R.forms(name, _ref_sums_fn(f), B, D)
    if name == "temp":
        assert abs(cal.T - float(f["temp_x"][0])) <= 2e-5
    else:
        assert np.max(np.abs(jac(cal.optim.x))) <= GTOL


def test_host_matrix_fit_and_soft_targets(fx):
    import calibrators as C
    from utils.ops import optim_temperature
    f = fx["s1"]
    B, D = f["x"].shape
    x64 = f["x"].astype(np.float64)
    cal = C.MatrixScalingCalibrator(x64, f["y"])
    fun, _, _, _ = R.forms("mat", _ref_sums_fn(f), B, D)
    assert np.isfinite(cal.W).all() and np.isfinite(cal.b).all() and cal.W.shape == (D, D)
    assert fun(cal.optim.x) < fun(np.zeros(D + D * D))
    # soft targets and both temperature methods run on the host
    soft = 0.9 * np.eye(D)[f["y"]] + 0.1 / D
    assert np.isfinite(C.MLRCalibrator(x64, soft).alpha)
    t_newton = optim_temperature(x64, f["y"])
    t_sgd = optim_temperature(x64, f["y"], method="sgd", min_diff=1e-4, step=0.5)
    assert abs(t_newton - float(f["temp_x"][0])) <= 2e-5 and abs(t_sgd - t_newton) <= 1e-2


def test_scaling_argument_validation_without_gpu():
    """The four entry points reject bad arguments before any launch."""
    lib = _lib.lib()
    P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    w = I64(-1)
    for kind, dim, want in ((0, 10, 12), (1, 10, 21), (2, 10, 111), (0, 256, 258), (1, 256, 513),
                            (2, 128, 1 + 128 + 128 * 128)):
        assert lib.cnf_scaling_sums_words(I32(kind), I32(dim), ctypes.byref(w)) == 0
        assert w.value == want
    assert lib.cnf_scaling_sums_words(I32(3), I32(10), ctypes.byref(w)) == -2
    assert lib.cnf_scaling_sums_words(I32(-1), I32(10), ctypes.byref(w)) == -2
    assert lib.cnf_scaling_sums_words(I32(0), I32(1), ctypes.byref(w)) == -2
    assert lib.cnf_scaling_sums_words(I32(0), I32(257), ctypes.byref(w)) == -3
    assert lib.cnf_scaling_sums_words(I32(2), I32(129), ctypes.byref(w)) == -3
    assert lib.cnf_scaling_sums_words(I32(0), I32(10), None) == -1

    n = ctypes.c_size_t(7)
    wb = lambda kind, dim, B: lib.cnf_scaling_workspace_bytes(I32(kind), I32(dim), I64(B),
                                                              ctypes.byref(n))
    assert wb(0, 10, 1) == 0 and n.value == 12 * 8            # one block
    assert wb(0, 10, 257) == 0 and n.value == 2 * 12 * 8      # 256 rows per block and pass
    assert wb(1, 100, 1 << 20) == 0 and n.value == 1024 * 201 * 8   # the grid cap
    assert wb(2, 100, 1 << 20) == 0 and n.value == 256 * 10101 * 8
    assert wb(2, 10, 0) == 0 and n.value == 0
    assert wb(3, 10, 8) == -2 and wb(0, 1, 8) == -2 and wb(2, 129, 8) == -3
    assert wb(0, 10, -1) == -4 and wb(0, 10, (1 << 26) + 1) == -4
    assert lib.cnf_scaling_workspace_bytes(I32(0), I32(10), I64(8), None) == -1

    x = (ctypes.c_float * 32)()
    y = (ctypes.c_int64 * 4)()
    prm = (ctypes.c_double * 128)()
    sums = (ctypes.c_double * 128)(*([7.0] * 128))
    ws = (ctypes.c_double * 256)()
    probs = (ctypes.c_float * 32)(*([7.0] * 32))
    px, py, pa, ps, pw, pp = (ctypes.addressof(v) for v in (x, y, prm, sums, ws, probs))

    def lg(x=px, lab=py, kind=0, dim=10, a=pa, b=pa + 8, grad=1, B=2, s=ps, w=pw, wbytes=2048):
        return lib.cnf_scaling_loss_grad(P(x), P(lab), I32(kind), I32(dim), P(a), P(b), I32(grad),
                                         I64(B), P(s), P(w), ctypes.c_size_t(wbytes), P(0))
    assert lg(kind=3) == -2 and lg(dim=1) == -2 and lg(dim=257) == -3
    assert lg(kind=2, dim=129) == -3
    assert lg(B=-1) == -4 and lg(B=(1 << 26) + 1) == -4
    assert lg(x=0) == -1 and lg(lab=0) == -1 and lg(a=0) == -1 and lg(s=0) == -1
    assert lg(w=0) == -1 and lg(wbytes=8) == -1          # no or too small a workspace
    assert lg(kind=1, b=0) == -1 and lg(kind=2, dim=3, b=0) == -1   # only the scalar kind has no bias
    assert lg(x=px + 2) == -6 and lg(lab=py + 4) == -6 and lg(a=pa + 4) == -6
    assert lg(b=pa + 12) == -6 and lg(s=ps + 4) == -6 and lg(w=pw + 4) == -6
    # B == 0 passes validation with no data pointers; the zero fill of `sums` is a
    # memset on the stream, which needs a device (-5 with hipErrorNoDevice here)
    st = lg(x=0, lab=0, w=0, wbytes=0, B=0)
    assert st == 0 or (st == -5 and lib.cnf_last_hip_error() == 100)

    def pr(x=px, kind=0, dim=10, a=pa, b=pa + 8, lp=pa + 256, out=pp, B=2):
        return lib.cnf_scaling_predict(P(x), I32(kind), I32(dim), P(a), P(b), P(lp), P(out),
                                       I64(B), P(0))
    assert pr(kind=3) == -2 and pr(dim=1) == -2 and pr(dim=257) == -3 and pr(kind=2, dim=129) == -3
    assert pr(B=-1) == -4 and pr(B=(1 << 26) + 1) == -4
    assert pr(x=0) == -1 and pr(a=0) == -1 and pr(lp=0) == -1 and pr(out=0) == -1
    assert pr(kind=1, b=0) == -1
    assert pr(x=px + 2) == -6 and pr(out=pp + 2) == -6 and pr(a=pa + 4) == -6
    assert pr(lp=pa + 260) == -6 and pr(b=pa + 12) == -6
    assert pr(x=0, out=0, B=0) == 0       # B == 0 is a no-op
    assert all(v == 7.0 for v in probs)


def test_torch_operators_register():
    import torch
    assert _lib.torch_ops() is not None, "libcnf_torch.so was not built"
    sch = str(torch.ops.cnf.scaling_loss_grad.default._schema)
    assert "Tensor(a!) sums" in sch and "Tensor? b" in sch and "bool want_grad" in sch
    assert "-> Tensor" in str(torch.ops.cnf.scaling_predict.default._schema)
