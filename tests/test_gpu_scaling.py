"""cnf_scaling_loss_grad / cnf_scaling_predict on the device (include/cnf.h;
cnf_hip/scaling.py; calibrators.py): evaluation parity through ctypes and
through the torch operators against the float64 restatement
(tests/_scaling_ref.py), the grid-stride path, the reference's recorded probe
values, saturation, bad labels, repeatability and graph replay, the device
fits of the four classes and the fused predict."""
import numpy as np
import pytest
import torch

import _scaling_ref as R
from cnf_hip import _lib, engine, scaling

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GTOL = 1e-5 + 1e-10
CLS = {"temp": "TempScalingCalibrator", "mlr": "MLRCalibrator",
       "vec": "VectorScalingCalibrator", "mat": "MatrixScalingCalibrator"}


@pytest.fixture(params=["ctypes", "torch_op"])
def path(request):
    old = engine.USE_TORCH_OPS
    engine.USE_TORCH_OPS = request.param == "torch_op"
    yield request.param
    engine.USE_TORCH_OPS = old


@pytest.fixture(scope="module")
def fx():
    return {n: R.load(n) for n in R.FIXTURES}


def _dev_sums(x, y, kind, a, b, want_grad=True, prefill=None):
    """One native call; returns every word of the sums buffer."""
    B, D = x.shape
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    ad = torch.from_numpy(np.asarray(a, dtype=np.float64).reshape(-1).copy()).to(DEV)
    bd = None if b is None else torch.from_numpy(np.asarray(b, dtype=np.float64).copy()).to(DEV)
    out = torch.full((scaling.sums_words(kind, D),), 0.0 if prefill is None else prefill,
                     dtype=torch.float64, device=DEV)
    ws = torch.empty(max(scaling.workspace_bytes(kind, D, B) // 8, 1), dtype=torch.float64,
                     device=DEV)
    scaling.loss_grad(xd, yd, kind, ad, bd, want_grad, out, ws)
    return out.cpu().numpy()


DIMS = {R.SCALAR: [2, 3, 10, 16, 17, 33, 100, 256], R.DIAG: [2, 3, 10, 16, 17, 33, 100, 256],
        R.FULL: [2, 3, 10, 16, 17, 33, 100, 128]}
CASES = [(k, D, bias) for k in (R.SCALAR, R.DIAG, R.FULL) for D in DIMS[k]
         for bias in ((True, False) if k == R.SCALAR else (True,))]


@pytest.mark.parametrize("kind,D,bias", CASES)
def test_evaluation_parity(path, kind, D, bias):
    """Every kind and width on both sides of each lanes-per-row and tile
    threshold, B around one wave / one block pass and a ragged 4,099, with and
    without want_grad: every word within EVAL_TOL * sum|terms|."""
    for B in (1, 63, 64, 65, 257, 4099):
        x, y, a, b = R.random_case(kind, D, B, 1000 * kind + 10 * D + B, bias)
        want, scale = R.sums(x, y, kind, a, b)
        got = _dev_sums(x, y, kind, a, b, True)
        R.assert_close(got, want, scale, B, (kind, D, B, "grad"))
        only = _dev_sums(x, y, kind, a, b, False, prefill=-3.0)
        R.assert_close(only[:1], want[:1], scale[:1], B, (kind, D, B, "loss"))
        assert (only[1:] == -3.0).all()
        assert only[0] == got[0] or abs(only[0] - got[0]) <= R.EVAL_TOL * scale[0]


def test_grid_stride_and_untouched_gradient_words():
    """D=3: 256 rows per block and pass, at most 1,024 blocks (the kernel's
    cap, read back from the workspace size): B = 2 * cap * 256 + 77 gives
    every block two full passes and some a ragged third."""
    D, kind = 3, R.SCALAR
    words = scaling.sums_words(kind, D)
    cap = scaling.workspace_bytes(kind, D, 1 << 26) // (8 * words)
    one = scaling.workspace_bytes(kind, D, 256) // (8 * words)
    two = scaling.workspace_bytes(kind, D, 257) // (8 * words)
    assert (one, two) == (1, 2)  # 256 rows per block and pass
    B = 2 * cap * 256 + 77
    x, y, a, b = R.random_case(kind, D, B, 7)
    want, scale = R.sums(x, y, kind, a, b)
    got = _dev_sums(x, y, kind, a, b, True)
    R.assert_close(got, want, scale, B, "grid-stride")
    only = _dev_sums(x, y, kind, a, b, False, prefill=5.5)
    R.assert_close(only[:1], want[:1], scale[:1], B, "grid-stride loss")
    assert (only[1:] == 5.5).all()


def _dev_sums_fn(f):
    xd, yd = torch.from_numpy(f["x"]).to(DEV), torch.from_numpy(f["y"]).to(DEV)
    objs = {}

    def fn(kind, a, b):
        if kind not in objs:
            objs[kind] = scaling.ScalingObjective(xd, yd, kind)
        return objs[kind].sums(a, b, True).copy(), R.sums(f["x"], f["y"], kind, a, b)[1]
    return fn


@pytest.mark.parametrize("name", R.CLASSES)
@pytest.mark.parametrize("fixture", R.FIXTURES)
def test_fixture_probes(fx, fixture, name):
    """Device `fun` and `jac`, formed as the classes form them, against the
    reference's recorded values."""
    f = fx[fixture]
    B, D = f["x"].shape
    fun, jac, fun_s, jac_s = R.forms(name, _dev_sums_fn(f), B, D)
    for i, x in enumerate(f[name + "_probe_x"]):
        R.assert_close(fun(x), f[name + "_probe_fun"][i], fun_s(x), B, (fixture, name, i, "fun"))
        R.assert_close(jac(x), f[name + "_probe_jac"][i], jac_s(x), B, (fixture, name, i, "jac"))


@pytest.mark.parametrize("kind", [R.SCALAR, R.DIAG, R.FULL])
def test_saturation(kind):
    """Logits x 50: finite everywhere, the restatement's loss, and a batch of
    rows whose p[y] underflowed sums to exactly B * -log(1e-7)."""
    D, B = 10, 64
    x, y, a, b = R.random_case(kind, D, B, 77)
    x = (x * np.float32(50)).astype(np.float32)
    want, scale = R.sums(x, y, kind, a, b)
    got = _dev_sums(x, y, kind, a, b, True)
    assert np.isfinite(got).all()
    R.assert_close(got, want, scale, B, "saturated")
    x[:] = 0
    x[:, 0] = 1000.0
    y[:] = 1 + (np.arange(B) % (D - 1))
    a1 = np.array([1.0]) if kind == R.SCALAR else np.ones(D) if kind == R.DIAG else np.eye(D).ravel()
    got = _dev_sums(x, y, kind, a1, np.zeros(D), True)
    assert np.isfinite(got).all()
    assert got[0] == B * -np.log(1e-7)   # 64 equal terms: every partial sum is exact


@pytest.mark.parametrize("kind,D", [(R.SCALAR, 10), (R.DIAG, 100), (R.FULL, 10), (R.FULL, 100)])
def test_bad_label_poisons_every_word(kind, D):
    x, y, a, b = R.random_case(kind, D, 300, 5)
    for bad in (-1, D):
        y2 = y.copy()
        y2[137] = bad
        got = _dev_sums(x, y2, kind, a, b, True)
        assert np.isnan(got).all()
        assert np.isnan(_dev_sums(x, y2, kind, a, b, False)[0])


@pytest.mark.parametrize("kind,D", [(R.SCALAR, 10), (R.DIAG, 100), (R.FULL, 33)])
def test_repeatable_and_graph_replay(kind, D):
    B = 4099
    x, y, a, b = R.random_case(kind, D, B, 11)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    ad, bd = torch.from_numpy(a.reshape(-1).copy()).to(DEV), torch.from_numpy(b.copy()).to(DEV)
    n = scaling.sums_words(kind, D)
    ws = torch.empty(scaling.workspace_bytes(kind, D, B) // 8, dtype=torch.float64, device=DEV)
    one = torch.zeros(n, dtype=torch.float64, device=DEV)
    two = torch.zeros(n, dtype=torch.float64, device=DEV)
    scaling.loss_grad(xd, yd, kind, ad, bd, True, one, ws)
    scaling.loss_grad(xd, yd, kind, ad, bd, True, two, ws)
    assert torch.equal(one.view(torch.int64), two.view(torch.int64))
    s = torch.cuda.Stream(device=DEV)
    rep = torch.zeros(n, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        scaling.loss_grad(xd, yd, kind, ad, bd, True, rep, ws)  # warm-up on the side stream
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            scaling.loss_grad(xd, yd, kind, ad, bd, True, rep, ws)
        rep.zero_()
        g.replay()
        s.synchronize()
    assert torch.equal(one.view(torch.int64), rep.view(torch.int64))


def test_empty_batch_zeroes_the_words():
    xd = torch.zeros(0, 10, device=DEV)
    yd = torch.zeros(0, dtype=torch.int64, device=DEV)
    ad = torch.ones(1, dtype=torch.float64, device=DEV)
    out = torch.full((12,), 9.0, dtype=torch.float64, device=DEV)
    scaling.loss_grad(xd, yd, R.SCALAR, ad, None, True, out, torch.empty(1, dtype=torch.float64,
                                                                          device=DEV))
    assert (out.cpu().numpy() == 0).all()


def _fit(name, f):
    import calibrators as C
    n0 = engine.stats["scaling"]
    cal = getattr(C, CLS[name])(torch.from_numpy(f["x"]).to(DEV), torch.from_numpy(f["y"]).to(DEV))
    assert engine.stats["scaling"] > n0, "the fit did not run on the device"
    return cal


FITS = [(fixture, name) for fixture in ("s1", "s2") for name in ("temp", "mlr", "vec")] + \
    [("s3", "temp")]


@pytest.mark.parametrize("fixture,name", FITS)
def test_device_fits(fx, fixture, name):
    """`success` as recorded.  CG fits: the restatement's reference-formula
    gradient at the device-fitted parameters meets SciPy CG's gtol.
    Temperature (Newton-CG stops on its step, xtol = 1e-5): |T - T_ref| <= 2e-5.
    Parameter and objective distances from the reference are recorded
    (conftest RECORDS -> scaling_fit_errors.jsonl) and carry no bar."""
    import conftest
    f = fx[fixture]
    B, D = f["x"].shape
    cal = _fit(name, f)
    assert bool(cal.optim.success) == bool(f[name + "_success"])
    ref_fn = lambda kind, a, b: R.sums(f["x"], f["y"], kind, a, b)
    fun, jac, _, _ = R.forms(name, ref_fn, B, D)
    x = np.asarray(cal.optim.x, dtype=np.float64).reshape(-1)
    if name == "temp":
        assert abs(cal.T - float(f["temp_x"][0])) <= 2e-5
    else:
        assert np.max(np.abs(jac(x))) <= GTOL
    row = {"fixture": fixture, "class": name, "nit": int(cal.optim.nit),
           "nit_ref": int(f[name + "_nit"]),
           "param_dist": float(np.max(np.abs(x - f[name + "_x"]))),
           "fun_dist": float(abs(fun(x) - float(f[name + "_fun"])))}
    conftest.RECORDS.setdefault("scaling_fit_errors", []).append(row)
    print("scaling_fit_errors", row)


@pytest.mark.parametrize("fixture", ["s1", "s2"])
def test_device_matrix_fit(fx, fixture):
    f = fx[fixture]
    B, D = f["x"].shape
    cal = _fit("mat", f)
    assert np.isfinite(cal.W).all() and np.isfinite(cal.b).all()
    fun, _, _, _ = R.forms("mat", lambda kind, a, b: R.sums(f["x"], f["y"], kind, a, b), B, D)
    assert fun(cal.optim.x) < fun(np.zeros(D + D * D))


@pytest.mark.parametrize("kind", [R.SCALAR, R.DIAG, R.FULL])
@pytest.mark.parametrize("fixture", R.FIXTURES)
def test_predict_against_restatement(fx, path, fixture, kind):
    """|delta| <= 2^-23 * p + 1e-12: the value is computed in float64 and
    rounded once to fp32; the bar allows twice that rounding."""
    f = fx[fixture]
    D = f["x"].shape[1]
    _, _, a, b = R.random_case(kind, D, 4, 31 + kind)
    lp = R.log_priors(f["y"], D)
    want = R.predict(f["held"], kind, a, b, lp)
    n0 = engine.stats["scaling_predict"]
    got = scaling.predict(torch.from_numpy(f["held"]).to(DEV), kind, a, b, lp)
    assert engine.stats["scaling_predict"] == n0 + 1
    assert got.is_cuda and got.dtype == torch.float32
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    assert (err <= 2.0 ** -23 * want + 1e-12).all(), float(np.max(err / (want + 1e-30)))


def test_fit_predict_score_end_to_end(fx):
    """A class fitted on the device, predict of a ROCm tensor, then
    calibration_record: the NLL of the record equals the NLL of the same
    probabilities scored on the host."""
    from cnf_hip.metrics import CalibrationSums, calibration_record
    f = fx["s2"]
    cal = _fit("vec", f)
    held = torch.from_numpy(f["held"]).to(DEV)
    probs = cal.predict(held)
    assert probs.is_cuda and probs.dtype == torch.float32
    yh = torch.from_numpy(f["y_held"]).to(DEV)
    dev_nll = CalibrationSums(calibration_record(probs, yh, 15), 15).nll()
    p64 = probs.cpu().numpy().astype(np.float64)
    host_nll = float(np.mean(-np.log(p64[np.arange(p64.shape[0]), f["y_held"]] + 1e-7)))
    assert abs(dev_nll - host_nll) <= 1e-9   # 2^-33 per row of fixed point, as cnf_metrics' tests
    host = cal.predict(f["held"].astype(np.float64))
    assert isinstance(host, np.ndarray) and host.dtype == np.float64
    assert np.max(np.abs(host - p64)) <= 1e-6
