"""The fused score launch on the GPU (cnf_planar_score; include/cnf.h,
csrc/cnf_score.h) and Calibrator.score on every calibrator.

The primary bar is exact: score(x, y, bins) must leave the 4 + 3 * bins words
that calibration_record(predict(x), y, bins) leaves -- the two-launch path the
existing tests pin to the reference -- on the fixtures, on each side of every
block / lane / tile edge, through splits, accumulation, graph replay and
views.  One test is anchored on the reference alone (its recorded float64
probabilities scored on the host) with bounds derived from the predict bars.
"""
import json
import os

import numpy as np
import pytest
import torch

import _metrics_ref as MR
import _pav_ref as PV
import _planar_predict_ref as PR
import _planar_ref as R
import _scaling_ref as SR
import calibrators as C
from _golden import GOLDEN
from cnf_hip import engine
from cnf_hip import pav, scaling  # noqa: F401  (their engine.stats counters exist from here on)
from cnf_hip.metrics import CalibrationSums, calibration_record
from conftest import RECORDS
from flows import flows as FL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BINS = (1, 15, 64)
_cache = {}


class Case:
    """One (family, model, x): score and predict as closures over device
    parameters, so both run with no host copy (graph-capturable)."""

    def __init__(self, name, score, predict, x, bar=None, ref=None):
        self.name, self.score, self.predict, self.bar, self.ref = name, score, predict, bar, ref
        self.x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
        self.B, self.D = self.x.shape

    def labels(self, seed=3):
        y = np.random.RandomState(seed).randint(0, self.D, size=self.B).astype(np.int64)
        return torch.from_numpy(y).to(DEV)


def two_launch(case, x, y, bins, record=None):
    return calibration_record(case.predict(x), y, bins, record)


def assert_same(case, x, y, bins=BINS):
    for b in bins:
        got, want = case.score(x, y, b), two_launch(case, x, y, b)
        assert got.dtype == torch.int64 and got.shape == (4 + 3 * b,)
        assert torch.equal(got, want), (case.name, b, got.tolist(), want.tolist())
        assert int(got[0] + got[1]) == x.shape[0]


# ---- the families ------------------------------------------------------------------
def planar_case(name, stack, x, lp, **kw):
    lp = torch.as_tensor(lp, dtype=torch.float32, device=DEV)
    return Case(name, lambda x, y, bins=15, record=None: stack.score(x, lp, y, bins, record),
                lambda x: stack.predict(x, lp), x, **kw)


def planar_fixture(name):
    d = PR.load(name)
    flow = R.build_flow(d, DEV)
    _cache[("flow", name)] = flow
    return planar_case("planar/" + name, flow._planar_stack(), d["x"], d["log_priors"],
                       bar=lambda p, f=R.bar(d["floor_probs"]): f * (p + 1.0), ref=d["probs64"])


def planar_random(D, L, B, seed):
    rs = np.random.RandomState(seed)
    d = {"W": (rs.standard_normal((L, D)) * 0.5).astype(np.float32),
         "U": (rs.standard_normal((L, D)) * 0.5).astype(np.float32),
         "Bv": (rs.standard_normal(L) * 0.5).astype(np.float32)}
    flow = R.build_flow(d, DEV)
    _cache[("flow", D, L, seed)] = flow
    x = rs.standard_normal((B, D)).astype(np.float32)
    lp = np.log(np.arange(1, D + 1) / (D * (D + 1) / 2.0))
    return planar_case("planar/D%d" % D, flow._planar_stack(), x, lp)


def random_case(D, B, seed=7):
    return planar_random(D, 3, B, seed)


# ---- 1. word-for-word equality on the fixtures ---------------------------------------
@pytest.mark.parametrize("name", ["one", "d3", "d10", "d17", "d100"])
def test_planar_fixtures(name):
    c = planar_fixture(name)
    n0, p0, m0 = (engine.stats[k] for k in ("planar_score", "planar_predict", "metrics"))
    rec = c.score(c.x, c.labels(), 15)
    assert (engine.stats["planar_score"], engine.stats["planar_predict"],
            engine.stats["metrics"]) == (n0 + 1, p0, m0)
    assert int(rec[0]) == c.B and int(rec[1]) == 0
    assert_same(c, c.x, c.labels())


@pytest.mark.parametrize("name", ["nan", "inf"])
def test_planar_non_finite_rows_are_invalid_only(name):
    c = planar_fixture(name)
    for b in BINS:
        rec = c.score(c.x, c.labels(), b)
        want = torch.zeros(4 + 3 * b, dtype=torch.int64)
        want[1] = c.B
        assert torch.equal(rec.cpu(), want)
        assert torch.equal(rec, two_launch(c, c.x, c.labels(), b))


def _fixture_cases():
    return [planar_fixture("d3"), planar_fixture("d10"), planar_fixture("d17"),
            planar_fixture("d100")]


@pytest.mark.parametrize("i", range(4))
def test_non_finite_inputs_and_bad_labels_are_invalid_only(i):
    """Rows holding NaN / +inf logits (the flow turns them into NaN rows)
    and labels -1 and D land in n_invalid and nowhere else: the record is that
    of the remaining rows plus n_invalid."""
    c = _fixture_cases()[i]
    x, y = c.x.clone(), c.labels()
    x[1, 0], x[5, c.D - 1] = float("nan"), float("inf")
    y[2], y[7], y[c.B - 1] = -1, c.D, c.D + 100
    keep = torch.ones(c.B, dtype=torch.bool, device=DEV)
    keep[[1, 5, 2, 7, c.B - 1]] = False
    for b in BINS:
        rec = c.score(x, y, b)
        assert torch.equal(rec, two_launch(c, x, y, b)), c.name
        only = c.score(x[keep], y[keep], b)
        assert int(only[1]) == 0
        only[1] += 5
        assert torch.equal(rec, only), c.name


# ---- 2. block and lane edges -----------------------------------------------------------
EDGES = [(3, 255), (3, 256), (3, 257), (10, 255), (10, 256), (10, 257), (17, 15), (17, 16),
         (17, 17), (100, 3), (100, 4), (100, 5), (10, 1), (17, 1), (100, 1)]


@pytest.mark.parametrize("D,B", EDGES)
def test_block_edges(D, B):
    """Each side of a block's row count: 256 rows (one lane per row), 16 rows
    (16 lanes per row), 4 rows (64 lanes per row); one row."""
    c = random_case(D, B)
    assert_same(c, c.x, c.labels())


@pytest.mark.parametrize("D", [2, 4, 5, 16, 17, 64, 65, 256])
def test_lane_switches(D):
    """Each side of every lanes-per-row / columns-per-lane switch, more than
    one block, a ragged last block."""
    rpb = 256 if D <= 16 else 16 if D <= 64 else 4
    c = random_case(D, 2 * rpb + 3)
    assert_same(c, c.x, c.labels())


def test_one_row_past_the_grid_cap():
    """1024 blocks x 256 rows + 1: block 0 takes a second pass of one row."""
    c = random_case(3, 1024 * 256 + 1)
    assert_same(c, c.x, c.labels(), bins=(15,))


# ---- 3. a crafted tie on a bin edge --------------------------------------------------------
TIES = [(2, 0, 1), (17, 2, 16), (100, 10, 64)]


def _tied_stack(D, i, j, B):
    """A 3-layer stack and logits whose columns i < j stay bitwise equal and
    the row maximum through the whole predict: w is 0 in both columns and
    u[i] == u[j], so u_hat[i] == u_hat[j] == u[i] and both get the same
    increment in every layer; x[:, i] == x[:, j] lies 12 above the other
    columns' N(0, 1); the priors are uniform.  D = 2 has no third column to
    carry w: there w = (c, -c) and b = 0, so the centred row (0, 0) gives
    tanh(0) = 0 in every layer and both columns stay 0."""
    rs = np.random.RandomState(100 + D)
    W = (0.3 * rs.standard_normal((3, D))).astype(np.float32)
    U = (0.3 * rs.standard_normal((3, D))).astype(np.float32)
    Bv = (0.3 * rs.standard_normal(3)).astype(np.float32)
    x = rs.standard_normal((B, D)).astype(np.float32)
    if D == 2:
        W[:, 1] = -W[:, 0]
        Bv[:] = 0.0
        x[:, j] = x[:, i]
    else:
        W[:, i] = W[:, j] = 0.0
        x[:, i] = x[:, j] = (12.0 + rs.uniform(0.0, 1.0, size=B)).astype(np.float32)
    U[:, j] = U[:, i]
    flow = R.build_flow({"W": W, "U": U, "Bv": Bv}, DEV)
    _cache[("tie", D)] = flow
    return planar_case("planar/tie%d" % D, flow._planar_stack(), x, np.full(D, -np.log(D)))


@pytest.mark.parametrize("D,i,j", TIES)
def test_tie_in_the_fused_kernel(D, i, j):
    """Two bitwise equal row maxima in columns i < j through cnf_planar_score
    (D = 17: 16 lanes per row, D = 100: 64; j sits in lane 0, below i's lane):
    the prediction is i, the smaller index, whichever lane holds it.  Checked
    from the record alone -- n_correct counts the rows labelled i and none
    labelled j, conf_fx is the sum of rint(conf * 2^32) of the tied value --
    and against the two-launch record.  At D = 2 every confidence is exactly
    0.5, the upper edge of bin 0 of 2: conf_fx = B * 2^31."""
    B = 301
    c = _tied_stack(D, i, j, B)
    y = torch.from_numpy(np.where(np.arange(B) % 3 == 0, j, i).astype(np.int64)).to(DEV)
    n_i = int((y == i).sum())
    probs = c.predict(c.x).cpu().numpy()
    conf = probs[:, i]
    assert np.array_equal(conf, probs[:, j]) and np.array_equal(conf, probs.max(axis=1))
    fx = np.rint(conf.astype(np.float64) * 2.0 ** 32).astype(np.int64)
    for bins in (2, 15):
        n0 = {k: engine.stats[k] for k in ("planar_score", "planar_predict", "metrics")}
        rec = c.score(c.x, y, bins)
        assert {k: engine.stats[k] - n0[k] for k in n0} == {"planar_score": 1, "planar_predict": 0,
                                                            "metrics": 0}
        assert torch.equal(rec, two_launch(c, c.x, y, bins))
        rec = rec.cpu().numpy()
        assert rec[0] == B and rec[1] == 0 and rec[3] == n_i          # the first maximum wins
        edges = np.arange(bins + 1) * (1.0 / bins)          # i * width < conf <= (i + 1) * width
        b = (edges[None, :] < conf.astype(np.float64)[:, None]).sum(axis=1) - 1
        assert np.array_equal(rec[4:4 + bins], np.bincount(b, minlength=bins))
        assert np.array_equal(rec[4 + bins:4 + 2 * bins],
                              np.bincount(b, weights=fx.astype(np.float64), minlength=bins)
                              .astype(np.int64))
        assert np.array_equal(rec[4 + 2 * bins:], np.bincount(b[(y == i).cpu().numpy()],
                                                              minlength=bins))
    if D == 2:
        assert (conf == 0.5).all()
        rec = c.score(c.x, y, 2).cpu().numpy()
        assert rec[4] == B and rec[5] == 0 and rec[6] == B * 2 ** 31 and rec[8] == n_i


@pytest.mark.parametrize("D,i,j", TIES)
def test_tie_on_a_bin_edge(D, i, j):
    """Two equal maxima in columns i < j (for D = 17 and 100 held by different
    lanes, j's lane below i's): the prediction is i.  At D = 2 every
    confidence is exactly 0.5 = the upper edge of bin 0 of 2."""
    cal = C.DummyCalibrator(np.zeros((D, D)), np.arange(D))      # uniform priors
    B = 301
    x = torch.zeros(B, D, device=DEV)
    if D > 2:
        x[:, i] = x[:, j] = 3.0
    y = torch.from_numpy(np.where(np.arange(B) % 3 == 0, j, i).astype(np.int64)).to(DEV)
    n_i = int((y == i).sum())
    sums, n = _delta(lambda: cal.score_sums(x, y, bins=2))
    assert n == {"scaling_predict": 1, "metrics": 1}          # Dummy: predict on the device
    rec = sums.record
    probs = cal.predict(x)
    assert torch.equal(torch.from_numpy(rec).to(DEV), calibration_record(probs, y, 2))
    assert rec[0] == B and rec[1] == 0 and rec[3] == n_i          # the first maximum wins
    conf = float(probs[0, i])
    assert float(probs[0, j]) == conf and bool((probs[:, i] == conf).all())
    b = 0 if conf <= 0.5 else 1
    assert rec[4 + b] == B and rec[4 + 1 - b] == 0
    assert rec[6 + b] == B * int(np.rint(conf * 2.0 ** 32)) and rec[8 + b] == n_i
    term = -np.log(np.float64(conf) + 1e-7) * 2.0 ** 32
    assert abs(int(rec[2]) - B * term) <= B                      # log rounding: <= 1 unit per row
    if D == 2:
        assert conf == 0.5 and b == 0 and rec[6] == B * 2 ** 31


# ---- 4. accumulation and splits --------------------------------------------------------------
@pytest.mark.parametrize("i", range(4))
def test_splits_accumulation_repeat_and_views(i):
    c = _fixture_cases()[i]
    x, y = c.x, c.labels()
    whole = c.score(x, y, 15)
    assert torch.equal(whole, c.score(x, y, 15))                 # two calls, bitwise
    for k in (1, 3, c.B // 2 + 1):                               # k inside a block
        assert torch.equal(c.score(x[:k], y[:k], 15) + c.score(x[k:], y[k:], 15), whole), k
    rec = torch.zeros_like(whole)
    assert c.score(x, y, 15, rec) is rec
    c.score(x, y, 15, rec)
    assert torch.equal(rec, 2 * whole)                           # added to, not overwritten
    rec.zero_()
    c.score(x[:k], y[:k], 15, rec)
    c.score(x[k:], y[k:], 15, rec)
    assert torch.equal(rec, whole)
    # views: x[1:] starts D floats into the buffer; a column slice is not contiguous
    assert torch.equal(c.score(x[1:], y[1:], 15), two_launch(c, x[1:], y[1:], 15))
    wide = torch.zeros(c.B, c.D + 3, device=DEV)
    wide[:, 1:c.D + 1] = x
    view = wide[:, 1:c.D + 1]
    assert not view.is_contiguous()
    assert torch.equal(c.score(view, y, 15), whole)
    assert torch.equal(c.score(x, torch.stack([y, y], 1)[:, 0], 15), whole)   # strided labels


@pytest.mark.parametrize("i", range(4))
def test_graph_replay_adds(i):
    """A call captured with torch.cuda.graph and replayed three times adds
    three times the eager record."""
    c = _fixture_cases()[i]
    x, y = c.x, c.labels()
    whole = c.score(x, y, 15)
    rec = torch.zeros_like(whole)
    s = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c.score(x, y, 15, rec)            # the side stream's buffers exist before capture
        s.synchronize()
        assert torch.equal(rec, whole)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            c.score(x, y, 15, rec)
        rec.zero_()
        for _ in range(3):
            g.replay()
        s.synchronize()
    assert torch.equal(rec, 3 * whole)


def test_record_rules():
    c = planar_fixture("d10")
    y = c.labels()
    for bad in (torch.zeros(49, dtype=torch.int32, device=DEV),
                torch.zeros(48, dtype=torch.int64, device=DEV),
                torch.zeros(49, dtype=torch.int64),
                torch.zeros(98, dtype=torch.int64, device=DEV)[::2]):
        n = dict(engine.stats)
        with pytest.raises(ValueError):
            c.score(c.x, y, 15, bad)
        assert dict(engine.stats) == n
    with pytest.raises(ValueError):
        c.score(c.x, y[:-1], 15)
    with pytest.raises(ValueError):
        c.score(c.x, y, 65)


# ---- 5. anchored on the reference ------------------------------------------------------------
def _g7_cal(name):
    from flows.realNVP_torch import RealNvpFlow
    f = np.load(os.path.join(GOLDEN, name + ".npz"))
    torch.manual_seed(0)
    cal = C.TorchFlowCalibrator(RealNvpFlow, f["x"].astype(np.float64), f["y"], layers=5,
                                hidden_size=[3, 3], epochs=0, dev=torch.device(DEV))
    cal.flow.load_state_dict({k[2:]: torch.from_numpy(f[k]) for k in f.files
                              if k.startswith("p:")})
    return cal, f


SCALING_CLS = {"temp": "TempScalingCalibrator", "mlr": "MLRCalibrator",
               "vec": "VectorScalingCalibrator", "mat": "MatrixScalingCalibrator"}
# every recorded *_pred (s3 records no matrix fit)
SCALING_REF = [(fixture, cls) for fixture in SR.FIXTURES for cls in SR.CLASSES
               if (fixture, cls) != ("s3", "mat")]


def _reference_cases():
    for n in ("d3", "d10", "d17", "d100"):
        c = planar_fixture(n)
        yield c.name, c, c.x, c.labels().cpu().numpy()
    for fixture, cls in SCALING_REF:      # the scaling calibrators' score_sums: the composed path
        f = SR.load(fixture)
        D = f["x"].shape[1]
        cal = getattr(C, SCALING_CLS[cls]).__new__(getattr(C, SCALING_CLS[cls]))
        C.Calibrator.__init__(cal, f["x"].astype(np.float64), f["y"])
        v = f[cls + "_x"]                 # the reference's recorded fit, not one of ours
        if cls == "temp":
            cal.T = float(v[0])
        elif cls == "mlr":
            cal.alpha, cal.gamma = float(v[0]), v[1:].copy()
        else:
            cal.b, cal.W = v[:D].copy(), (v[D:] if cls == "vec" else v[D:].reshape(D, D)).copy()
        x = torch.from_numpy(f["held"]).to(DEV)
        c = Case("scaling/%s/%s" % (fixture, cls), lambda x, y, bins=15, record=None, cal=cal:
                 torch.from_numpy(cal.score_sums(x, y, bins, record).record).to(DEV), None, x,
                 bar=lambda p: 2.0 ** -23 * p + 1e-12, ref=f[cls + "_pred"])
        yield c.name, c, x, f["y_held"]
    for n in ("mod", "sat"):      # PAVCalibrator.score_sums: the composed path
        f = PV.load(n)
        with np.errstate(divide="ignore"):
            cal = C.PAVCalibrator(f["x"].astype(np.float64), f["y"])
        x = torch.from_numpy(f["held"]).to(DEV)
        y = np.random.RandomState(3).randint(0, x.shape[1], size=x.shape[0]).astype(np.int64)
        c = Case("pav/" + n, lambda x, y, bins=15, record=None, cal=cal:
                 torch.from_numpy(cal.score_sums(x, y, bins, record).record).to(DEV), None, x,
                 bar=lambda p: np.full_like(p, 2.0 ** -22), ref=f["pred"])
        yield c.name, c, x, y
    for n in ("g7_calibrator_d3", "g7b_calibrator_d3_mb128"):
        cal, f = _g7_cal(n)
        x = torch.from_numpy(f["x_test"]).to(DEV)
        y = np.random.RandomState(3).randint(0, 3, size=x.shape[0]).astype(np.int64)
        c = Case(n, lambda x, y, bins=15, record=None, cal=cal:
                 torch.from_numpy(cal.score_sums(x, y, bins, record).record).to(DEV), None, x,
                 bar=lambda p: np.full_like(p, 1e-5), ref=f["pred"])
        yield n.split("_")[0], c, x, y


REF_NAMES = ["planar/d3", "planar/d10", "planar/d17", "planar/d100"] + \
    ["scaling/%s/%s" % fc for fc in SCALING_REF] + ["pav/mod", "pav/sat", "g7", "g7b"]


@pytest.mark.parametrize("name", REF_NAMES)
def test_against_the_reference_record(name):
    """The fused record against tests/_metrics_ref.score of the reference's
    recorded float64 probabilities.  F: rows whose reference confidence lies
    within 1e-5 of a bin edge i / 15 (a device value within the predict bar may
    fall in the neighbouring bin: two count words each); G: rows whose top-two
    gap is <= 2e-5 (the prediction may flip).  NLL: d(-log(p + 1e-7)) =
    dp / (p + 1e-7), |dp| <= the family's predict bar, factor two for the
    second order."""
    if "ref" not in _cache:
        _cache["ref"] = {n: (c, x, y) for n, c, x, y in _reference_cases()}
    c, x, y = _cache["ref"][name]
    p = np.asarray(c.ref, dtype=np.float64)
    B = p.shape[0]
    ref = MR.score(p, y, 15)
    conf = np.max(p, axis=1)
    top2 = np.sort(p, axis=1)[:, -2:]
    F = int((np.abs(conf[:, None] - np.arange(16)[None, :] / 15.0) <= 1e-5).any(axis=1).sum())
    G = int((top2[:, 1] - top2[:, 0] <= 2e-5).sum())
    assert F + G <= 0.02 * B, (F, G)
    s = CalibrationSums(c.score(x, torch.from_numpy(y).to(DEV), 15), 15)
    nll_bar = 2.0 * float(np.mean(c.bar(p[np.arange(B), y]) / (p[np.arange(B), y] + 1e-7)))
    row = {"case": name, "rows": B, "F": F, "G": G,
           "d_correct": abs(s.n_correct - ref["n_correct"]),
           "d_bins_l1": int(np.abs(s.bin_count - ref["count"]).sum()),
           "d_nll": abs(s.nll() - ref["nll"]), "nll_bar": nll_bar,
           "d_ece": abs(s.ece() - ref["ece"])}
    RECORDS.setdefault("score_parity", []).append(row)
    print("score_parity", json.dumps(row))
    assert s.n == ref["n"] == B and s.n_invalid == 0
    assert row["d_correct"] <= G
    assert row["d_bins_l1"] <= 2 * F
    assert row["d_nll"] <= nll_bar


# ---- 6. the calibrators ------------------------------------------------------------------------
KEYS = ("planar_score", "planar_predict", "scaling_predict",
        "pav_predict", "predict", "metrics")


def _delta(fn):
    n0 = {k: engine.stats[k] for k in KEYS}
    out = fn()
    return out, {k: engine.stats[k] - n0[k] for k in KEYS if engine.stats[k] != n0[k]}


def _scaling_cals():
    if "cals" not in _cache:
        f = SR.load("s1")
        xd, yd = torch.from_numpy(f["x"]).to(DEV), torch.from_numpy(f["y"]).to(DEV)
        _cache["cals"] = (f, {n: getattr(C, n)(xd, yd) for n in (
            "TempScalingCalibrator", "MLRCalibrator", "VectorScalingCalibrator",
            "MatrixScalingCalibrator")})
    return _cache["cals"]


@pytest.mark.parametrize("name", ["DummyCalibrator", "TempScalingCalibrator", "MLRCalibrator",
                                  "VectorScalingCalibrator", "MatrixScalingCalibrator"])
def test_scaling_calibrators_score_on_the_device(name):
    """No fused kernel for this family: score of a ROCm tensor is the fused
    predict plus one cnf_metrics launch, under the same interface."""
    f, cals = _scaling_cals()
    cal = C.DummyCalibrator(f["x"].astype(np.float64), f["y"]) if name == "DummyCalibrator" \
        else cals[name]
    held, yh = torch.from_numpy(f["held"]).to(DEV), f["y_held"]
    got, d = _delta(lambda: cal.score(held, yh))
    assert d == {"scaling_predict": 1, "metrics": 1}
    assert got == cal.evaluate(held, yh) and got["n"] == 256
    assert cal.score(held, np.eye(3)[yh], bins=7) == cal.evaluate(held, yh, bins=7)
    rec = torch.zeros(49, dtype=torch.int64, device=DEV)
    cal.score_sums(held, torch.from_numpy(yh).to(DEV), 15, rec)
    sums = cal.score_sums(held, yh, 15, rec)
    probs, d = _delta(lambda: cal.predict(held))
    assert d == {"scaling_predict": 1} and probs.is_cuda and probs.dtype == torch.float32
    assert np.array_equal(sums.record, 2 * calibration_record(probs, torch.from_numpy(yh), 15)
                          .cpu().numpy())
    if name == "DummyCalibrator":   # softmax of the centred logits, then the prior correction
        want = C.Calibrator.predict(cal, f["held"].astype(np.float64))
        err = np.abs(probs.cpu().numpy().astype(np.float64) - want)
        assert (err <= 2.0 ** -23 * want + 1e-12).all()
        # host inputs stay on the host
        _, d = _delta(lambda: cal.score(f["held"].astype(np.float64), yh))
        assert d == {}


def test_pav_calibrator_scores_on_the_device():
    f = PV.load("mod")
    cal = C.PAVCalibrator(f["x"].astype(np.float64), f["y"])
    held = torch.from_numpy(f["held"]).to(DEV)
    yh = np.random.RandomState(5).randint(0, 4, size=held.shape[0])
    got, d = _delta(lambda: cal.score(held, yh))
    assert d == {"pav_predict": 1, "metrics": 1}     # no fused kernel for this family
    assert got == cal.evaluate(held, yh)


def test_planar_flow_calibrator_scores_in_one_launch(monkeypatch):
    from flows._factory import PlanarFlow
    d = PR.load_cal("mb128")
    torch.manual_seed(int(d["seed"]))
    cal = C.TorchFlowCalibrator(PlanarFlow, d["logits"], np.eye(3)[d["labels"]], layers=4,
                                epochs=int(d["epochs"]), batch_size=int(d["batch_size"]),
                                dev=torch.device(DEV))
    held = d["held"]
    y = np.random.RandomState(71).randint(0, 3, size=held.shape[0])
    cal.predict(held)                                   # the resident replica exists
    for logits in (held, torch.as_tensor(held, dtype=torch.float32).to(DEV)):
        got, n = _delta(lambda: cal.score(logits, y))
        assert n == {"planar_score": 1}
        assert got == cal.evaluate(held, y)
    rec = torch.zeros(49, dtype=torch.int64, device=DEV)
    cal.score_sums(held, y, record=rec)
    cal.score_sums(held, np.eye(3)[y], record=rec)
    assert np.array_equal(rec.cpu().numpy(), 2 * cal.evaluate_sums(held, y).record)
    # CNF_PLANAR_NATIVE=0: no native launch of any kind
    monkeypatch.setattr(FL, "PLANAR_NATIVE", False)
    got0, n = _delta(lambda: cal.score(held, y))
    assert n == {} and got0["n"] == held.shape[0]
    # ... and a caller's device record is still added to
    rec.zero_()
    held32 = np.asarray(held, dtype=np.float32)
    sums = cal.score_sums(torch.from_numpy(held32).to(DEV), y, record=rec)
    assert np.array_equal(sums.record, cal.score_sums(held32, y).record)     # the host path's
    assert np.array_equal(rec.cpu().numpy(), sums.record) and sums.n == held.shape[0]


def test_coupling_flow_calibrator_keeps_two_launches():
    cal, f = _g7_cal("g7_calibrator_d3")
    y = np.random.RandomState(3).randint(0, 3, size=200)
    cal.predict(f["x_test"])
    for logits in (f["x_test"], torch.from_numpy(f["x_test"]).to(DEV)):
        got, n = _delta(lambda: cal.score(logits, y))
        assert n == {"predict": 1, "metrics": 1}
        assert got == cal.evaluate(f["x_test"], y)


# ---- 7. one large call per family ---------------------------------------------------------------
def test_million_rows_once():
    """2^20 x 10, L = 10: the fused record equals the two-launch one."""
    B, D = 1 << 20, 10
    c = planar_random(D, 10, 4, 61)
    g = torch.Generator(device="cpu").manual_seed(62)
    x = (1.5 * torch.randn(B, D, generator=g)).to(DEV)
    y = torch.randint(0, D, (B,), generator=g).to(DEV)
    got = c.score(x, y, 15)
    assert torch.equal(got, two_launch(c, x, y, 15))
    assert int(got[0]) + int(got[1]) == B
