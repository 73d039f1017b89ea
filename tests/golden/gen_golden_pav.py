"""Generate the isotonic-calibrator fixtures (tests/golden/pav/*.npz) FROM THE
REFERENCE ITSELF: its PAVCalibrator (calibrators.py:208-236) over the installed
sklearn's IsotonicRegression, fitted on seeded logits.

Test infrastructure only; runs in the build container on the CPU, where the
reference is mounted read-only at /root/reference.  Nothing here is imported
by the product or by the tests: those read only the committed .npz files.
The reference still says `np.float`, which NumPy 2 dropped: this generator
sets `np.float = float` before it imports the reference.

Inputs.  Training logits are fp32 values whose rows sum to exactly zero, built
as tests/golden/gen_golden_scaling.py builds them (z rounded to multiples of
2^-10, x_j = (D k_j - sum_i k_i) 2^-10 / P, P the power of two nearest D), so
the reference's float64 centring leaves them unchanged: a fit from the fp32
values (a tensor input) and the reference's fit see identical numbers.
z = scale * 2 * N(0, 1); the label of a row is drawn from softmax(z / (2 * scale)), an over-confident model.  Held-out rows are plain
fp32 draws of the same law (predict centres them itself).

  ties   D=3, B=1000  rows 700..999 are copies of rows 0..299 (labels drawn
                      anew): exact ties that both sides see identically
  mod    D=4, B=512
  sat    D=4, B=512   logits x 40: scores saturate below 1e-15 and within
                      1e-15 of 1, which exercises _make_unique's grouping
  degen  D=3, B=64    class 2 never occurs (one-hot targets with an empty
                      column): its model is the constant 0, its log prior -inf
  one    D=3, B=1     (one-hot target)

Recorded per fixture: x, y, held, each class's X_thresholds_ / y_thresholds_
(concatenated in thr_x / thr_y, counts in n_thr), pred = predict(held) as
float64 (NaN where the reference returns NaN), log_priors and the seed.

For `ties` and `mod` the generator asserts, on the reference's own float64
scores, that per class the smallest gap between DISTINCT training scores is
>= 1e-8 (recorded as min_gap), taking the first seed of seed0, seed0 + 10, ...
on which it holds: a device score differs from NumPy's by a few float64 ulps
(<= ~1e-15), which moves a value interpolated across a ramp of width g by at
most 1e-15 / g <= 1e-7, the order of the fp32 output rounding.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_pav.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "pav")
MIN_GAP = 1e-8


def _reference():
    sys.dont_write_bytecode = True
    np.float = float  # the alias NumPy 2 removed; the reference's fit uses it
    sys.path.insert(0, REF)
    import calibrators as C  # the reference's
    return C


def make_inputs(D, B, held, seed, scale=1.0, copies=None):
    rs = np.random.RandomState(seed)
    z = 2.0 * scale * rs.standard_normal((B + held, D))
    if copies is not None:
        dst, src = copies
        z[dst] = z[src]
    p = np.exp(z / (2.0 * scale))
    p /= p.sum(axis=1, keepdims=True)
    y = np.array([rs.choice(D, p=row) for row in p])
    k = np.rint(z[:B] * 1024).astype(np.int64)
    q = D * k - k.sum(axis=1, keepdims=True)
    P = 2 ** int(np.rint(np.log2(D)))
    assert np.abs(q).max() < 2 ** 24
    x = (q.astype(np.float64) / (1024. * P)).astype(np.float32)
    assert (x.astype(np.float64) * (1024. * P) == q).all()
    assert (np.mean(x.astype(np.float64), axis=1) == 0).all()
    return x, y[:B].astype(np.int64), z[B:].astype(np.float32)


def min_gap(C, x64):
    from scipy.special import softmax
    sc = softmax(x64 - np.mean(x64, axis=1, keepdims=True), axis=1)
    gaps = []
    for c in range(sc.shape[1]):
        d = np.diff(np.unique(sc[:, c]))
        gaps.append(d.min() if d.size else np.inf)
    return float(min(gaps))


def record(C, x, y, held, target, seed, extra=None):
    with np.errstate(divide="ignore", invalid="ignore"):
        cal = C.PAVCalibrator(x.astype(np.float64), target)
        pred = np.asarray(cal.predict(held.astype(np.float64)), dtype=np.float64)
    tx = [np.asarray(m.X_thresholds_, dtype=np.float64) for m in cal.models]
    ty = [np.asarray(m.y_thresholds_, dtype=np.float64) for m in cal.models]
    data = {"x": x, "y": y, "held": held, "thr_x": np.concatenate(tx),
            "thr_y": np.concatenate(ty), "n_thr": np.array([len(t) for t in tx], dtype=np.int64),
            "pred": pred, "log_priors": np.asarray(cal.log_priors, dtype=np.float64),
            "seed": np.int64(seed)}
    data.update(extra or {})
    return data


def _save(name, data):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **data)
    print("%s: seed=%d n_thr=%s nan=%d %d bytes" % (name, data["seed"], data["n_thr"].tolist(),
                                                   int(np.isnan(data["pred"]).sum()),
                                                   os.path.getsize(path)))
    assert os.path.getsize(path) < (1 << 20)


def main():
    C = _reference()
    for name, D, B, seed0, copies in (("ties", 3, 1000, 201, (slice(700, 1000), slice(0, 300))),
                                      ("mod", 4, 512, 202, None)):
        for seed in range(seed0, seed0 + 500, 10):
            x, y, held = make_inputs(D, B, 256, seed, copies=copies)
            gap = min_gap(C, x.astype(np.float64))
            if gap >= MIN_GAP and len(np.unique(y)) == D:
                break
        assert gap >= MIN_GAP, name
        print("%s: smallest gap between distinct scores %.3e" % (name, gap))
        _save(name, record(C, x, y, held, y, seed, {"min_gap": np.float64(gap)}))
    x, y, held = make_inputs(4, 512, 256, 203, scale=40.0)
    assert len(np.unique(y)) == 4
    _save("sat", record(C, x, y, held, y, 203))
    x, y, held = make_inputs(3, 64, 64, 204)
    y = y % 2  # class 2 never occurs
    _save("degen", record(C, x, y, held, np.eye(3)[y], 204))
    x, y, held = make_inputs(3, 1, 16, 205)
    _save("one", record(C, x, y, held, np.eye(3)[y], 205))


if __name__ == "__main__":
    main()
