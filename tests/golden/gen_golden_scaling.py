"""Generate the scaling-calibrator fixtures (tests/golden/scaling/*.npz) FROM
THE REFERENCE ITSELF: its TempScalingCalibrator, MLRCalibrator,
VectorScalingCalibrator and MatrixScalingCalibrator (calibrators.py:57-205,
utils/ops.py:69-115) fitted on seeded logits.

Test infrastructure only; runs in the build container on the CPU, where the
reference is mounted read-only at /root/reference.  Nothing here is imported
by the product or by the tests: those read only the committed .npz files.

Inputs.  Training logits are fp32 values whose rows sum to exactly zero:
z = 1.8 * (N(0, 1) + 2 * onehot(y)) is rounded to multiples of 2^-10 (integers
k), and x_j = (D * k_j - sum_i k_i) * 2^-10 / P with P the power of two nearest
D.  Every x_j is an integer multiple of 2^-10 / P below 2^24 of them, so it is
exact in fp32 and the reference's float64 centring (calibrators.py:17) leaves
it unchanged: the reference and the fp32 device path see identical values.
The 256 held-out rows are plain fp32 draws (predict centres them itself).

  s1  D=3,   B=600     s2  D=10,  B=2000     s3  D=100, B=512
  s3m the matrix-scaling probes of s3 (10,100 parameters; no fit), in a file
      of their own so that every file stays well under 1 MiB

Per class (prefix temp_ / mlr_ / vec_ / mat_): the fitted parameters `x`
(SciPy's vector, in the reference's own packing), `fun`, `success`, `nit`,
`pred` (predict on the held-out rows, float64), and the reference's OWN
objective and gradient at three probe points -- x0, a seeded point near it,
and the fitted optimum (`probe_x`, `probe_fun`, `probe_jac`).  The fit
closures are local to `fit`; they are captured by wrapping `minimize` in the
reference modules' namespaces for the duration of the run.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_scaling.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "scaling")
HELD = 256


class _Stop(Exception):
    pass


def _reference():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import calibrators as C  # the reference's
    import utils.ops as O
    return C, O


def make_inputs(D, B, seed):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, D, size=B + HELD)
    y[:D] = np.arange(D)  # every class occurs: finite log priors
    z = rs.standard_normal((B + HELD, D))
    z[np.arange(B + HELD), y] += 2.0
    z *= 1.8
    k = np.rint(z[:B] * 1024).astype(np.int64)
    q = D * k - k.sum(axis=1, keepdims=True)
    P = 2 ** int(np.rint(np.log2(D)))
    assert np.abs(q).max() < 2 ** 24
    x = (q.astype(np.float64) / (1024. * P)).astype(np.float32)
    assert (x.astype(np.float64) * (1024. * P) == q).all()
    assert (np.mean(x.astype(np.float64), axis=1) == 0).all()
    return x, y[:B].astype(np.int64), z[B:].astype(np.float32), y[B:].astype(np.int64)


def run_class(C, O, name, cls, x64, y, held64, rs, fit=True):
    cap = {}
    real = C.minimize.__wrapped__ if hasattr(C.minimize, "__wrapped__") else C.minimize

    def wrap(fun, x0, args=(), method=None, jac=None, **kw):
        cap.update(fun=fun, jac=jac, args=args, x0=np.array(x0, dtype=np.float64, ndmin=1))
        if not fit:
            raise _Stop
        return real(fun, x0=x0, args=args, method=method, jac=jac, **kw)

    C.minimize, O.minimize = wrap, wrap
    out = {}
    try:
        try:
            cal = cls(x64, y)
        except _Stop:
            cal = None
    finally:
        C.minimize, O.minimize = real, real
    x0 = cap["x0"]
    probes = [x0, x0 + 0.1 * rs.standard_normal(x0.shape)]
    if name == "temp":
        probes[1] = np.abs(probes[1]) + 0.5
    if cal is not None:
        opt = getattr(cal, "optim", None)
        if name == "temp":
            # optim_temperature keeps only T; run the same call again for the result
            opt = real(cap["fun"], x0=1.0, args=cap["args"], method="Newton-CG", jac=cap["jac"])
            assert opt.x[0] == cal.T
        out["x"] = np.array(opt.x, dtype=np.float64)
        out["fun"] = np.float64(opt.fun)
        out["success"] = np.bool_(opt.success)
        out["nit"] = np.int64(opt.nit)
        out["pred"] = np.asarray(cal.predict(held64), dtype=np.float64)
        probes.append(out["x"].copy())
        print("  %s: success=%s nit=%d fun=%.12f  %s" % (name, opt.success, opt.nit, opt.fun,
                                                         opt.message))
    else:
        probes.append(x0 + 0.05 * rs.standard_normal(x0.shape))
    out["probe_x"] = np.stack(probes)
    out["probe_fun"] = np.array([float(cap["fun"](p, *cap["args"])) for p in probes])
    out["probe_jac"] = np.stack([np.asarray(cap["jac"](p, *cap["args"]),
                                            dtype=np.float64).reshape(-1) for p in probes])
    return {"%s_%s" % (name, k): v for k, v in out.items()}


def _save(name, data):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **data)
    print("%s: %d bytes" % (name, os.path.getsize(path)))
    assert os.path.getsize(path) < (1 << 20)


def main():
    C, O = _reference()
    classes = [("temp", C.TempScalingCalibrator), ("mlr", C.MLRCalibrator),
               ("vec", C.VectorScalingCalibrator), ("mat", C.MatrixScalingCalibrator)]
    for fx, D, B, seed0 in (("s1", 3, 600, 101), ("s2", 10, 2000, 102), ("s3", 100, 512, 103)):
        # the reference's temperature, MLR and vector fits must end success == True:
        # the first seed of seed0, seed0 + 10, ... on which all three do
        for seed in range(seed0, seed0 + 200, 10):
            x, y, held, y_held = make_inputs(D, B, seed)
            print("%s: D=%d B=%d seed=%d" % (fx, D, B, seed))
            x64, held64 = x.astype(np.float64), held.astype(np.float64)
            rs = np.random.RandomState(seed + 1000)
            data = {"x": x, "y": y, "held": held, "y_held": y_held, "seed": np.int64(seed)}
            extra = None
            ok = True
            for name, cls in classes:
                big = fx == "s3" and name == "mat"
                got = run_class(C, O, name, cls, x64, y, held64, rs, fit=not big)
                if name != "mat" and not bool(got[name + "_success"]):
                    ok = False
                    break
                if big:
                    extra = got
                else:
                    data.update(got)
            if ok:
                break
        assert ok, fx
        if extra is not None:
            _save("s3m", extra)
        _save(fx, data)


if __name__ == "__main__":
    main()
