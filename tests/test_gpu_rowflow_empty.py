"""The row families' B == 0 contract on the device, through the C ABI: every
launching entry point returns OK, zeroes exactly what an empty batch defines
(the three loss terms, the flat gradient, affine's one-number log-det) and
writes nothing else.  Every buffer starts at a sentinel; the values are exact."""
import ctypes

import pytest
import torch

import test_rowflow_args_cpu as T
from cnf_hip import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, L = 3, 2
SENTINEL = 7
# the flat gradient of L layers; mixed: T.KINDS, one planar and one affine layer
GRAD_FLOATS = {"planar": L * (2 * D + 1), "radial": L * (D + 2), "affine": L * 2 * D,
               "mixed": (2 * D + 1) + 2 * D}
assert (D, L) == (T.D, T.L) and GRAD_FLOATS["mixed"] == 13
N = 64                                    # elements per buffer, more than any GRAD_FLOATS + 1
INT64 = ("y", "record")


def _zeroed(fam, entry):
    """{argument: leading elements an empty batch zeroes}"""
    out = {}
    if "loss" in entry:
        out["terms"] = 3
    if "vjp" in entry:
        out["grads"] = GRAD_FLOATS[fam]
    if fam == "affine" and entry in ("forward", "inverse", "forward_loss"):
        out["ld"] = 1
    return out


@pytest.mark.parametrize("fam,entry", T.ENTRIES)
def test_empty_batch(fam, entry):
    names, nt = T.names(fam, entry), T.N_TABLE[fam]
    params = [torch.full((D,), float(SENTINEL), device=DEV) for _ in range(nt)]
    bufs = {n: torch.full((N,), SENTINEL, device=DEV,
                          dtype=torch.int64 if n in INT64 else torch.float32)
            for n in names if n not in T.CTYPES and n not in ("kinds", "params", "stream")}
    vals = dict(T.GOOD, B=0, wb=4 * N, stream=torch.cuda.current_stream(DEV).cuda_stream,
                kinds=T.kinds_of(fam), params=(T.P * nt)(*[p.data_ptr() for p in params]))
    vals.update({n: t.data_ptr() for n, t in bufs.items()})
    args = [vals[n] if n in ("kinds", "params") else T.CTYPES.get(n, T.P)(vals[n]) for n in names]
    with torch.cuda.device(DEV):
        st = getattr(_lib.lib(), "cnf_%s_%s" % (fam, entry))(*args)
    torch.cuda.synchronize(DEV)
    assert st == 0
    zeroed = _zeroed(fam, entry)
    assert set(zeroed) <= set(bufs)
    for n, t in bufs.items():
        k = zeroed.get(n, 0)
        got = t.cpu()
        assert (got[:k] == 0).all() and (got[k:] == SENTINEL).all(), (n, k, got.tolist())
    assert all((p.cpu() == SENTINEL).all() for p in params)
