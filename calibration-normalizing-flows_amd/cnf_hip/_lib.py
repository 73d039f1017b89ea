"""ctypes binding of libcnf_hip.so (the C ABI declared in include/cnf.h).

The library is built in-tree by `make -C calibration-normalizing-flows_amd/csrc`
(or `__graft_entry__.build()`).  `torch` is imported first so the process has a
single HIP runtime: libcnf_hip.so's NEEDED libamdhip64.so.7 then resolves to
the copy torch already loaded (same SONAME).  There is no fallback: if the
library is missing, every native entry point raises.
"""
import ctypes
import os
import threading

import torch  # noqa: F401  (load torch's HIP runtime before ours)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CNF_HIP_LIB", os.path.join(_HERE, "libcnf_hip.so"))

ABI_VERSION = 2
MAX_HIDDEN = 8
MAX_DIM = 256
MAX_BINS = 64     # CNF_MAX_BINS (cnf_metrics)
LOSS_CAL = 0
LOSS_CE = 1
OPT_NO_SGPR = 1   # cnf_desc.options (include/cnf.h)
OPT_NO_WIDE = 2
OPT_ALT_MASK = 4  # legacy code-old/realNVP.py semantics (flows/legacy.py)
OPT_S_TANH = 8
SCALE_SCALAR = 0  # CNF_SCALE_* (cnf_scaling_*): t = a*x + b, a one double
SCALE_DIAG = 1    # t = w.x + b
SCALE_FULL = 2    # t = x@W + b, D <= SCALE_FULL_MAX_DIM
SCALE_FULL_MAX_DIM = 128
PAV_LDS_ENTRIES = 2048  # cnf_pav_predict stages the tables in LDS when D * cap <= this
PLANAR_MAX_LAYERS = 64  # CNF_PLANAR_MAX_LAYERS (cnf_planar_*)
PLANAR_REG_LAYERS = 10  # deeper stacks keep their tanh tape in the workspace
RADIAL_MAX_LAYERS = 64  # CNF_RADIAL_MAX_LAYERS (cnf_radial_*)
RADIAL_REG_LAYERS = 10  # deeper stacks keep their tape of r in the workspace
AFFINE_MAX_LAYERS = 64  # CNF_AFFINE_MAX_LAYERS (cnf_affine_*)
MIXED_MAX_LAYERS = 64   # CNF_MIXED_MAX_LAYERS (cnf_mixed_*)
LAYER_PLANAR = 0        # CNF_LAYER_*: a mixed stack's `kinds`
LAYER_RADIAL = 1
LAYER_AFFINE = 2
VJP_PLAN_WORDS = 16     # CNF_VJP_PLAN_WORDS (cnf_vjp_launch_plan)
VJP_PATHS = ("none", "vjp2", "vjp-rows", "layerwise", "wide-fused")  # CNF_VJP_PATH_*
# k_wgemm's instantiations in cnf_vjp_launch_plan's bit order: (BT, EPI, PAIR, NC)
WGEMM_BITS = tuple((bt, epi, pair, nc)
                   for bt, epi, pair in ((True, "bias", False), (True, "bias_relu", False),
                                         (False, "mask", False), (False, "add", True),
                                         (False, "add", False))
                   for nc in (1, 2))
# k_wdw16g's (G tiles, H tiles) classes in its bit order (CNF_DWG_CLASSES, cnf_wvjp.hip)
WDWG_CLASSES = ((7, 4), (7, 7), (4, 7), (4, 4), (4, 2), (4, 5), (1, 5))

# Every symbol include/cnf.h declares (checked by tests/test_abi.py).
EXPORTS = (
    "cnf_param_count", "cnf_param_tensor_count", "cnf_prepared_bytes", "cnf_prepare",
    "cnf_forward", "cnf_inverse", "cnf_forward_loss_workspace_bytes", "cnf_forward_loss",
    "cnf_predict", "cnf_vjp_workspace_bytes", "cnf_vjp", "cnf_loss_vjp", "cnf_adam_step",
    "cnf_adam_step_sched", "cnf_adam_step_guarded", "cnf_adam_step_tensors",
    "cnf_vjp_inverse_workspace_bytes", "cnf_vjp_inverse", "cnf_guard_nonfinite",
    "cnf_metrics_record_words", "cnf_metrics_workspace_bytes", "cnf_metrics",
    "cnf_scaling_sums_words", "cnf_scaling_workspace_bytes", "cnf_scaling_loss_grad",
    "cnf_scaling_predict",
    "cnf_pav_predict",
    "cnf_planar_param_count", "cnf_planar_workspace_bytes", "cnf_planar_launch_plan",
    "cnf_planar_forward",
    "cnf_planar_forward_loss", "cnf_planar_predict", "cnf_planar_score", "cnf_planar_vjp",
    "cnf_planar_loss_vjp",
    "cnf_radial_param_count", "cnf_radial_workspace_bytes", "cnf_radial_launch_plan",
    "cnf_radial_forward",
    "cnf_radial_forward_loss", "cnf_radial_predict", "cnf_radial_score", "cnf_radial_vjp",
    "cnf_radial_loss_vjp",
    "cnf_affine_param_count", "cnf_affine_workspace_bytes", "cnf_affine_launch_plan",
    "cnf_affine_forward", "cnf_affine_inverse",
    "cnf_affine_forward_loss", "cnf_affine_predict", "cnf_affine_score", "cnf_affine_vjp",
    "cnf_affine_loss_vjp",
    "cnf_mixed_param_count", "cnf_mixed_workspace_bytes", "cnf_mixed_launch_plan",
    "cnf_mixed_forward", "cnf_mixed_forward_loss", "cnf_mixed_predict", "cnf_mixed_score",
    "cnf_mixed_vjp", "cnf_mixed_loss_vjp",
    "cnf_kernel_name", "cnf_vjp_kernel_name", "cnf_vjp_launch_plan", "cnf_strerror", "cnf_last_hip_error", "cnf_abi_version",
)


class CnfDesc(ctypes.Structure):
    """Mirror of `cnf_desc` (include/cnf.h)."""
    _fields_ = [
        ("abi_version", ctypes.c_int32),
        ("dim", ctypes.c_int32),
        ("n_layers", ctypes.c_int32),
        ("n_hidden", ctypes.c_int32),
        ("hidden", ctypes.c_int32 * MAX_HIDDEN),
        ("scale", ctypes.c_int32),
        ("shift", ctypes.c_int32),
        ("strict_nan", ctypes.c_int32),
        ("options", ctypes.c_int32),
        ("perms", ctypes.POINTER(ctypes.c_int64)),
    ]


class CnfError(RuntimeError):
    def __init__(self, fn, status, lib):
        msg = lib.cnf_strerror(status).decode()
        if status == -5:
            msg += " (hipError %d)" % lib.cnf_last_hip_error()
        super().__init__("%s failed: %s [%d]" % (fn, msg, status))
        self.status = status


class UnsupportedShape(CnfError):
    pass


_lib = None
_lock = threading.Lock()


def _bind(lib):
    P, I32, I64, F, DB = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float,
                          ctypes.c_double)
    D = ctypes.POINTER(CnfDesc)
    sig = {
        "cnf_param_count": (ctypes.c_int, [D, ctypes.POINTER(I64)]),
        "cnf_param_tensor_count": (ctypes.c_int, [D, ctypes.POINTER(I32)]),
        "cnf_prepared_bytes": (ctypes.c_int, [D, ctypes.POINTER(ctypes.c_size_t)]),
        "cnf_prepare": (ctypes.c_int, [D, ctypes.POINTER(P), P, P]),
        "cnf_forward": (ctypes.c_int, [D, P, P, P, P, P, I64, P]),
        "cnf_inverse": (ctypes.c_int, [D, P, P, P, P, P, I64, P]),
        "cnf_forward_loss_workspace_bytes": (ctypes.c_int,
                                             [D, I64, ctypes.POINTER(ctypes.c_size_t)]),
        "cnf_forward_loss": (ctypes.c_int, [D, P, P, P, I32, F, P, P, P, I64, P, ctypes.c_size_t,
                                            P]),
        "cnf_predict": (ctypes.c_int, [D, P, P, P, P, P, I64, P]),
        "cnf_vjp_workspace_bytes": (ctypes.c_int, [D, I64, ctypes.POINTER(ctypes.c_size_t)]),
        "cnf_vjp": (ctypes.c_int, [D, P, P, P, P, P, P, P, I64, P, ctypes.c_size_t, P]),
        "cnf_loss_vjp": (ctypes.c_int, [D, P, P, P, I32, F, F, P, P, P, I64, P, ctypes.c_size_t,
                                        P]),
        "cnf_vjp_inverse_workspace_bytes": (ctypes.c_int,
                                            [D, I64, ctypes.POINTER(ctypes.c_size_t)]),
        "cnf_vjp_inverse": (ctypes.c_int, [D, P, P, P, P, P, P, P, I64, P, ctypes.c_size_t, P]),
        "cnf_adam_step": (ctypes.c_int, [D, ctypes.POINTER(P), P, P, P, I64, DB, DB, DB, DB, DB,
                                         P]),
        "cnf_adam_step_sched": (ctypes.c_int, [D, ctypes.POINTER(P), P, P, P, P, DB, DB, DB, DB,
                                               P]),
        "cnf_adam_step_guarded": (ctypes.c_int, [D, ctypes.POINTER(P), P, P, P, I64, DB, P, DB,
                                                 DB, DB, DB, P, P]),
        "cnf_adam_step_tensors": (ctypes.c_int, [I32, ctypes.POINTER(I64), ctypes.POINTER(P), P, P,
                                                 P, I64, DB, P, DB, DB, DB, DB, P, P]),
        "cnf_guard_nonfinite": (ctypes.c_int, [P, I64, P, P]),
        "cnf_metrics_record_words": (ctypes.c_int, [I32, ctypes.POINTER(I64)]),
        "cnf_metrics_workspace_bytes": (ctypes.c_int, [I32, I32, I64,
                                                       ctypes.POINTER(ctypes.c_size_t)]),
        "cnf_metrics": (ctypes.c_int, [P, P, I32, I32, I64, P, P, ctypes.c_size_t, P]),
        "cnf_scaling_sums_words": (ctypes.c_int, [I32, I32, ctypes.POINTER(I64)]),
        "cnf_scaling_workspace_bytes": (ctypes.c_int, [I32, I32, I64,
                                                       ctypes.POINTER(ctypes.c_size_t)]),
        "cnf_scaling_loss_grad": (ctypes.c_int, [P, P, I32, I32, P, P, I32, I64, P, P,
                                                 ctypes.c_size_t, P]),
        "cnf_scaling_predict": (ctypes.c_int, [P, I32, I32, P, P, P, P, I64, P]),
        "cnf_pav_predict": (ctypes.c_int, [P, I32, I64, P, P, P, I32, P, P, P]),
        "cnf_planar_param_count": (ctypes.c_int, [I32, I32, ctypes.POINTER(I64)]),
        "cnf_planar_workspace_bytes": (ctypes.c_int, [I32, I32, I64,
                                                      ctypes.POINTER(ctypes.c_size_t)]),
        "cnf_planar_launch_plan": (ctypes.c_int, [I32, I32, I64, ctypes.POINTER(I32)]),
        "cnf_planar_forward": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, P, P, I64, P,
                                              ctypes.c_size_t, P]),
        "cnf_planar_forward_loss": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, I32, F, P, P,
                                                   P, I64, P, ctypes.c_size_t, P]),
        "cnf_planar_predict": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, P, P, I64, P,
                                              ctypes.c_size_t, P]),
        "cnf_planar_score": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, P, I32, P, I64, P,
                                            ctypes.c_size_t, P]),
        "cnf_planar_vjp": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, P, P, P, P, I64, P,
                                          ctypes.c_size_t, P]),
        "cnf_planar_loss_vjp": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, I32, F, F, P, P,
                                               P, I64, P, ctypes.c_size_t, P]),
        "cnf_radial_param_count": (ctypes.c_int, [I32, I32, ctypes.POINTER(I64)]),
        "cnf_radial_workspace_bytes": (ctypes.c_int, [I32, I32, I64,
                                                      ctypes.POINTER(ctypes.c_size_t)]),
        "cnf_radial_launch_plan": (ctypes.c_int, [I32, I32, I64, ctypes.POINTER(I32)]),
        "cnf_radial_forward": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, P, I64, P,
                                              ctypes.c_size_t, P]),
        "cnf_radial_forward_loss": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, I32, P, P,
                                                   I64, P, ctypes.c_size_t, P]),
        "cnf_radial_predict": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, P, I64, P,
                                              ctypes.c_size_t, P]),
        "cnf_radial_score": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, P, I32, P, I64, P,
                                            ctypes.c_size_t, P]),
        "cnf_radial_vjp": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, P, P, P, I64, P,
                                          ctypes.c_size_t, P]),
        "cnf_radial_loss_vjp": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, I32, F, P, P, P,
                                               I64, P, ctypes.c_size_t, P]),
        "cnf_affine_param_count": (ctypes.c_int, [I32, I32, ctypes.POINTER(I64)]),
        "cnf_affine_workspace_bytes": (ctypes.c_int, [I32, I32, I64,
                                                      ctypes.POINTER(ctypes.c_size_t)]),
        "cnf_affine_launch_plan": (ctypes.c_int, [I32, I32, I64, ctypes.POINTER(I32)]),
        "cnf_affine_forward": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, P, P, I64, P,
                                              ctypes.c_size_t, P]),
        "cnf_affine_inverse": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, P, P, I64, P,
                                              ctypes.c_size_t, P]),
        "cnf_affine_forward_loss": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, I32, F, P, P,
                                                   P, I64, P, ctypes.c_size_t, P]),
        "cnf_affine_predict": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, P, I64, P,
                                              ctypes.c_size_t, P]),
        "cnf_affine_score": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, P, I32, P, I64, P,
                                            ctypes.c_size_t, P]),
        "cnf_affine_vjp": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, P, P, P, P, I64, P,
                                          ctypes.c_size_t, P]),
        "cnf_affine_loss_vjp": (ctypes.c_int, [I32, I32, ctypes.POINTER(P), P, P, I32, F, F, P, P,
                                               P, I64, P, ctypes.c_size_t, P]),
        # the planar signatures with `kinds` (a host int32 array) after n_layers
        "cnf_mixed_param_count": (ctypes.c_int, [I32, I32, ctypes.POINTER(I32),
                                                 ctypes.POINTER(I64)]),
        "cnf_mixed_workspace_bytes": (ctypes.c_int, [I32, I32, ctypes.POINTER(I32), I64,
                                                     ctypes.POINTER(ctypes.c_size_t)]),
        "cnf_mixed_launch_plan": (ctypes.c_int, [I32, I32, ctypes.POINTER(I32), I64,
                                                 ctypes.POINTER(I32)]),
        "cnf_mixed_forward": (ctypes.c_int, [I32, I32, ctypes.POINTER(I32), ctypes.POINTER(P), P,
                                             P, P, P, I64, P, ctypes.c_size_t, P]),
        "cnf_mixed_forward_loss": (ctypes.c_int, [I32, I32, ctypes.POINTER(I32),
                                                  ctypes.POINTER(P), P, P, I32, F, P, P, P, I64,
                                                  P, ctypes.c_size_t, P]),
        "cnf_mixed_predict": (ctypes.c_int, [I32, I32, ctypes.POINTER(I32), ctypes.POINTER(P), P,
                                             P, P, P, I64, P, ctypes.c_size_t, P]),
        "cnf_mixed_score": (ctypes.c_int, [I32, I32, ctypes.POINTER(I32), ctypes.POINTER(P), P, P,
                                           P, I32, P, I64, P, ctypes.c_size_t, P]),
        "cnf_mixed_vjp": (ctypes.c_int, [I32, I32, ctypes.POINTER(I32), ctypes.POINTER(P), P, P,
                                         P, P, P, P, I64, P, ctypes.c_size_t, P]),
        "cnf_mixed_loss_vjp": (ctypes.c_int, [I32, I32, ctypes.POINTER(I32), ctypes.POINTER(P), P,
                                              P, I32, F, F, P, P, P, I64, P, ctypes.c_size_t, P]),
        "cnf_kernel_name": (ctypes.c_char_p, [D]),
        "cnf_vjp_kernel_name": (ctypes.c_char_p, [D]),
        "cnf_vjp_launch_plan": (ctypes.c_int, [D, I64, I32, ctypes.POINTER(I32)]),
        "cnf_strerror": (ctypes.c_char_p, [ctypes.c_int]),
        "cnf_last_hip_error": (ctypes.c_int, []),
        "cnf_abi_version": (ctypes.c_int, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def lib():
    """The loaded library; raises (never falls back) if it cannot be loaded."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        "libcnf_hip.so not found at %s -- build it with "
                        "`make -C calibration-normalizing-flows_amd/csrc` or "
                        "`python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
                l = _bind(ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL))
                if l.cnf_abi_version() != ABI_VERSION:
                    raise RuntimeError("libcnf_hip ABI %d != %d" % (l.cnf_abi_version(),
                                                                   ABI_VERSION))
                _lib = l
    return _lib


TORCH_LIB_PATH = os.environ.get("CNF_TORCH_LIB", os.path.join(_HERE, "libcnf_torch.so"))
_ops = None
_ops_tried = False


def torch_ops():
    """torch.ops.cnf (the TORCH_LIBRARY operators of csrc/cnf_torch_ops.cpp over
    the same C ABI), or None when libcnf_torch.so was not built.  Loaded after
    libcnf_hip.so so both resolve to the one in-tree copy."""
    global _ops, _ops_tried
    if not _ops_tried:
        with _lock:
            if not _ops_tried:
                lib()
                if os.path.exists(TORCH_LIB_PATH):
                    torch.ops.load_library(TORCH_LIB_PATH)
                    _ops = torch.ops.cnf
                _ops_tried = True
    return _ops


def desc_list(d):
    """cnf_desc as the int[] the torch operators take."""
    return [d.dim, d.n_layers, d.n_hidden] + [d.hidden[i] for i in range(MAX_HIDDEN)] + \
        [d.scale, d.shift, d.strict_nan, d.options]


def check(fn, status):
    if status != 0:
        l = lib()
        raise (UnsupportedShape if status == -3 else CnfError)(fn, status, l)


def make_desc(dim, n_layers, hidden, scale=True, shift=True, strict_nan=False, perms=None,
              options=0):
    """Build a CnfDesc; `perms` is an int64 host tensor [L, D] (row[0] < 0: no perm)
    that must stay alive while the descriptor is used."""
    hidden = list(hidden)
    if len(hidden) > MAX_HIDDEN:
        raise ValueError("at most %d hidden layers" % MAX_HIDDEN)
    d = CnfDesc()
    d.abi_version = ABI_VERSION
    d.dim = int(dim)
    d.n_layers = int(n_layers)
    d.n_hidden = len(hidden)
    for i, h in enumerate(hidden):
        d.hidden[i] = int(h)
    d.scale = int(bool(scale))
    d.shift = int(bool(shift))
    d.strict_nan = int(bool(strict_nan))
    d.options = int(options)
    d.perms = None
    if perms is not None:
        assert perms.dtype == torch.int64 and perms.is_contiguous() and not perms.is_cuda
        d.perms = ctypes.cast(perms.data_ptr(), ctypes.POINTER(ctypes.c_int64))
    return d
