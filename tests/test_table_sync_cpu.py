"""The compile-time kernel tables and the sweep's shape list agree (no GPU).

Every row of kTable / kLTable (cnf_valu.hip), kSTable (cnf_sgpr.hip), kVTable
(cnf_vjp.hip) and kV2Part{A,B,C} (cnf_vjp2_*.hip) is its own set of template
instantiations; tests/_sweep.NARROW is what the GPU sweeps launch.  A row
added to (or dropped from) a table fails here until the sweep follows.  The
dispatch queries (cnf_kernel_name, cnf_vjp_kernel_name) are held to the rule
the dispatch code implies, written out in _sweep.expected_*."""
import ctypes
import os
import re

import pytest

import _sweep
from cnf_hip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "calibration-normalizing-flows_amd", "csrc")


def _shipped(src):
    """The source without the branches only a *_DEV development build compiles."""
    out, stack = [], []
    for line in src.splitlines():
        m = re.match(r"\s*#\s*(ifdef|ifndef|if|else|endif)\b\s*(\w*)", line)
        if m:
            kind, name = m.group(1), m.group(2)
            if kind in ("ifdef", "ifndef", "if"):
                dev = kind != "if" and name.endswith("_DEV")
                stack.append([dev, kind == "ifndef" or not dev])
            elif kind == "else":
                if stack[-1][0]:
                    stack[-1][1] = not stack[-1][1]
            else:
                stack.pop()
            continue
        if all(active for _, active in stack):
            out.append(line)
    assert not stack
    return "\n".join(out)


def _rows(files, macro):
    rows = []
    for name in files:
        src = _shipped(open(os.path.join(CSRC, name)).read())
        rows += [tuple(map(int, m)) for m in
                 re.findall(r"\b%s\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)" % macro, src)]
    return rows


def _key(D, hidden):
    h = list(hidden) + [0, 0]
    return (D, h[0], h[1])


def _const(name, pattern):
    src = open(os.path.join(CSRC, name)).read()
    m = re.search(pattern, src)
    assert m, (name, pattern)
    return m


ALL = [_key(D, h) for D, h, _ in _sweep.NARROW]
SGPR = [_key(D, h) for D, h, s in _sweep.NARROW if s]


def test_shipped_filter_drops_dev_branches():
    src = "a\n#ifdef X_DEV\nb\n#else\nc\n#endif\n#ifndef X_DEV\nd\n#endif\n#ifdef T\ne\n#endif"
    assert _shipped(src).split() == ["a", "c", "d", "e"]


def test_sweep_list_shape():
    assert len(ALL) == 18 and len(set(ALL)) == 18
    assert len(SGPR) == 15
    assert sorted(set(ALL) - set(SGPR)) == [(10, 7, 0), (10, 10, 0), (10, 10, 10)]
    assert len(_sweep.TANH) == 3


def test_valu_table_is_the_sweep_list():
    rows = _rows(["cnf_valu.hip"], "CNF_VALU")
    assert len(rows) == len(set(rows))
    assert rows == ALL


def test_valu_tanh_table_is_the_sweep_list():
    rows = _rows(["cnf_valu.hip"], "CNF_VALU_TANH")
    assert rows == [_key(D, h) for D, h in _sweep.TANH]


def test_sgpr_table_is_the_sweep_list():
    rows = _rows(["cnf_sgpr.hip"], "CNF_SGPR")
    assert len(rows) == len(set(rows))
    assert sorted(rows) == sorted(SGPR)


def test_vjp_table_is_the_sweep_list():
    rows = _rows(["cnf_vjp.hip"], "CNF_VJP")
    assert len(rows) == len(set(rows))
    assert sorted(rows) == sorted(ALL)


def test_vjp2_parts_are_the_sweep_list():
    rows = _rows(["cnf_vjp2_a.hip", "cnf_vjp2_b.hip", "cnf_vjp2_c.hip"], "CNF_V2")
    assert sorted(set(rows)) == sorted(SGPR)
    # find_v2 takes the first match: a row in two parts would be dead code
    assert len(rows) == len(set(rows))


def test_constants_the_gpu_tests_mirror():
    m = _const("cnf_valu.hip", r"constexpr int64_t kLargeBatch = (\d+)ll << (\d+);")
    assert int(m.group(1)) << int(m.group(2)) == _sweep.LARGE_BATCH
    assert int(_const("cnf_vjp2.h", r"constexpr int kV2LMax = (\d+);").group(1)) == _sweep.V2_LMAX
    assert int(_const("cnf_vjp.hip", r"constexpr int kVRows = (\d+);").group(1)) == _sweep.VJP_ROWS
    assert int(_const("cnf_vjp.hip", r"constexpr int kGP = (\d+);").group(1)) == _sweep.VJP_GP
    # the bound vjp_path() holds k_vjp's LDS estimate to
    assert _const("cnf_vjp.hip", r"lds_bytes\(s, \*e\) <= 64 \* 1024\) return VjpPath::kRows")


def _names(D, L, hidden, **kw):
    d = _lib.make_desc(D, L, hidden, **kw)
    lib = _lib.lib()
    return (lib.cnf_kernel_name(ctypes.byref(d)).decode(),
            lib.cnf_vjp_kernel_name(ctypes.byref(d)).decode())


@pytest.mark.parametrize("D,hidden,sg", _sweep.NARROW,
                         ids=[_sweep.shape_id(D, h) for D, h, _ in _sweep.NARROW])
def test_dispatch_names_follow_the_rule(D, hidden, sg):
    ek, ev = _sweep.expected_kernel, _sweep.expected_vjp_path
    # RealNVP, L = 3 and L = 9 (past kV2LMax)
    for L in (3, 9):
        assert _names(D, L, hidden) == (ek(D, hidden), ev(D, hidden, L)), L
    assert _names(D, 3, hidden)[1] == ("vjp2" if sg else "vjp-rows")
    # NICE
    assert _names(D, 4, hidden, scale=False) == (ek(D, hidden), ev(D, hidden, 4, scale=False))
    # shift=False: neither scalar-weight kernel
    assert _names(D, 3, hidden, shift=False) == ("valu-fused", "vjp-rows")
    assert ev(D, hidden, 3, shift=False) == "vjp-rows"
    # OPT_NO_SGPR keeps forward launches off k_sgpr; the reverse mode is unchanged
    assert _names(D, 3, hidden, options=_lib.OPT_NO_SGPR) == ("valu-fused", ev(D, hidden, 3))
    # strict_nan: k_valu's strict instantiations; reverse mode layer at a time
    assert _names(D, 3, hidden, strict_nan=True) == ("valu-fused", "layerwise")
    assert ev(D, hidden, 3, strict=True) == "layerwise"


def test_l9_rows_kernel_gives_way_where_its_lds_estimate_passes_64k():
    got = {(D, tuple(h)): _names(D, 9, h)[1] for D, h, _ in _sweep.NARROW}
    assert got.pop((10, (10, 10))) == "layerwise"
    assert set(got.values()) == {"vjp-rows"}


def test_vjp_kernel_name_outside_the_tables():
    name = lambda *a, **k: _names(*a, **k)[1]
    assert name(100, 12, [100, 100]) == "wide-fused"
    assert name(100, 12, [100, 100], options=_lib.OPT_NO_WIDE) == "layerwise"
    assert name(100, 12, [100, 100], strict_nan=True) == "layerwise"
    assert name(7, 3, [5, 5]) == "layerwise"
    assert name(256, 2, [512]) == "none"
    d = _lib.make_desc(10, 3, [5, 5])
    d.dim = 1
    assert _lib.lib().cnf_vjp_kernel_name(ctypes.byref(d)).decode() == "none"
    # legacy options: the layer-at-a-time kernels
    assert name(10, 4, [10], options=_lib.OPT_ALT_MASK | _lib.OPT_S_TANH) == "layerwise"
