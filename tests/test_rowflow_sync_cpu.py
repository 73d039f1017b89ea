"""The row families' shape dispatch and the sweep's case list agree (no GPU).

CNF_ROWFLOW_DISPATCH (csrc/cnf_rowflow.h) instantiates every planar and radial
row kernel per geometry <lpr, cpl>; tests/_rowsweep.WIDTHS is what the GPU
sweeps launch.  A geometry added to (or dropped from) the macro, a constant
that moves, or a change of launch_bwd's split fails here until the sweep
follows.  cnf_<family>_launch_plan is held to the plan _rowsweep restates, for
every case, and the case list to every reverse-mode variant the library can
select."""
import os
import re

import pytest

import _rowsweep as S
from cnf_hip import _lib, rowstack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "calibration-normalizing-flows_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def dispatch_table(src):
    """[(lpr, {case label: cpl}, default cpl)] per lanes-per-row branch of
    CNF_ROWFLOW_DISPATCH, in source order."""
    m = re.search(r"#define CNF_ROWFLOW_DISPATCH\(FN, \.\.\.\)(.*?)while \(0\)", src, re.S)
    assert m, "CNF_ROWFLOW_DISPATCH not found"
    out = []
    for body in re.findall(r"switch \(g\.cpl\) \{(.*?)\}", m.group(1), re.S):
        cases = re.findall(r"case (\d+): FN<(\d+), (\d+)>\(__VA_ARGS__\); break;", body)
        default = re.findall(r"default: FN<(\d+), (\d+)>\(__VA_ARGS__\); break;", body)
        assert len(default) == 1, body
        # nothing else launches in this branch
        assert len(re.findall(r"FN<", body)) == len(cases) + 1
        lprs = {int(l) for _, l, _ in cases} | {int(default[0][0])}
        assert len(lprs) == 1, body
        out.append((lprs.pop(), {int(n): int(c) for n, _, c in cases}, int(default[0][1])))
    return out


def check_dispatch(src):
    """Raises AssertionError unless the macro instantiates exactly the
    geometries of _rowsweep.WIDTHS and sends each to its own instantiation."""
    table = dispatch_table(src)
    fns = [(lpr, c) for lpr, cases, dflt in table for c in list(cases.values()) + [dflt]]
    assert len(fns) == len(set(fns)), "a geometry instantiated twice"
    assert sorted(fns) == S.GEOMETRIES, (sorted(set(fns) ^ set(S.GEOMETRIES)))
    assert [lpr for lpr, _, _ in table] == [1, 16, 64]
    for lpr, cases, dflt in table:
        assert all(label == cpl for label, cpl in cases.items()), (lpr, cases)
        # the default branch takes exactly one cpl of the list: its own
        mine = {c for l, c in S.GEOMETRIES if l == lpr}
        assert mine - set(cases) == {dflt}, (lpr, sorted(mine - set(cases)), dflt)


def test_dispatch_macro_is_the_sweep_list():
    check_dispatch(_src("cnf_rowflow.h"))


def test_a_dropped_or_added_geometry_fails():
    """The check itself, on mutated copies of the macro's text."""
    src = _src("cnf_rowflow.h")
    line = "        case 7: FN<1, 7>(__VA_ARGS__); break;            \\\n"
    assert line in src
    with pytest.raises(AssertionError):
        check_dispatch(src.replace(line, ""))
    with pytest.raises(AssertionError):       # one more geometry than the list
        check_dispatch(src.replace(line, line + line.replace("7", "17")))
    with pytest.raises(AssertionError):       # a label sent to another instantiation
        check_dispatch(src.replace("case 3: FN<16, 3>", "case 3: FN<16, 2>"))


def test_widths_cover_each_geometry_at_both_ends():
    assert len(S.WIDTHS) == 28 and len(S.GEOMETRIES) == 22
    for lpr, cpl in S.GEOMETRIES:
        ws = [D for D in S.WIDTHS if S.geometry(D) == (lpr, cpl)]
        if lpr == 1:
            assert ws == [cpl]
        else:                                 # most padding, no padding
            assert ws == [lpr * (cpl - 1) + 1, lpr * cpl]


def _const(src, name):
    m = re.search(r"constexpr int %s = (\d+);" % name, src)
    assert m, name
    return int(m.group(1))


def test_constants_the_sweep_mirrors():
    h, p = _src("cnf_rowflow.h"), _src("cnf_planar.hip")
    assert _const(h, "kRegL") == S.REG_L == _lib.PLANAR_REG_LAYERS == _lib.RADIAL_REG_LAYERS
    assert _const(h, "kLdsWords") == S.LDS_WORDS
    assert _const(h, "kFwdCap") == S.FWD_CAP and _const(h, "kBwdCap") == S.BWD_CAP
    assert _const(h, "kThreads") == S.THREADS and _const(h, "kFinThreads") == 64 * S.FIN_GROUPS
    assert _const(p, "kAccD") == S.ACC_D
    assert re.search(r"constexpr int kWaves = kThreads / 64;", h) and S.WAVES == S.THREADS // 64
    # the families' row sums per layer and the lanes-per-row rule
    assert "geometry(D, L, 2 * padded_dim(D) + 8, 2 * D + 2)" in p
    assert "geometry(D, L, padded_dim(D) + 8, D + 2)" in _src("cnf_radial.hip")
    assert "return D <= 16 ? 1 : D <= 64 ? 16 : 64;" in h


def test_case_list_shape():
    assert len(S.MAIN) == 2 * 28 * 2 * 2 == 224
    assert all(c.B in (1, S.ragged(c.D)) and c.L in (3, 11) for c in S.MAIN)
    assert {S.ragged(D) for D in S.WIDTHS} == {515, 35, 11}
    assert set(S.BOUNDS) <= set(S.BY_ID)
    # the boundary pairs sit on each side of kLdsWords
    pws = {c.id: S.pw(c.family, c.D, c.L) for c in S.CASES}
    for lo, hi, a, b in [("planar-d22-l64-b35", "planar-d23-l64-b35", 2948, 3076),
                         ("planar-d152-l10-b11", "planar-d153-l10-b11", 3064, 3084),
                         ("radial-d45-l64-b35", "radial-d46-l64-b35", 3012, 3076),
                         ("radial-d256-l11-b11", "radial-d256-l12-b11", 2842, 3100)]:
        assert (pws[lo], pws[hi]) == (a, b) and a <= S.LDS_WORDS < b
    assert pws["planar-d256-l64-b251"] == 32900
    assert S.finish_chunk(124) == 8 and S.finish_chunk(38) == 3
    # 38 units in chunks of 3: twelve full groups, one of 2, three empty
    assert divmod(38, 3) == (12, 2) and S.FIN_GROUPS - 13 == 3


@pytest.mark.parametrize("case", S.CASES, ids=S.IDS)
def test_launch_plan_and_workspace(case):
    """cnf_<family>_launch_plan (host only) is the restated plan, the literals
    the case is about included, and the workspace follows from it."""
    want = case.plan()
    assert rowstack.launch_plan(case.family, case.D, case.L, case.B) == want
    assert rowstack.workspace_bytes(case.family, case.D, case.L, case.B) == \
        4 * S.workspace_floats(case.family, case.D, case.L, case.B)


def test_launch_plan_argument_errors():
    import ctypes
    I32, I64 = ctypes.c_int32, ctypes.c_int64
    out = (I32 * 8)()
    for fam in S.FAMILIES:
        fn = getattr(_lib.lib(), "cnf_%s_launch_plan" % fam)
        assert fn(I32(3), I32(2), I64(8), None) == -1
        assert fn(I32(0), I32(2), I64(8), out) == -2
        assert fn(I32(3), I32(0), I64(8), out) == -2
        assert fn(I32(257), I32(2), I64(8), out) == -3
        assert fn(I32(3), I32(65), I64(8), out) == -3
        assert fn(I32(3), I32(2), I64(-1), out) == -4
        assert fn(I32(3), I32(2), I64((1 << 31) + 1), out) == -4
        assert fn(I32(3), I32(2), I64(0), out) == 0 and list(out)[5:] == [1, 1, 1]
        with pytest.raises(_lib.UnsupportedShape):
            rowstack.launch_plan(fam, 300, 2, 8)


def test_cases_cover_every_variant_the_library_can_select():
    """Every (family, lpr, cpl, reverse-mode variant) cnf_*_launch_plan reports
    anywhere in the envelope (D = 1..256, L = 1..64) is a case, and so is the
    record placement (gacc) on and off, in both families."""
    reach = set()
    for fam in S.FAMILIES:
        for D in range(1, _lib.MAX_DIM + 1):
            for L in range(1, 65):
                p = rowstack.launch_plan(fam, D, L, 1)
                assert (p["lpr"], p["cpl"]) == S.geometry(D)
                assert (p["regt"], p["rega"]) == tuple(map(int, S.variant(fam, D, L)))
                assert p["gacc"] == int(S.pw(fam, D, L) > S.LDS_WORDS)
                reach.add((fam, p["lpr"], p["cpl"], S.variant_name(p)))
    have = set()
    for c in S.CASES:
        p = c.plan()
        have.add((c.family, p["lpr"], p["cpl"], S.variant_name(p)))
    assert have == reach and len(reach) == 2 * 22 * 2
    for fam in S.FAMILIES:
        got = {(S.variant_name(c.plan()), c.plan()["gacc"]) for c in S.CASES if c.family == fam}
        assert {("tape", 0), ("tape", 1), ("regt", 0), ("rega", 0)} <= got
        # gacc under a register tape needs pw > 3072 at L <= 10: planar only (D >= 153)
        assert (("regt", 1) in got) == (fam == "planar")
    # the bounds cases: one per variant and record placement
    kinds = {(c.family, S.variant_name(c.plan()), c.plan()["lpr"], c.plan()["gacc"])
             for c in map(S.BY_ID.get, S.BOUNDS)}
    assert kinds == {("planar", "rega", 1, 0), ("radial", "rega", 1, 0), ("planar", "regt", 1, 0),
                     ("planar", "tape", 16, 0), ("radial", "tape", 16, 0),
                     ("planar", "tape", 64, 0), ("radial", "tape", 64, 0),
                     ("planar", "tape", 16, 1), ("planar", "regt", 64, 1),
                     ("radial", "tape", 16, 1), ("radial", "tape", 64, 1)}
