"""The MFMA family's reverse-mode dispatch and the sweep's case list agree (no GPU).

tests/_widesweep.py restates the constants csrc/cnf_wvjp.hip and
cnf_wide16.hip dispatch on, the launch plan that follows from them, and the
cases the GPU sweeps run.  Here the constants are parsed out of the sources, the
restated plan is held to cnf_vjp_launch_plan (and cnf_vjp_kernel_name) over a
grid of descriptors, and the cases are shown to reach every class the library
selects on that grid: a table row, a k_wdw16g class or a threshold that moves,
or a class no case launches, fails here until the sweep follows."""
import ctypes
import itertools
import os
import re

import pytest

import _widesweep as W
from cnf_hip import _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "calibration-normalizing-flows_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _const(src, name):
    m = re.search(r"constexpr \w+ %s = ([^;]+);" % name, src)
    assert m, name
    return eval(m.group(1), {"__builtins__": {}})


def check_sources(wide, wvjp):
    """Raises AssertionError unless the sources' tables and constants are
    _widesweep's."""
    m = re.search(r"const WEntry16 kW16Table\[\] = \{(.*?)\};", wide, re.S)
    assert m, "kW16Table not found"
    rows = [tuple(map(int, r)) for r in re.findall(r"CNF_W16\((\d+), (\d+), (\d+)\)", m.group(1))]
    assert len(rows) == len(re.findall(r"CNF_W16", m.group(1)))
    assert [(D, [h for h in (h1, h2) if h]) for D, h1, h2 in rows] == W.W16_TABLE
    m = re.search(r"#define CNF_DWG_CLASSES\(X\)(.*)", wvjp)
    assert m, "CNF_DWG_CLASSES not found"
    assert [tuple(map(int, c)) for c in re.findall(r"X\((\d+), (\d+)\)", m.group(1))] \
        == W.DWG_CLASSES
    m = re.search(r"F pick_nj\(int D, F f1, F f2, F f3, F f4\) \{\s*return D <= (\d+) \? f1 : "
                  r"\(D <= (\d+) \? f2 : \(D <= (\d+) \? f3 : f4\)\);", wvjp)
    assert m, "pick_nj not found"
    assert tuple(map(int, m.groups())) == W.NJ_MAX
    assert _const(wvjp, "kBN") == W.KBN and _const(wvjp, "kKC") == W.KKC
    assert _const(wvjp, "kDw16CT") == W.DW16_CT
    assert _const(wvjp, "kLds") == W.LDS_BYTES
    assert _const(wvjp, "kWdwgNkb") == W.KB_RECORDS
    assert W.NJ_MAX[-1] < _lib.MAX_DIM <= 4 * 64     # kNJ = 4 covers CNF_MAX_DIM


def test_sources_are_the_sweep_constants():
    check_sources(_src("cnf_wide16.hip"), _src("cnf_wvjp.hip"))


def test_a_dropped_row_class_or_moved_threshold_fails():
    """The check itself, on mutated copies of the sources' text."""
    wide, wvjp = _src("cnf_wide16.hip"), _src("cnf_wvjp.hip")
    for old, new, which in (("    CNF_W16(100, 100, 0),\n", "", 0),
                            ("    CNF_W16(32, 64, 64),\n",
                             "    CNF_W16(32, 64, 64),\n    CNF_W16(64, 64, 64),\n", 0),
                            (" X(4, 5)", "", 1), ("D <= 128 ? f2", "D <= 192 ? f2", 1),
                            ("constexpr int kKC = 128;", "constexpr int kKC = 64;", 1)):
        srcs = [wide, wvjp]
        assert srcs[which].count(old) == 1, old
        srcs[which] = srcs[which].replace(old, new)
        with pytest.raises(AssertionError):
            check_sources(*srcs)


@pytest.mark.parametrize("case", W.CASES, ids=[c.id for c in W.CASES])
def test_launch_plan_of_every_case(case):
    """cnf_vjp_launch_plan is the restated plan at every batch the case runs,
    has the literals the case is there for, and cnf_vjp_kernel_name the path."""
    s = W.shape_of(case)
    d = _lib.make_desc(case.D, case.L, case.hidden, case.scale, case.shift, case.strict)
    for B in case.batches + ((W.FUSED_FORWARD_BATCHES) if case.group == "fused" else ()):
        assert engine.vjp_launch_plan(d, B, case.inverse) == W.expected_plan(s, B, case.inverse)
    got = engine.vjp_launch_plan(d, case.batches[-1], case.inverse)
    assert {k: got[k] for k in case.expect} == case.expect, got
    want = "wide-fused" if case.group == "fused" else "layerwise"
    assert got["path"] == ("layerwise" if case.inverse else want)
    assert _lib.lib().cnf_vjp_kernel_name(ctypes.byref(d)).decode() == want


def test_lds_edge_is_280_281():
    """wvjp_ok's bound through the library: with two nets the paired
    first-Linear back-prop of (256, [H]) fits 160 KB up to H = 280."""
    name = lambda h: _lib.lib().cnf_vjp_kernel_name(
        ctypes.byref(_lib.make_desc(256, 2, [h]))).decode()
    assert [name(h) for h in (279, 280, 281, 288)] == ["layerwise", "layerwise", "none", "none"]
    assert W.r8(280) * 72 * 4 * 2 <= W.LDS_BYTES < W.r8(281) * 72 * 4 * 2
    D, hidden = W.PAST_LDS
    d = _lib.make_desc(D, 2, hidden)
    assert engine.vjp_launch_plan(d, 69) == {"path": "none"}
    assert engine.vjp_launch_plan(d, 69, True) == {"path": "none"}
    # one net: no paired launch, so the same width still runs
    assert engine.vjp_launch_plan(_lib.make_desc(D, 2, hidden, scale=False), 69)["path"] \
        == "layerwise"


WIDTHS = (1, 24, 64, 100, 120, 130, 136, 280, 281, 512)
HIDDEN = [[]] + [[a] for a in WIDTHS] + [[a, b] for a in WIDTHS for b in WIDTHS]
D_EDGES = (17, 32, 33, 40, 63, 64, 65, 100, 127, 128, 129, 130, 191, 192, 193, 200, 255, 256)
BATCHES = (1, 133, 261, 65541)


def _grid():
    """(D, hidden): every width 17..256 with the conditioners of kW16Table and a
    narrow one, and the widths next to a threshold with every hidden list."""
    for D in range(17, _lib.MAX_DIM + 1):
        for h in ([], [24], [100], [100, 100], [64, 64]):
            yield D, h
    for D in D_EDGES:
        for h in HIDDEN:
            yield D, h


def test_cases_cover_every_class_the_library_selects():
    """Over the grid (nets 1 and 2, strict on and off, L 1 and 2, B of
    BATCHES, forward and inverse) the library's plan is the restated one, and
    every class it is ever in is one some case is in."""
    lib = _lib.lib()
    seen = {}
    for (D, h), nets, strict, L in itertools.product(_grid(), (2, 1), (False, True), (1, 2)):
        d = _lib.make_desc(D, L, h, scale=nets == 2, shift=True, strict_nan=strict)
        s = W.Shape(D, h, L, nets == 2, True, strict)
        name = lib.cnf_vjp_kernel_name(ctypes.byref(d)).decode()
        for B, inverse in [(b, False) for b in BATCHES] + [(133, True)]:
            got = engine.vjp_launch_plan(d, B, inverse)
            assert got == W.expected_plan(s, B, inverse), (D, h, nets, strict, L, B, inverse, got)
            if B == 1:
                assert got["path"] == name
            for c in W.classes_of(got):
                seen.setdefault(c, (D, h, nets, strict, L, B, inverse))
    have = {("path", "none")}      # PAST_LDS, asserted by the layerwise GPU file
    for case in W.CASES:
        for B in case.batches:
            have |= W.classes_of(W.case_plan(case, B))
    missing = {c: at for c, at in seen.items() if c not in have}
    assert not missing, "classes no case reaches (first grid point): %r" % missing
    # and the grid is wide enough to select everything the sources instantiate
    assert {c[1] for c in seen if c[0] == "kNJ"} == {0, 1, 2, 3, 4}
    assert {c[1:] for c in seen if c[0] == "gemm"} == set(_lib.WGEMM_BITS)
    assert {c[1] for c in seen if c[0] == "chunks"} == {1, 2, 3, 4}   # r8(CNF_MAX_WIDTH) / kKC
    assert {c[1:] for c in seen if c[0] == "wdwg class"} == set(W.DWG_CLASSES)
    assert {c[1:] for c in seen if c[0] == "row x nets"} == \
        {(r, n) for r in range(len(W.W16_TABLE)) for n in (1, 2)}
    for tag in ("ny>1", "dw16_z>1", "keep_acts", "wave_blocks capped"):
        assert {c[1] for c in seen if c[0] == tag} == {False, True}, tag
    for path in ("layerwise", "wide-fused"):
        for tag in ("nkb>1", "rows_kb>256", "nseed capped"):
            assert {c[2] for c in seen if c[:2] == (path, tag)} == {False, True}, (path, tag)
