"""The argument checks of every launching cnf_planar_* / cnf_radial_* /
cnf_affine_* / cnf_mixed_* entry point, and their order, without a GPU.

Every call below carries at least one fault, so it returns before any HIP
call; the pointers are fake.  One table serves the four families: an entry
point is its argument names (HEADS, SIGS), a fault is a set of overrides of the
good call plus the status it earns alone (FAULTS), and a fault applies to an
entry point that has the arguments it overrides -- the `kinds` faults to the
mixed family's, whose head carries `kinds` after n_layers and whose parameter
table is packed, 3 + 2 entries for KINDS.  PAIRS pins the order of the checks:
a call carrying both faults of a pair returns the status of the first.

The order: shape, kinds (null, then each value), batch,
parameter table (entry by entry: null, then alignment), x / workspace null or
short, x / workspace alignment; then per kind of call -- forward: loss kind,
loss nulls, loss alignment, output alignment; reverse: grads null, the loss
checks, alignment; predict: nulls, alignment; score: shape, kinds, the scoring
arguments, then as predict."""
import ctypes

import pytest

from cnf_hip import _lib, rowstack

P = ctypes.c_void_p
I32, I64, F32, SZ = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
D, L, B = 3, 2, 8
KINDS = [0, 2]                  # mixed: planar + affine
N_TABLE = {"planar": 3 * L, "radial": 3 * L, "affine": 2 * L, "mixed": 3 + 2}

HEADS = dict.fromkeys(("planar", "radial", "affine"), "dim L params x")
HEADS["mixed"] = "dim L kinds params x"
TAIL = "B ws wb stream"
_FWD_LD, _FWD = "z ld z_all", "z z_all"
_LOSS_LD, _LOSS = "y kind det z ld terms", "y kind z terms"
_VJP_LD, _VJP = "gz gz_all gld grads dx", "gz gz_all grads dx"
_LV_DET, _LV = "y kind det gscale terms grads dx", "y kind gscale terms grads dx"
_SCORE = "lp y bins record"
SIGS = {
    "planar": {"forward": _FWD_LD, "forward_loss": _LOSS_LD, "predict": "lp probs ld",
               "score": _SCORE, "vjp": _VJP_LD, "loss_vjp": _LV_DET},
    "radial": {"forward": _FWD, "forward_loss": _LOSS, "predict": "lp probs",
               "score": _SCORE, "vjp": _VJP, "loss_vjp": _LV},
    "affine": {"forward": _FWD_LD, "inverse": _FWD_LD, "forward_loss": _LOSS_LD,
               "predict": "lp probs", "score": _SCORE, "vjp": _VJP_LD, "loss_vjp": _LV_DET},
}
SIGS["mixed"] = SIGS["planar"]
ENTRIES = [(fam, e) for fam in SIGS for e in SIGS[fam]]
assert len(ENTRIES) == 19 + 6


def names(fam, entry):
    return (HEADS[fam] + " " + SIGS[fam][entry] + " " + TAIL).split()


def kinds_of(fam, vals=KINDS):
    """The `kinds` argument of a family's calls (none unless its head has one)."""
    return (I32 * len(vals))(*vals) if "kinds" in HEADS[fam] else None


CTYPES = {"dim": I32, "L": I32, "kind": I32, "bins": I32, "B": I64, "det": F32, "gscale": F32,
          "wb": SZ}
GOOD = {"dim": D, "L": L, "B": B, "kind": 0, "bins": 15, "det": 1.0, "gscale": 1.0, "stream": 0}

# name: (overrides, status alone).  "bad" lists (index, value) pairs written
# into the parameter table (index -1: the last entry, N_TABLE - 1);
# "only" restricts a fault to entry points that have that argument.
FAULTS = {
    "kinds_null": ({"kinds": None}, -1),
    "kinds_bad_first": ({"kinds": [3, 2]}, -2),
    "kinds_bad_last": ({"kinds": [0, -1]}, -2),
    "dim_big": ({"dim": 300}, -3),
    "dim_zero": ({"dim": 0}, -2),
    "layers_zero": ({"L": 0}, -2),
    "layers_big": ({"L": 65}, -3),
    "batch_neg": ({"B": -1}, -4),
    "batch_big": ({"B": (1 << 31) + 1}, -4),
    "table_null": ({"params": None}, -1),
    "entry_null_first": ({"bad": [(0, 0)]}, -1),
    "entry_null_last": ({"bad": [(-1, 0)]}, -1),
    "entry_mis_first": ({"bad": [(0, 4098)]}, -6),
    "entry_mis_last": ({"bad": [(-1, 4098)]}, -6),
    "entry_mis0_null1": ({"bad": [(0, 4098), (1, 0)]}, -6),
    "entry_null0_mis1": ({"bad": [(0, 0), (1, 4098)]}, -1),
    "x_null": ({"x": 0}, -1),
    "ws_null": ({"ws": 0}, -1),
    "ws_short": ({"wb": -4}, -1),                 # relative to the workspace's size
    "x_mis": ({"x": 18}, -6),
    "ws_mis": ({"ws": 18}, -6),
    "kind_bad": ({"kind": 7}, -2),
    "kind_two": ({"kind": 2}, -2),
    "terms_null": ({"terms": 0}, -1),
    "y_null": ({"y": 0}, -1),
    "y_mis": ({"y": 20}, -6),
    "terms_mis": ({"terms": 18}, -6),
    "z_mis": ({"z": 18}, -6),
    "ld_mis": ({"ld": 18}, -6),
    "z_all_mis": ({"z_all": 18}, -6),
    "grads_null": ({"grads": 0}, -1),
    "gz_mis": ({"gz": 18}, -6),
    "gz_all_mis": ({"gz_all": 18}, -6),
    "gld_mis": ({"gld": 18}, -6),
    "grads_mis": ({"grads": 18}, -6),
    "dx_mis": ({"dx": 18}, -6),
    "lp_null": ({"lp": 0}, -1),
    "probs_null": ({"probs": 0}, -1),
    "lp_mis": ({"lp": 18}, -6),
    "probs_mis": ({"probs": 18}, -6),
    "bins_zero": ({"bins": 0}, -2),
    "bins_big": ({"bins": _lib.MAX_BINS + 1}, -2),
    "dim_one": ({"dim": 1, "only": "bins"}, -2),
    "batch_score_cap": ({"B": (1 << 26) + 1, "only": "bins"}, -4),
    "record_null": ({"record": 0}, -1),
    "record_mis": ({"record": 20}, -6),
}

# (earlier check, later check): both in one call return the earlier's status
PAIRS = [
    ("dim_big", "batch_neg"),             # shape before batch: -3
    ("batch_neg", "table_null"),          # batch before the table: -4
    ("entry_mis_last", "ws_short"),       # the table before the workspace: -6
    ("entry_null_last", "x_mis"),         # -1
    ("ws_short", "x_mis"),                # nulls / sizes before alignment: -1
    ("x_mis", "kind_bad"),                # the common checks before the loss checks: -6
    ("ws_short", "z_mis"),                # ... and before the outputs' alignment: -1
    ("kind_bad", "terms_null"),           # loss: kind, nulls, alignment: -2
    ("kind_bad", "y_null"),
    ("terms_null", "y_mis"),              # -1
    ("y_null", "terms_mis"),
    ("terms_null", "z_mis"),              # the loss checks before the outputs' alignment
    ("x_mis", "grads_null"),              # reverse: common, grads, loss, alignment: -6
    ("grads_null", "kind_bad"),           # -1
    ("grads_null", "gz_mis"),
    ("kind_bad", "dx_mis"),               # -2
    ("terms_null", "grads_mis"),          # -1
    ("ws_short", "lp_mis"),               # predict: common, nulls, alignment: -1
    ("x_mis", "lp_null"),                 # -6
    ("x_mis", "probs_null"),
    ("probs_null", "lp_mis"),             # -1
    ("lp_null", "probs_mis"),
    ("dim_big", "bins_zero"),             # score: the shape first: -3
    ("layers_big", "bins_zero"),
    ("bins_zero", "batch_neg"),           # the scoring arguments: -2 ...
    ("batch_score_cap", "table_null"),    # ... before the common checks: -4
    ("record_mis", "table_null"),         # -6
    ("record_null", "entry_mis_first"),   # -1
    ("record_mis", "lp_null"),
    ("dim_big", "kinds_null"),            # the shape before kinds: -3
    ("layers_big", "kinds_bad_first"),
    ("kinds_null", "batch_neg"),          # kinds directly after the shape: -1 ...
    ("kinds_bad_last", "batch_neg"),      # ... -2
    ("kinds_bad_first", "table_null"),    # -2
    ("kinds_null", "entry_mis_first"),    # -1
    ("kinds_null", "bins_zero"),          # score: kinds before the scoring arguments: -1
    ("kinds_bad_last", "record_null"),    # -2
    ("kinds_bad_first", "x_mis"),
]


def _applies(fault, args):
    over = FAULTS[fault][0]
    return all(over["only"] in args if k == "only" else k in args or k == "bad" for k in over)


def _cases():
    out = []
    for fam, entry in ENTRIES:
        args = names(fam, entry)
        for f in FAULTS:
            if _applies(f, args):
                out.append((fam, entry, (f,), FAULTS[f][1]))
        for a, b in PAIRS:
            if _applies(a, args) and _applies(b, args):
                assert FAULTS[a][1] != FAULTS[b][1], (a, b)   # or the pair shows nothing
                out.append((fam, entry, (a, b), FAULTS[a][1]))
    return out


CASES = _cases()
IDS = ["%s_%s-%s" % (fam, entry, "+".join(fs)) for fam, entry, fs, _ in CASES]


def call(fam, entry, faults):
    nt = N_TABLE[fam]
    vals = dict(GOOD, kinds=KINDS)
    vals["wb"] = rowstack.workspace_bytes(fam, D, L, B, kinds_of(fam))
    table = [4096 + 64 * i for i in range(nt)]
    null_table = False
    for f in faults:
        for k, v in FAULTS[f][0].items():
            if k == "bad":
                for i, p in v:
                    table[i] = p
            elif k == "params":
                null_table = True
            elif k == "wb":
                vals["wb"] += v
            elif k != "only":
                vals[k] = v
    vals["params"] = None if null_table else (P * nt)(*table)
    vals["kinds"] = None if vals["kinds"] is None else kinds_of(fam, vals["kinds"])
    args = []
    for n in names(fam, entry):
        v = vals.get(n, 16)                      # any other argument: a fake aligned pointer
        args.append(v if n in ("params", "kinds") else CTYPES.get(n, P)(v))
    return getattr(_lib.lib(), "cnf_%s_%s" % (fam, entry))(*args)


@pytest.mark.parametrize("fam,entry,faults,status", CASES, ids=IDS)
def test_status_and_precedence(fam, entry, faults, status):
    assert L == len(KINDS) and call(fam, entry, faults) == status


def test_table_covers_every_entry_point_and_fault():
    assert len(IDS) == len(set(IDS))
    exports = sorted(n for n in _lib.EXPORTS if n.split("_")[1] in SIGS and
                     n.split("_", 2)[2] not in ("param_count", "workspace_bytes", "launch_plan"))
    assert exports == sorted("cnf_%s_%s" % fe for fe in ENTRIES)
    used = {f for _, _, fs, _ in CASES for f in fs}
    assert used == set(FAULTS)
    hit = {fs for _, _, fs, _ in CASES if len(fs) == 2}
    assert hit == set(PAIRS)
    for fam, entry in ENTRIES:
        mine = {fs for f, e, fs, _ in CASES if (f, e) == (fam, entry)}
        # the common checks reach every entry point
        assert {("dim_big",), ("batch_neg",), ("table_null",), ("entry_null_last",),
                ("entry_mis_last",), ("ws_short",), ("x_mis",), ("dim_big", "batch_neg"),
                ("batch_neg", "table_null"), ("entry_mis0_null1",), ("ws_short", "x_mis")} <= mine
        assert (("kind_bad", "terms_null") in mine) == ("loss" in entry)
        assert (("bins_zero", "batch_neg") in mine) == (entry == "score")
        assert (("grads_null",) in mine) == ("vjp" in entry)
        # the kinds checks reach exactly the entry points that take kinds
        has_kinds = "kinds" in names(fam, entry)
        assert has_kinds == (fam == "mixed") == any("kinds" in f for fs in mine for f in fs)
        if has_kinds:
            assert {("kinds_null",), ("kinds_bad_first",), ("kinds_bad_last",),
                    ("dim_big", "kinds_null"), ("kinds_null", "batch_neg"),
                    ("kinds_bad_last", "batch_neg")} <= mine
            assert (("kinds_null", "bins_zero") in mine) == (entry == "score")


@pytest.mark.parametrize("fam,entry", [fe for fe in ENTRIES if "loss" not in fe[1]
                                       and "vjp" not in fe[1]])
def test_empty_batch_without_outputs_needs_no_device(fam, entry):
    """B == 0 with null buffers returns OK before any HIP call (the entry
    points that zero something at B == 0 run in tests/test_gpu_rowflow_empty.py)."""
    nt = N_TABLE[fam]
    vals = dict(GOOD, B=0, wb=0, record=16, kinds=kinds_of(fam),
                params=(P * nt)(*[4096 + 64 * i for i in range(nt)]))
    args = [vals[n] if n in ("params", "kinds") else CTYPES.get(n, P)(vals.get(n, 0))
            for n in names(fam, entry)]
    assert getattr(_lib.lib(), "cnf_%s_%s" % (fam, entry))(*args) == 0
