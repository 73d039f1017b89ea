"""Instruction census of a line range of an ISA listing (make asm, or hipcc -S
--cuda-device-only with the Makefile's flags): one JSON line of counts by
class -- packed FMAs, transcendental exps, other VALU, lane reads / writes
(the SGPR-spill traffic), nops, waits, scalar ALU, scalar loads, LDS and
global memory instructions.  The ranges of a kernel's blocks (prologue, layer
loop, epilogue) are read off the listing's block labels by hand: the
compiler's block layout moves between builds.
usage: isa_census.py LISTING.s FIRST-LAST[,FIRST-LAST...] [label]   (1-based, inclusive)"""
import json
import re
import sys

CLASSES = [
    ("v_pk_fma_f32", r"v_pk_fma_f32\b"),
    ("v_exp_f32", r"v_exp_f32"),
    ("lane_rw", r"v_(readlane|writelane)_b32"),
    ("valu_other", r"v_"),
    ("s_nop", r"s_nop\b"),
    ("s_waitcnt", r"s_waitcnt\b"),
    ("s_load", r"s_load_"),
    ("salu", r"s_"),
    ("ds", r"ds_"),
    ("global", r"global_"),
]


def census(lines):
    out = {k: 0 for k, _ in CLASSES}
    out["other"] = 0
    for l in lines:
        t = l.strip()
        if not t or t.startswith((";", ".", "#")) or t.endswith(":") or re.match(r"[.\w$]+:", t):
            continue
        for k, pat in CLASSES:
            if re.match(pat, t):
                out[k] += 1
                break
        else:
            out["other"] += 1
    out["valu"] = out["v_pk_fma_f32"] + out["v_exp_f32"] + out["lane_rw"] + out["valu_other"]
    out["total"] = sum(v for k, v in out.items() if k != "valu")
    return out


if __name__ == "__main__":
    path, spans = sys.argv[1], sys.argv[2]
    text = open(path).read().split("\n")
    lines = []
    for span in spans.split(","):
        a, b = (int(v) for v in span.split("-"))
        lines += text[a - 1:b]
    r = census(lines)
    r["lines"] = spans
    if len(sys.argv) > 3:
        r["block"] = sys.argv[3]
    print(json.dumps(r))
