"""Compare two directories of `make asm` listings function by function: every
function symbol's instruction text together with its .amdhsa_kernel block,
across all files of a directory (code that moved between translation units
compares equal), with the function-index part of local labels (.LBB<k>_,
.Lfunc_end<k>, .Ltmp<n>) normalised and comments dropped.  Text only.
usage: python tools/isa_diff.py OLD_DIR NEW_DIR   (exit status 0: all identical)"""
import glob
import os
import re
import sys

TYPE = re.compile(r"\s+\.type\s+(\S+),@function")
END = re.compile(r"\.Lfunc_end\d+:")
LOCAL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin)\d+")
TMP = re.compile(r"\.Ltmp\d+")


def functions(path):
    """symbol -> normalised text, from its .type line to its .Lfunc_end label"""
    out, sym, body, tmps = {}, None, [], {}
    for line in open(path):
        m = TYPE.match(line)
        if m and sym is None:
            sym, body, tmps = m.group(1), [], {}
            continue
        if sym is None:
            continue
        text = line.split(";", 1)[0].rstrip()
        if END.match(text):
            out[sym] = "\n".join(body)
            sym = None
        elif text:
            text = LOCAL.sub(lambda m: "." + m.group(1), text)
            body.append(TMP.sub(lambda m: ".Ltmp%d" % tmps.setdefault(m.group(0), len(tmps)), text))
    return out


def listing(d):
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        for sym, text in functions(path).items():
            if out.setdefault(sym, text) != text:
                sys.exit("%s: %s defined twice with different code" % (d, sym))
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = listing(sys.argv[1]), listing(sys.argv[2])
    differ = sorted(s for s in old if s in new and old[s] != new[s])
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    for tag, syms in (("differs", differ), ("only in " + sys.argv[1], only_old),
                      ("only in " + sys.argv[2], only_new)):
        for s in syms:
            print("%s: %s" % (tag, s))
    same = len(set(old) & set(new)) - len(differ)
    print("%d symbols identical, %d differ, %d on one side only" %
          (same, len(differ), len(only_old) + len(only_new)))
    sys.exit(0 if same and not differ and not only_old and not only_new else 1)


if __name__ == "__main__":
    main()
