#!/usr/bin/env python3
"""Which kernels of two sets of kept gfx950 listings (build/*.s) differ in their instruction stream?  A refactoring that only removes
dead switches or moves kernels between translation units must leave every surviving kernel's listing identical (labels and comments
aside).  The kernels of all listings of a directory are pooled: a kernel that moved to another file is the same kernel.
    python tools/asm_diff.py [--pair] <dir with the old *gfx950.s> [dir with the new ones, default sparse-videogen_amd/build]
--pair: a kernel whose template arguments changed has a new symbol; pair each removed kernel with an added one of identical
instruction stream (a rename) and count only the rest as removed / added.  Exit code 1 if any kernel changed or, with --pair, if
a removed or added kernel is left unpaired."""
import glob
import re
import sys
from pathlib import Path


def funcs(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = "\n".join(body)
            name = None
            continue
        t = re.sub(r";.*", "", line).strip()
        if not t or t.startswith("."):
            continue
        body.append(re.sub(r"\.LBB\d+_\d+", "LBB", t))
    return out


def pair_renames(a, b, gone, added):
    """(old, new) symbol pairs with identical bodies, and the removed / added symbols left over"""
    pairs, left = [], list(added)
    for k in gone:
        m = next((n for n in left if b[n] == a[k]), None)
        if m is not None:
            pairs.append((k, m))
            left.remove(m)
    paired = {k for k, _ in pairs}
    return pairs, [k for k in gone if k not in paired], left


def pooled(directory):
    """the kernels of every kept listing of a directory (a kernel lives in one listing; which one may change between builds)"""
    out = {}
    for f in sorted(glob.glob(directory + "/*gfx950.s")):
        out.update(funcs(f))
    return out


def main():
    args = sys.argv[1:]
    pair = "--pair" in args
    args = [x for x in args if x != "--pair"]
    old = args[0]
    new = args[1] if len(args) > 1 else str(Path(__file__).resolve().parent.parent / "sparse-videogen_amd" / "build")
    a, b = pooled(old), pooled(new)
    diff = [k for k in a if k in b and a[k] != b[k]]
    gone = [k for k in a if k not in b]
    added = [k for k in b if k not in a]
    pairs = []
    if pair:
        pairs, gone, added = pair_renames(a, b, gone, added)
    print(f"kernels {len(a):3d} -> {len(b):3d}  identical {len([k for k in a if k in b]) - len(diff):3d}  changed {len(diff)}  "
          f"removed {len(gone)}  added {len(added)}" + (f"  renamed {len(pairs)}" if pair else ""))
    for k in diff:
        print("   CHANGED", k[:110])
    for k in gone:
        print("   removed", k[:110])
    for k in added:
        print("   added  ", k[:110])
    for k, n in pairs:
        print("   renamed", k[:110], "\n        ->", n[:110])
    return 1 if diff or (pair and (gone or added)) else 0


if __name__ == "__main__":
    sys.exit(main())
