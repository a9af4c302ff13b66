#!/usr/bin/env python3
"""Pair the kernels that scripts/kernel_diff.py lists as present in one tree only because a change gave them one more template
argument.  Reads the two assembly files kernel_diff.py leaves behind (--keep DIR: DIR/a.s, DIR/b.s), pairs every kernel that
only A has with the kernel of B whose demangled name is A's with `, false` appended to the template arguments, and reports per
pair whether the descriptors (VGPRs, SGPRs, accum offset, LDS, scratch; the kernel-argument size is listed apart) and the
instruction streams are identical.  Then lists the descriptors of the kernels that only B has and nothing pairs with: the new
forms.  Compiles nothing; no GPU is needed.

    python scripts/kernel_diff.py PARENT NEW --quiet --keep DIR ; python scripts/kernel_pair.py DIR
"""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_diff import FIELDS, split_asm  # noqa: E402


def demangle(names):
    tool = os.environ.get("CXXFILT", "c++filt")
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def head(demangled):
    """`void name<args>(params)` -> (name, args); the parameter list is dropped (the new forms add one)"""
    m = re.match(r"(?:void )?([A-Za-z_0-9]+)<(.*)>\(", demangled)
    return (m.group(1), m.group(2)) if m else (demangled, "")


def main():
    work = sys.argv[1]
    fa, da = split_asm(open(os.path.join(work, "a.s")).read())
    fb, db = split_asm(open(os.path.join(work, "b.s")).read())
    only_a, only_b = sorted(set(da) - set(db)), sorted(set(db) - set(da))
    dem = demangle(only_a + only_b)
    by_head = {head(dem[k]): k for k in only_b}
    paired, same_desc, same_code, grew = 0, 0, 0, 0
    used = set()
    for k in only_a:
        name, args = head(dem[k])
        kb = by_head.get((name, args + ", false"))
        if kb is None:
            print(f"unpaired in A: {dem[k]}")
            continue
        paired += 1
        used.add(kb)
        d = [f"{f[8:]} {da[k].get(f)} -> {db[kb].get(f)}" for f in FIELDS[:-1] if da[k].get(f) != db[kb].get(f)]
        same_desc += not d
        code_a, code_b = [line.replace(k, "SELF") for line in fa[k]], [line.replace(kb, "SELF") for line in fb[kb]]  # (section names carry the kernel's own)
        same_code += code_a == code_b
        grew += da[k].get(FIELDS[-1]) != db[kb].get(FIELDS[-1])
        if d or code_a != code_b:
            print(f"DIFFERS: {name}<{args}>: {', '.join(d) or 'descriptors equal'}; instruction stream {'equal' if code_a == code_b else 'differs'}")
    print(f"{paired} of {len(only_a)} kernels of A paired with B's form with one more `false`: {same_desc} with identical descriptors, "
          f"{same_code} with identical instruction streams, {grew} with a larger kernel-argument segment")
    new = [k for k in only_b if k not in used]
    print(f"{len(new)} kernels only in B (new forms): name, VGPRs, SGPRs, LDS bytes, scratch bytes")
    for k in sorted(new, key=lambda k: dem[k]):
        name, args = head(dem[k])
        d = db[k]
        print(f"  {name}<{args}>: {d.get(FIELDS[0])} {d.get(FIELDS[1])} {d.get(FIELDS[3])} {d.get(FIELDS[4])}")
    return 0 if paired == len(only_a) == same_desc == same_code else 1


if __name__ == "__main__":
    sys.exit(main())
