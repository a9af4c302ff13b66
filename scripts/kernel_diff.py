#!/usr/bin/env python3
"""Compare the gfx950 device code of csrc/hvs.hip between two checkouts.  Compiles each tree's hvs.hip with that tree's own
library flags (engine.HIPCC_FLAGS minus -shared / -fPIC, plus --cuda-device-only -S), splits the assembly per function and
reports
  (a) kernels present in only one tree,
  (b) per kernel the descriptor fields that differ (VGPRs, SGPRs, accum_offset, LDS, scratch, kernel-argument size),
  (c) per function whether the instruction stream is identical after label renumbering, with a unified diff where not.
Exit status: 1 iff (a) or (b) is non-empty.  Compiles and reads text only; no GPU is needed.

    python scripts/kernel_diff.py TREE_A TREE_B [-DNAME=VALUE ...] [--keep DIR] [--quiet]
"""
import argparse
import ast
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FIELDS = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_accum_offset", ".amdhsa_group_segment_fixed_size",
          ".amdhsa_private_segment_fixed_size", ".amdhsa_kernarg_size")


def find_source(tree):
    hits = sorted(glob.glob(os.path.join(tree, "*", "csrc", "hvs.hip")))
    if len(hits) != 1:
        sys.exit(f"{tree}: expected one */csrc/hvs.hip, found {hits}")
    return hits[0]


def library_flags(src):
    engine = os.path.join(os.path.dirname(os.path.dirname(src)), "engine.py")
    for node in ast.parse(open(engine).read()).body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "HIPCC_FLAGS" for t in node.targets):
            return [f for f in ast.literal_eval(node.value) if f not in ("-shared", "-fPIC")]
    sys.exit(f"{engine}: no HIPCC_FLAGS")


def compile_asm(tree, defines, out):
    src = find_source(tree)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + library_flags(src) + defines + ["--cuda-device-only", "-S", "-Wno-unused-command-line-argument", src, "-o", out]
    subprocess.run(cmd, check=True, cwd=os.path.dirname(src))
    return open(out).read()


LABEL = re.compile(r"\.L(BB|tmp|JTI|func_begin|func_end)\d+(?:_\d+)?")


def normalise(line):
    return line.split(";", 1)[0].rstrip()  # comments carry block numbers and source positions


def renumber(body):
    """Labels of one function renamed by order of first appearance: an inserted block does not rename the ones behind it."""
    names = {}

    def new_name(m):
        return names.setdefault(m.group(0), ".L%s_%d" % (m.group(1), len(names)))

    return [LABEL.sub(new_name, line) for line in body]


def split_asm(text):
    """-> ({function: [instruction lines]}, {kernel: {field: value}})"""
    funcs, descs = {}, {}
    name, body, kernel = None, None, None
    for raw in text.splitlines():
        s = raw.strip()
        if kernel is not None:
            if s == ".end_amdhsa_kernel":
                kernel = None
            else:
                parts = s.split()
                if parts and parts[0] in FIELDS:
                    descs[kernel][parts[0]] = parts[1]
            continue
        if s.startswith(".amdhsa_kernel "):
            kernel = s.split()[1]
            descs[kernel] = {}
            continue
        m = re.match(r"\.type\s+([^,\s]+),@function", s)
        if m:
            name, body = m.group(1), None
            continue
        if name is not None and body is None:
            if raw.startswith(name + ":"):
                body = []
            continue
        if body is not None:
            if re.match(r"\.Lfunc_end\d+:", s):
                funcs[name] = renumber(body)
                name, body = None, None
                continue
            n = normalise(raw)
            if n.strip() and not n.lstrip().startswith((".p2align", ".loc", ".file", ".cfi")):
                body.append(n)
    return funcs, descs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("-D", dest="defines", action="append", default=[], metavar="NAME=VALUE", help="passed to both compilations")
    ap.add_argument("--keep", metavar="DIR", help="keep a.s / b.s there")
    ap.add_argument("--quiet", action="store_true", help="no unified diffs, only the names")
    a = ap.parse_args()
    defines = ["-D" + d for d in a.defines]
    work = a.keep or tempfile.mkdtemp(prefix="kernel_diff_")
    os.makedirs(work, exist_ok=True)
    with ThreadPoolExecutor(2) as ex:
        ja = ex.submit(compile_asm, a.tree_a, defines, os.path.join(work, "a.s"))
        jb = ex.submit(compile_asm, a.tree_b, defines, os.path.join(work, "b.s"))
        (fa, da), (fb, db) = split_asm(ja.result()), split_asm(jb.result())
    bad = 0
    print(f"kernel descriptors: {len(da)} in A, {len(db)} in B   functions: {len(fa)} in A, {len(fb)} in B   defines: {a.defines}")
    for k in sorted(set(da) ^ set(db)):
        bad += 1
        print(f"(a) only in {'A' if k in da else 'B'}: {k}")
    for k in sorted(set(da) & set(db)):
        d = [f"{f[8:]} {da[k].get(f)} -> {db[k].get(f)}" for f in FIELDS if da[k].get(f) != db[k].get(f)]
        if d:
            bad += 1
            print(f"(b) descriptor differs: {k}: " + ", ".join(d))
    differ = [f for f in sorted(set(fa) & set(fb)) if fa[f] != fb[f]]
    for f in sorted(set(fa) ^ set(fb)):
        if f not in da and f not in db:
            print(f"(c) function only in {'A' if f in fa else 'B'}: {f}")
    for f in differ:
        print(f"(c) instruction stream differs: {f} ({len(fa[f])} -> {len(fb[f])} lines)")
        if not a.quiet:
            sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(fa[f], fb[f], "A/" + f, "B/" + f, lineterm="", n=2))
    common = len(set(fa) & set(fb))
    print(f"(c) {common - len(differ)} of {common} common functions have identical instruction streams")
    print("descriptors and kernel sets identical" if not bad else f"{bad} kernel(s) differ in presence or descriptor")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
