"""Compare the gfx950 device assembly of the kernel units between a git revision and the working tree.

    python tools/isa_diff.py REV [--pattern REGEX] [--lines N] [--tables] [--quiet]

Every *.hip unit of csrc/ is compiled to assembly with its Makefile's flags (check_lds_wait.py's
compile_asm), once from the sources of REV (git show into a temporary directory) and once from the
working tree.  Per kernel it prints `equal`, `equal but for N immediates` or `differs` with the
first lines of a diff, and the VGPRs, SGPRs, scratch and LDS bytes of the code object metadata
(REV -> tree where they changed).  Comments, directives and the numbering of local labels are not
compared.  Kernels are matched by demangled name without the parameter list and without template
arguments that are types (a rule policy); where several share such a name, the closest streams
pair up.  Kernels on one side only are listed with their size.  A refactor of the kernel sources
should leave the kernels it does not mean to change `equal`.  A v_bitop3 truth table is part of the
instruction (another table is another function) unless --tables asks to count it as an immediate: a
change of tables alone then reads `equal but for N immediates`.  --quiet prints one line per kernel.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_lds_wait import CSRC, ROOT, compile_asm, kernels  # noqa: E402

CSRC_REL = os.path.relpath(CSRC, ROOT)
NUMBER = r"-?(?:0x[0-9a-fA-F]+|\d+)"
# --tables: a v_bitop3 truth table counts as an immediate (a change of tables that must leave the
# streams alone); by default another table is another instruction
TABLES_ARE_IMMEDIATES = False


def stream(body):
    """Instructions and labels of a kernel body: no comments, directives or blank lines, local
    labels numbered in order of appearance, other symbols by name."""
    labels = {}

    def label(m):
        return labels.setdefault(m.group(0), ".L%d" % len(labels))
    out = []
    for line in body.splitlines():
        s = " ".join(line.split(";")[0].split())
        if not s or (s.startswith(".") and not s.endswith(":")):
            continue
        out.append(re.sub(r"\.L\w+", label, s))
    return out


def immediates(line):
    """(the line with its immediate operands masked, the immediates)."""
    imm = []

    def mask(m):
        imm.append(m.group(2))
        return m.group(1) + "#"
    names = "offset|bitop3" if TABLES_ARE_IMMEDIATES else "offset"
    return re.sub(r"((?:^|[ ,]|\b(?:%s):))(%s)(?=$|[ ,])" % (names, NUMBER), mask, line), imm


def kind_of(a, b):
    """Two streams -> "equal", "immediates" (they differ only there) or "differs"."""
    if a == b:
        return "equal"
    if len(a) == len(b) and all(x == y or immediates(x)[0] == immediates(y)[0] for x, y in zip(a, b)):
        return "immediates"
    return "differs"


def compare(a, b):
    """Two streams -> ("equal", 0), ("immediates", lines that differ only there) or ("differs", diff lines)."""
    kind = kind_of(a, b)
    if kind == "equal":
        return kind, 0
    if kind == "immediates":
        return kind, sum(x != y for x, y in zip(a, b))
    return kind, [d for d in difflib.unified_diff(a, b, "REV", "tree", n=0, lineterm="")][2:]


def short_name(demangled):
    """golk::band_step_kernel<8, 2, false> of `void golk::band_step_kernel<8, 2, false, golk::B3S23>(golk::B3S23)`."""
    s = re.sub(r"^void ", "", demangled)
    anon = "(anonymous namespace)::"  # (its parenthesis is not the parameter list's)
    s = s.replace(anon, "\0")
    depth = 0
    for i, c in enumerate(s):  # cut the parameter list: the first '(' outside the template arguments
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            s = s[:i]
            break
    s = s.replace("\0", anon)
    m = re.match(r"([^<]*)<(.*)>$", s)
    if not m:
        return s
    args, depth = [""], 0
    for c in m.group(2):  # the top-level template arguments
        depth += (c in "<(") - (c in ">)")
        if c == "," and depth == 0:
            args.append("")
        else:
            args[-1] += c
    args = [t.strip() for t in args]
    keep = [t for t in args if t in ("true", "false") or not re.match(r"[A-Za-z_]", t)]  # values, not types
    return "%s<%s>" % (m.group(1), ", ".join(keep))


def resources(asm):
    """mangled name -> (vgpr, sgpr, scratch, lds) from the code object metadata."""
    out = {}
    for blk in re.findall(r"- \.agpr_count.*?(?=\n  - \.agpr_count|\namdhsa\.target)", asm, re.S):
        def field(f):
            return int(re.search(r"\.%s:\s+(\d+)" % f, blk).group(1))
        out[re.search(r"\.name:\s+(\S+)", blk).group(1)] = (
            field("vgpr_count"), field("sgpr_count"), field("private_segment_fixed_size"),
            field("group_segment_fixed_size"))
    return out


def load(asm, pattern):
    """short name -> [(demangled, stream, resources)]."""
    res = resources(asm)
    found = {}
    for name, body in kernels(asm, pattern):
        if name in res and name not in found:
            found[name] = stream(body)
    names = list(found)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True,
                         check=True).stdout.splitlines() if names else []
    out = {}
    for name, d in zip(names, dem):
        out.setdefault(short_name(d), []).append((re.sub(r"^void ", "", d), found[name], res[name]))
    return out


def sources_at(rev, d):
    """csrc/ and golhip.h of a revision under d -> (csrc, include)."""
    csrc, inc = os.path.join(d, "csrc"), os.path.join(d, "include")
    os.makedirs(csrc)
    os.makedirs(inc)
    files = subprocess.run(["git", "-C", ROOT, "ls-tree", "--name-only", rev, CSRC_REL + "/"], capture_output=True,
                           text=True, check=True).stdout.split()
    for f in files + ["include/golhip.h"]:
        dst = os.path.join(inc if f.startswith("include/") else csrc, os.path.basename(f))
        with open(dst, "wb") as o:
            o.write(subprocess.run(["git", "-C", ROOT, "show", "%s:%s" % (rev, f)], capture_output=True, check=True).stdout)
    return csrc, inc


def units(csrc):
    return tuple(sorted(f for f in os.listdir(csrc) if f.endswith(".hip")))


def fmt_res(a, b=None):
    return " ".join("%s %s" % (n, x if b is None or x == y else "%d -> %d" % (x, y))
                    for n, x, y in zip(("vgpr", "sgpr", "scratch", "lds"), a, b or a))


def distance(a, b):
    """(no diff is made here: pairing n kernels of one name asks n^2 times)"""
    return {"equal": 0, "immediates": 1, "differs": 2 + abs(len(a) - len(b))}[kind_of(a, b)]


def report(old, new, lines, out=print):
    counts = {"equal": 0, "immediates": 0, "differs": 0, "unmatched": 0}
    for key in sorted(set(old) | set(new)):
        o, t = list(old.get(key, [])), list(new.get(key, []))
        while o and t:
            i, j = min(((i, j) for i in range(len(o)) for j in range(len(t))),
                       key=lambda ij: distance(o[ij[0]][1], t[ij[1]][1]))
            (_, sa, ra), (name, sb, rb) = o.pop(i), t.pop(j)
            kind, what = compare(sa, sb)
            counts[kind] += 1
            if kind == "equal":
                out("equal: %s  [%s]" % (name, fmt_res(ra, rb)))
            elif kind == "immediates":
                out("equal but for %d immediates: %s  [%s]" % (what, name, fmt_res(ra, rb)))
                for x, y in zip(sa, sb):
                    if x != y:
                        out("    %s  ->  %s" % (x, y))
            else:
                out("differs: %s  %d -> %d instructions  [%s]" % (name, len(sa), len(sb), fmt_res(ra, rb)))
                for d in what[:lines]:
                    out("    " + d)
                if len(what) > lines:
                    out("    ... %d more diff lines" % (len(what) - lines))
        for side, rest in (("only at REV", o), ("only in the tree", t)):
            for name, s, r in rest:
                counts["unmatched"] += 1
                out("%s: %s  %d instructions  [%s]" % (side, name, len(s), fmt_res(r)))
    out("%(equal)d equal, %(immediates)d equal but for immediates, %(differs)d differ, %(unmatched)d on one side only" % counts)
    return counts


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev")
    ap.add_argument("--pattern", default=r"", help="regex on the mangled kernel name")
    ap.add_argument("--lines", type=int, default=12, help="diff lines shown per differing kernel")
    ap.add_argument("--tables", action="store_true", help="count v_bitop3 truth tables as immediates")
    ap.add_argument("--quiet", action="store_true", help="one line per kernel: no instruction lines")
    args = ap.parse_args()
    global TABLES_ARE_IMMEDIATES
    TABLES_ARE_IMMEDIATES = args.tables
    with tempfile.TemporaryDirectory() as d:
        csrc, inc = sources_at(args.rev, d)
        compile_asm(os.path.join(d, "rev.s"), csrc, inc, units(csrc))
        compile_asm(os.path.join(d, "tree.s"), units=units(CSRC))
        old = load(open(os.path.join(d, "rev.s")).read(), args.pattern)
        new = load(open(os.path.join(d, "tree.s")).read(), args.pattern)
    report(old, new, args.lines, (lambda s: s.startswith("    ") or print(s)) if args.quiet else print)
    return 0


if __name__ == "__main__":
    sys.exit(main())
