#!/usr/bin/env python3
"""Compare the machine code of csrc/gru_persist.hip between a parent commit and the working tree, kernel by kernel.

    python tools/scan_isa_diff.py [--parent REV] [--diff] [--keep DIR] [--markdown]

Both trees are compiled with the Makefile's CXXFLAGS plus `-S --cuda-device-only` (no GPU needed, ~10 s each); the parent's sources come
from `git archive REV` into a scratch directory.  Each listing is cut per kernel symbol, and what cannot matter is normalised away:
comments, blank lines, assembler directives inside the body, and the numbers of local labels (.LBB / .Ltmp / .Lfunc, renumbered in order of
first appearance inside the kernel).  What is left is the instruction stream; two kernels are `identical` when theirs are equal line by
line.  The four resource counts come from the listing's metadata (.vgpr_count, .sgpr_count, .private_segment_fixed_size = scratch bytes,
.group_segment_fixed_size = static LDS bytes), printed old -> new.

One row per kernel; exit status 0 when every kernel of the parent exists in the working tree with an identical stream and equal counts.
--diff prints a unified diff of the normalised streams of the kernels that differ (read it before such a kernel runs on a GPU).
A plain differ: it knows nothing about instructions."""
import argparse
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("m3f.pytorch_amd", "csrc")
COUNTS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def makefile_flags(root):
    """CXXFLAGS and HIPCC as csrc/Makefile sets them, with $(ARCH) and $(ROOT) filled in"""
    text = open(os.path.join(root, CSRC, "Makefile")).read()
    var = {k: v.strip() for k, v in re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M)}
    var["ROOT"] = root
    flags = var["CXXFLAGS"]
    for _ in range(4):
        flags = re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), flags)
    return os.environ.get("HIPCC", var.get("HIPCC", "hipcc")), flags.split()


def listing(root, out):
    hipcc, flags = makefile_flags(root)
    cmd = [hipcc] + flags + ["-S", "--cuda-device-only", "gru_persist.hip", "-o", out]
    subprocess.run(cmd, cwd=os.path.join(root, CSRC), check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def kernels(text):
    """{symbol: (normalised instruction stream, {count name: value})} of one listing"""
    meta = {}
    for blk in re.split(r"^  - \.agpr_count:", text, flags=re.M)[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)", blk, re.M).group(1)
        meta[name] = {c: int(re.search(r"^\s+%s:\s+(\d+)" % re.escape(c), blk, re.M).group(1)) for c in COUNTS}
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        name = m.group(1)
        if name not in meta:
            continue
        labels, stream = {}, []

        def canon(lm):
            return labels.setdefault(lm.group(0), ".L%d" % len(labels))

        for line in m.group(2).split("\n"):
            line = line.split(";", 1)[0].strip()
            if not line or (line.startswith(".") and not line.startswith(".L")):
                continue                                      # comments, blank lines, directives (.p2align, .loc, ...)
            stream.append(re.sub(r"\.L(?:BB|tmp|func_\w+?)\d+(?:_\d+)?", canon, line))
        out[name] = (stream, meta[name])
    return out


def pretty(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")
    if not filt:
        return {n: n for n in names}
    res = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    short = {}
    for n, d in zip(names, res):
        d = d.replace("m3t_gru::(anonymous namespace)::", "").replace("m3t_gru::", "")
        short[n] = re.sub(r"^void ", "", d.split("(")[0])
    return short


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent", default="HEAD", help="the commit to compare the working tree against (default HEAD)")
    ap.add_argument("--diff", action="store_true", help="print the diff of every kernel whose stream changed")
    ap.add_argument("--keep", metavar="DIR", help="keep the scratch tree and both listings in DIR")
    ap.add_argument("--markdown", action="store_true", help="print the table as markdown")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="scan_isa_")
    os.makedirs(os.path.join(tmp, "parent"), exist_ok=True)
    try:
        tar = subprocess.run(["git", "archive", a.parent, CSRC, "include"], cwd=ROOT, check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", os.path.join(tmp, "parent")], input=tar, check=True)
        old = kernels(listing(os.path.join(tmp, "parent"), os.path.join(tmp, "parent.s")))
        new = kernels(listing(ROOT, os.path.join(tmp, "tree.s")))
    finally:
        if not a.keep:
            shutil.rmtree(tmp, ignore_errors=True)
    names = pretty(sorted(set(old) | set(new)))
    sep = " | " if a.markdown else "  "
    head = ["kernel", "stream", "vgpr", "sgpr", "scratch", "lds"]
    rows, same = [], 0
    for n in sorted(names, key=lambda k: names[k]):
        o, w = old.get(n), new.get(n)
        if o is None or w is None:
            rows.append([names[n], "only in the parent" if w is None else "only in the tree"] + ["-"] * 4)
            continue
        ident = o[0] == w[0]
        same += ident and o[1] == w[1]
        rows.append([names[n], "identical" if ident else "DIFFERENT (%d -> %d lines)" % (len(o[0]), len(w[0]))] +
                    ["%d" % o[1][c] if o[1][c] == w[1][c] else "%d -> %d" % (o[1][c], w[1][c]) for c in COUNTS])
        if a.diff and not ident:
            sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(o[0], w[0], "parent " + names[n], "tree " + names[n], lineterm="", n=2))
    width = [max(len(r[i]) for r in rows + [head]) for i in range(len(head))]
    for r in [head] + ([["-" * w for w in width]] if a.markdown else []) + rows:
        line = sep.join(c.ljust(w) for c, w in zip(r, width))
        print("| " + line + " |" if a.markdown else line)
    print("%d kernels in the parent, %d in the tree, %d identical in stream and counts" % (len(old), len(new), same))
    return 0 if same == len(old) == len(new) else 1


if __name__ == "__main__":
    sys.exit(main())
