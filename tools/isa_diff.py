#!/usr/bin/env python3
"""Compare the kernels of two hipcc -S listings (hipcc <CXXFLAGS> --cuda-device-only -S file.hip), instruction for instruction:

    tools/isa_diff.py parent.s this.s [--rename 'REGEX=>REPL' ...] [--only REGEX]

Kernels are paired by demangled name without the argument list, e.g. `k_convdiff_adjoint<3, 3, true>`.  --rename rewrites the names of the
FIRST listing before pairing (re.sub, applied in order), for a kernel that changed its name or template arguments:
    --rename 'k32a_momentum_pullback<(\\d), (\\w+)>=>k_convdiff_adjoint<\\1, float, 3, \\2>'
Two bodies are identical when their instruction sequences agree after comments, directives and symbol names are dropped and local labels
are renumbered in order of appearance.  Prints one markdown table row per kernel: instruction counts, identical or not, and VGPR / SGPR /
scratch bytes from the listing's metadata (first listing -> second where they differ).  Exit status 1 if any pair differs or is unpaired.
"""
import argparse, re, subprocess, sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    res = {}
    for n, d in zip(names, out):
        d = d.replace("void ", "", 1).replace("(anonymous namespace)::", "")
        depth, cut = 0, len(d)
        for p, ch in enumerate(d):  # the argument list opens at the first '(' outside the template brackets
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0:
                cut = p
                break
        res[n] = d[:cut]
    return res


def kernels(path):
    s = open(path).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", s.split("amdhsa.kernels:")[1], re.S):
        f = dict(re.findall(r"\.(vgpr_count|sgpr_count|private_segment_fixed_size):\s+(\d+)", m.group(0)))
        meta[m.group(1)] = (int(f["vgpr_count"]), int(f["sgpr_count"]), int(f["private_segment_fixed_size"]))
    names = demangle(list(meta))
    res = {}
    for sym, short in names.items():
        body = re.search(r"^" + re.escape(sym) + r":[^\n]*\n(.*?)\n\.Lfunc_end", s, re.S | re.M).group(1)
        labels, ins = {}, []
        for line in body.split("\n"):
            line = line.split(";")[0].rstrip()
            if not line.strip() or line.lstrip().startswith(".") and not line.rstrip().endswith(":"):
                continue
            line = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), line)
            ins.append(re.sub(r"_Z\w+", "SYM", " ".join(line.split())))
        res[short] = (ins, meta[sym])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--rename", action="append", default=[])
    ap.add_argument("--only", default=None, help="regex on the (renamed) kernel name")
    a = ap.parse_args()
    old, new = kernels(a.parent), kernels(a.this)
    for r in a.rename:
        pat, rep = r.split("=>")
        old = {re.sub(pat, rep, k): v for k, v in old.items()}
    bad = 0
    print("| kernel | instructions parent | this | identical | VGPR | SGPR | scratch |")
    print("|---|---|---|---|---|---|---|")
    for k in sorted(set(old) | set(new)):
        if a.only and not re.search(a.only, k):
            continue
        if k not in old or k not in new:
            print(f"| `{k}` | {'-' if k not in old else len([x for x in old[k][0] if not x.endswith(':')])} | "
                  f"{'-' if k not in new else len([x for x in new[k][0] if not x.endswith(':')])} | unpaired | | | |")
            bad += 1
            continue
        (io, mo), (im, mn) = old[k], new[k]
        same = io == im
        bad += not same
        cnt = lambda ins: len([x for x in ins if not x.endswith(":")])
        col = lambda x, y: str(x) if x == y else f"{x} -> {y}"
        print(f"| `{k}` | {cnt(io)} | {cnt(im)} | {'yes' if same else 'NO'} | {col(mo[0], mn[0])} | {col(mo[1], mn[1])} | {col(mo[2], mn[2])} |")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
