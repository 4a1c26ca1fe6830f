#!/usr/bin/env python3
"""Compare the kernels of two sets of device-only assembly files (hipcc --cuda-device-only -S), kernel
by kernel: for a change that must leave device code as it is (a file split, a helper moved into a
header).

  tools/kernel_asm_diff.py --old OLD.s [...] --new NEW.s [...] [--show N]

A kernel is matched by its demangled name with anonymous namespaces left out (a parameter type that
moved into a header changes nothing else).  Compared: the .amdhsa_kernel resource block and the
compiler's kernel-info comment (registers, scratch, occupancy, LDS), and the instruction stream from
the kernel's label to its .Lfunc_end with comments dropped and the compiler's local label numbers
(.LBB<n>_<m>, .Ltmp<k>) and the kernel's own mangled name normalised.  Prints one line per kernel and a summary; the exit
status is 1 when a kernel differs, is missing, is new, or appears twice in a set.
"""
import argparse
import difflib
import re
import subprocess
import sys

CXXFILT = "c++filt"


def kernels_of(path):
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[i]))
        tmp = {}
        body = []
        for l in lines[start + 1:end]:
            l = l.split(";")[0].rstrip().replace(name, "<kernel>")
            if not l.strip():
                continue
            l = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", l)
            l = re.sub(r"\.Ltmp\d+", lambda m: tmp.setdefault(m.group(0), ".Ltmp_%d" % len(tmp)), l)
            body.append(l)
        info = [l.strip() for l in lines[end:end + 160]]
        info = info[info.index("; Kernel info:"):] if "; Kernel info:" in info else []
        info = info[:next((i for i, l in enumerate(info) if not l.startswith(";")), len(info))]
        a = next(i for i, l in enumerate(lines) if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(name) + r"$", l))
        b = next(i for i in range(a, len(lines)) if ".end_amdhsa_kernel" in lines[i])
        out[name] = (body, [l.strip() for l in lines[a + 1:b]] + info)
    return out


def demangle(names):
    r = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True)
    return [d.replace("(anonymous namespace)::", "") for d in r.stdout.split("\n")[:len(names)]]


def load(paths):
    ks, dup = {}, []
    for p in paths:
        k = kernels_of(p)
        for name, dem in zip(k, demangle(list(k))):
            if dem in ks:
                dup.append(dem)
            ks[dem] = k[name] + (p,)
    return ks, dup


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--show", type=int, default=12, help="diff lines printed per differing kernel")
    a = ap.parse_args()
    old, dup_old = load(a.old)
    new, dup_new = load(a.new)
    bad = 0
    for dem in sorted(set(old) | set(new)):
        if dem not in new or dem not in old:
            print("%-7s %s" % ("LOST" if dem in old else "NEW", dem))
            bad += 1
            continue
        (b0, r0, _), (b1, r1, p1) = old[dem], new[dem]
        same_b, same_r = b0 == b1, r0 == r1
        print("%-7s %5d instr  %-22s %s" % ("same" if same_b and same_r else "DIFFERS", len(b1), p1.split("/")[-1], dem))
        if not (same_b and same_r):
            bad += 1
            d = list(difflib.unified_diff(r0 + b0, r1 + b1, lineterm="", n=0))
            print("\n".join("    " + l for l in d[:a.show]))
    for d in dup_old + dup_new:
        print("TWICE   " + d)
    print("kernels: old %d, new %d; differing, lost, new or twice: %d" % (len(old), len(new), bad + len(dup_old) + len(dup_new)))
    return 1 if bad or dup_old or dup_new else 0


if __name__ == "__main__":
    sys.exit(main())
