#!/usr/bin/env python3
"""Compare two compiler resource reports (hipcc -Rpass-analysis=kernel-resource-usage, stderr saved to a file):
per kernel the VGPRs, AGPRs, SGPRs, scratch, occupancy and LDS, and the kernels whose figures differ.

    tools/kres_diff.py before.txt after.txt [--show REGEX]

--show lists the figures of the kernels whose demangled name matches, changed or not.
"""
import argparse
import collections
import re
import shutil
import subprocess


def parse(path):
    out, cur = collections.OrderedDict(), None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out.setdefault(cur, collections.OrderedDict())
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?)\s*:\s*(\S+)\s*(\[-R|$)", line)
        if m and cur:
            out[cur][m.group(1).strip()] = m.group(2)
    return out


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool:
        return {n: n for n in names}
    r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--show", default=None)
    a = ap.parse_args()
    A, B = parse(a.before), parse(a.after)
    names = demangle(list(A))
    print(f"kernels: {len(A)} before, {len(B)} after")
    changed = 0
    for k, fa in A.items():
        fb = B.get(k)
        if fb is None:
            print(f"only before: {names[k]}")
            continue
        if fa != fb:
            changed += 1
            print(f"CHANGED {names[k]}")
            for f in fa:
                if fa[f] != fb.get(f):
                    print(f"    {f}: {fa[f]} -> {fb.get(f)}")
    for k in B:
        if k not in A:
            print(f"only after: {k}")
    print(f"{changed} of {len(A)} kernels differ")
    if a.show:
        rx = re.compile(a.show)
        for k, fa in A.items():
            if rx.search(names[k]) and k in B:
                same = "same" if fa == B[k] else "differs"
                print(f"{names[k]}\n    {same}: " + ", ".join(f"{f} {v}" for f, v in B[k].items()))


if __name__ == "__main__":
    main()
