#!/usr/bin/env python3
"""Wave D's drain in the assembly of k_bwd_quad (csrc/tog_bwd_quad.hpp): the instructions between its last tag poll
(the wait for tmp1's last row) and its flg[2] store, the last thing it does before the path to the B2b s_barrier.

    tools/quad_drain_isa.py UNIT.s [KERNEL_REGEX]

UNIT.s: the Makefile's compile line of a model unit plus `--cuda-device-only -S`. For every kernel whose mangled name
matches (default: every k_bwd_quad instance) prints the instruction count of that range, the out-of-line blocks it
branches to included, and the exec-mask branches (s_cbranch_exec*), v_accvgpr moves and v_cmp_class_f64 (tog_rsqrt's
class test) in it.
"""
import re
import sys

LABEL = re.compile(r"^(\.LBB\d+_\d+):")
INSTR = re.compile(r"^\t([a-z]\w+)\b(.*)")


def functions(path, rx):
    name, body = None, []
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+):", line)
        if m and rx.search(m.group(1)):
            name, body = m.group(1), []
        elif name and line.startswith(".Lfunc_end"):
            yield name, body
            name = None
        elif name:
            body.append(line.rstrip("\n"))


def polls(body):
    """Indices of the back branches of the tag polls: ds_read_b32, s_waitcnt, v_cmp_ne_u32, s_cbranch_vccnz to the
    label right above."""
    out = []
    for i, line in enumerate(body):
        m = re.match(r"^\ts_cbranch_vccnz (\.LBB\d+_\d+)", line)
        if m and i >= 3 and "ds_read_b32" in body[i - 3] and any(
                LABEL.match(body[j]) and LABEL.match(body[j]).group(1) == m.group(1) for j in range(max(0, i - 8), i - 3)):
            out.append(i)
    return out


def count(body, lo, hi):
    """Instructions in body[lo:hi] plus the out-of-line blocks branched to from there (each up to its s_branch)."""
    labels = {LABEL.match(l).group(1): i for i, l in enumerate(body) if LABEL.match(l)}
    ops, side = [], []
    for i in range(lo, hi):
        m = INSTR.match(body[i])
        if not m:
            continue
        ops.append(m.group(1))
        t = re.search(r"(\.LBB\d+_\d+)", m.group(2))
        if t and m.group(1).startswith("s_cbranch_exec") and t.group(1) in labels:
            j = labels[t.group(1)]
            if not (lo <= j < hi) and j not in side:
                side.append(j)
    for j in side:  # a block placed out of line: it ends with the s_branch back into the range
        e = next((k for k in range(j, len(body)) if re.match(r"^\ts_branch ", body[k])), None)
        back = e is not None and lo <= labels.get(body[e].split()[-1], -1) < hi
        if back:
            ops += [INSTR.match(l).group(1) for l in body[j:e + 1] if INSTR.match(l)]
    return ops


def main():
    rx = re.compile(sys.argv[2] if len(sys.argv) > 2 else "k_bwd_quad")
    for name, body in functions(sys.argv[1], rx):
        shr = [i for i, l in enumerate(body) if "row_shr:1" in l]
        if not shr:
            continue
        before = [p for p in polls(body) if p < shr[-1]]
        if not before:
            continue
        lo = before[-1] + 1
        flag = re.compile(r"^\tds_write_b32 .*offset:(\d+)")
        # flg[2]: the first 32-bit LDS store behind the last systolic shift
        hi = next(i for i in range(shr[-1], len(body)) if flag.match(body[i])) + 1
        ops = count(body, lo, hi)
        print(name)
        print(f"  wave D, last tag poll -> flg[2] store: {len(ops)} instructions, "
              f"{sum(o.startswith('s_cbranch_exec') for o in ops)} s_cbranch_exec*, "
              f"{sum(o.startswith('v_accvgpr') for o in ops)} v_accvgpr moves, "
              f"{sum(o.startswith('v_cmp_class_f64') for o in ops)} v_cmp_class_f64")


if __name__ == "__main__":
    main()
