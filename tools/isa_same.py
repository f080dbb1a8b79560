#!/usr/bin/env python3
"""Is the gfx950 device code of two builds the same, function by function?

    tools/isa_same.py BEFORE_DIR AFTER_DIR [--allow-missing REGEX]

Both directories hold the device side of each unit, same relative paths: the Makefile's compile line plus
`--cuda-device-only -c` (and `make HDR_HASH=...` pinned to one value on both sides, so a header-text change is
not mistaken for a code change). Each file is an offload bundle or the bare code object. Per unit, the function
symbols' names and sizes and a hash of each function's disassembly are compared; the order of the functions in the
file is not. Two texts that differ only in position-relative addresses of the same targets (only_moved) count as
the same and are reported apart. Prints "N functions, 0 differ" or the names that differ, are missing or are new,
and exits non-zero on any difference other than functions missing after whose demangled name matches
--allow-missing.
"""
import argparse, bisect, hashlib, os, pathlib, re, shutil, subprocess, sys, tempfile

LLVM = pathlib.Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin"


def run(tool, *args):
    return subprocess.run([str(LLVM / tool), *map(str, args)], capture_output=True, text=True, check=True).stdout


class Unit:
    """The gfx950 code object in `path`: fn[symbol] = (size, sha1 of its disassembly), lines[symbol] =
    [(address, text)], syms = [(address, size, name)] of every defined function and object, by address."""

    def __init__(self, path, tmp):
        elf = path
        if open(path, "rb").read(4) != b"\x7fELF":
            elf = pathlib.Path(tmp) / "unit.elf"
            run("clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                f"--input={path}", f"--output={elf}")
        size, syms = {}, set()
        for line in run("llvm-readelf", "-sW", elf).splitlines():
            f = line.split()
            if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6] != "UND":
                syms.add((int(f[1], 16), int(f[2], 0), f[7]))
                if f[3] == "FUNC":
                    size[f[7]] = int(f[2], 0)
        self.syms, self.lines, cur = sorted(syms), {}, None
        for line in run("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", elf).splitlines():
            m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:$", line)
            if m:
                cur = m.group(1)
            elif cur in size and line.strip():
                text, _, addr = line.partition("//")
                self.lines.setdefault(cur, []).append((int(addr.split(":")[0], 16) if addr.strip() else 0, text.strip()))
        sha = lambda s: hashlib.sha1("\n".join(t for _, t in self.lines.get(s, [])).encode()).hexdigest()
        self.fn = {s: (size[s], sha(s)) for s in size}

    def target(self, addr):
        """(symbol, offset) that holds `addr`, or None."""
        i = bisect.bisect_right(self.syms, (addr, 1 << 62, "")) - 1
        if i < 0 or addr >= self.syms[i][0] + max(self.syms[i][1], 1):
            return None
        return self.syms[i][2], addr - self.syms[i][0]


LITERAL = re.compile(r"\b0x[0-9a-f]+\b")


def only_moved(A, B, s):
    """The two texts of function s differ only in literals that are position-relative addresses of one target: the
    instruction's address plus the literal (mod 2^32) lies at the same offset of the same symbol on both sides.
    (A linked code object holds such offsets to the functions and tables it calls and reads; they all move
    when functions leave the unit.)"""
    la, lb = A.lines[s], B.lines[s]
    if len(la) != len(lb):
        return False
    for (aa, ta), (ab, tb) in zip(la, lb):
        if ta == tb:
            continue
        va, vb = LITERAL.findall(ta), LITERAL.findall(tb)
        if len(va) != 1 or len(vb) != 1 or LITERAL.sub("", ta) != LITERAL.sub("", tb):
            return False
        to_a, to_b = A.target((aa + int(va[0], 16)) & 0xFFFFFFFF), B.target((ab + int(vb[0], 16)) & 0xFFFFFFFF)
        if to_a is None or to_a != to_b:
            return False
    return True


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout
    return dict(zip(names, out.split("\n")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before", type=pathlib.Path)
    ap.add_argument("after", type=pathlib.Path)
    ap.add_argument("--allow-missing", default=None, help="demangled names that may be missing after")
    a = ap.parse_args()
    allow = re.compile(a.allow_missing) if a.allow_missing else None
    units = sorted(p.relative_to(a.before) for p in a.before.rglob("*") if p.suffix in (".o", ".so"))
    units += sorted(p.relative_to(a.after) for p in a.after.rglob("*")
                    if p.suffix in (".o", ".so") and p.relative_to(a.after) not in units)
    bad = 0
    for u in units:
        if not ((a.before / u).exists() and (a.after / u).exists()):
            print(f"{u}: only {'before' if (a.before / u).exists() else 'after'}")
            bad += 1
            continue
        with tempfile.TemporaryDirectory() as tmp:
            UA, UB = Unit(a.before / u, tmp), Unit(a.after / u, tmp)
        A, B = UA.fn, UB.fn
        names = demangle(sorted(set(A) | set(B)))
        moved = [s for s in A if s in B and A[s] != B[s] and A[s][0] == B[s][0] and only_moved(UA, UB, s)]
        differ = [s for s in A if s in B and A[s] != B[s] and s not in moved]
        missing = [s for s in A if s not in B]
        new = [s for s in B if s not in A]
        allowed = [s for s in missing if allow and allow.search(names[s])]
        print(f"{u}: {len(A)} functions, {len(differ)} differ" +
              (f" ({len(moved)} the same but for position-relative addresses)" if moved else "") +
              (f", {len(missing)} only before ({len(allowed)} allowed)" if missing else "") +
              (f", {len(new)} only after" if new else ""))
        for tag, group in (("DIFFERS", differ), ("only before", missing), ("only after", new)):
            for s in group:
                print(f"    {tag}: {names[s]}")
        bad += len(differ) + len(new) + len(missing) - len(allowed)
    print("identical" if not bad else f"{bad} differences")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
