#!/usr/bin/env python3
"""Per-kernel comparison of two device assembly listings of one HIP source: which kernels compile to the same instructions.

  hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S X.hip -o new.s       (and the same on the other tree -> old.s)
  python scripts/asm_diff_kernels.py old.s new.s [--drop-trailing ', false']

A kernel's body is the text between its `<symbol>:` label and its `.Lfunc_end` label, comments and directives stripped and the
compiler's local label indices (.LBBn_m) renumbered in order of appearance.  Kernels are matched by demangled name;
--drop-trailing removes a trailing template argument that the new listing's names carry (a flag appended with a default), so that
an instantiation keeps the name it had.  Prints the counts and every kernel that differs or that only one side has; exit status 1 if
a kernel both sides have differs."""
import re
import subprocess
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        s = line.split(";")[0].strip()
        if not s or (s.startswith(".") and not s.startswith(".LBB")):
            continue
        body.append(s)
    return out


def normalise(body):
    ids = {}
    def sub(m):
        return ids.setdefault(m.group(0), f".L{len(ids)}")
    return [re.sub(r"\.LBB\d+_\d+", sub, s) for s in body]


def demangle(names):
    return subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")[:len(names)]


def main():
    args = sys.argv[1:]
    drop = None
    if "--drop-trailing" in args:
        i = args.index("--drop-trailing")
        drop = args[i + 1]
        del args[i:i + 2]
    old, new = kernels(args[0]), kernels(args[1])
    # the template arguments identify a kernel; its parameter list may be spelt anew (a kernel of an unnamed namespace keeps its name)
    strip = lambda d: re.sub(r"\(.*\)$", "", d.replace("(anonymous namespace)::", ""))
    dold = {strip(d): b for d, b in zip(demangle(list(old)), old.values())}
    dnew = {}
    for d, b in zip(demangle(list(new)), new.values()):
        d = strip(d)
        if drop:
            d = re.sub(re.escape(drop) + r">$", ">", d)
        dnew[d] = b
    same = [k for k in dold if k in dnew and normalise(dold[k]) == normalise(dnew[k])]
    diff = [k for k in dold if k in dnew and k not in same]
    print(f"# {len(dold)} kernels before, {len(dnew)} after; {len(same)} with identical instructions, {len(diff)} that differ")
    for k in diff:
        print("DIFFERS  " + k)
    for k in sorted(set(dold) - set(dnew)):
        print("ONLY BEFORE  " + k)
    for k in sorted(set(dnew) - set(dold)):
        print("ONLY AFTER  " + k)
    sys.exit(1 if diff else 0)


if __name__ == "__main__":
    main()
