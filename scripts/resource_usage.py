#!/usr/bin/env python3
"""Register / scratch / LDS figures of every kernel of a HIP source, from hipcc's own remarks.

  hipcc -O3 -std=c++17 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage -c X.hip -o /dev/null 2> X.log
  python scripts/resource_usage.py X.log [Y.log ...]             one listing
  python scripts/resource_usage.py --diff A.log B.log            the kernels whose figures differ, or that only one side has

One line per kernel: demangled name, SGPRs, VGPRs, AGPRs, scratch bytes per lane, occupancy, static LDS bytes.  Compile one
source per log (the remarks of parallel compiles interleave)."""
import re
import subprocess
import sys

KEYS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")
HEAD = ("sgpr", "vgpr", "agpr", "scratch", "occ", "lds")


def parse(paths):
    rows, cur = {}, None
    for path in paths:
        for line in open(path):
            m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
            if not m:
                continue
            body = m.group(1).strip()
            if body.startswith("Function Name:"):
                cur = body.split(":", 1)[1].strip()
                rows[cur] = {}
            elif cur is not None and ":" in body:
                k, v = body.rsplit(":", 1)
                if k.strip() in KEYS:
                    rows[cur][k.strip()] = v.strip()
    names = list(rows)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for n, d in zip(names, dem):
        d = re.sub(r"^void ", "", d)
        d = re.sub(r"\((TailArgs|PairBwdArgs|std::conditional<[^<>]*, TailArgsG, TailArgs>::type)\)$", "", d)
        if d.startswith("enf_tail_"):
            if d.startswith("enf_tail_bwd_kernel"):
                d = re.sub(r", false>$", ">", d)      # the backward tail's trailing GRP = false is the default: the name it had before
            d = re.sub(r", 8>$", ">", d)      # the tail's trailing AW = 8 is the default: the name it had before AW existed
        out[d] = tuple(rows[n].get(k, "?") for k in KEYS)
    return out


def fmt(name, fig):
    return "  ".join(f"{h}={v}" for h, v in zip(HEAD, fig)) + "  " + name


def main():
    args = sys.argv[1:]
    if args and args[0] == "--diff":
        a, b = parse([args[1]]), parse([args[2]])
        same = sum(1 for k in a if k in b and a[k] == b[k])
        print(f"# {same} kernels with identical figures; the others:")
        for k in sorted(set(a) | set(b)):
            if a.get(k) != b.get(k):
                print("- " + (fmt(k, a[k]) if k in a else f"(absent)  {k}"))
                print("+ " + (fmt(k, b[k]) if k in b else f"(absent)  {k}"))
        return
    for k, v in sorted(parse(args).items()):
        print(fmt(k, v))


if __name__ == "__main__":
    main()
