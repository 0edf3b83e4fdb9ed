"""Per-kernel comparison of the gfx950 instruction streams of two builds of one object file.

    python tools/isa_diff.py PARENT.o BRANCH.o [KERNEL_REGEX] [--require-same REGEX]

For every kernel symbol (matching KERNEL_REGEX when given) prints `same` when the two disassemblies agree instruction for
instruction (addresses and encodings stripped), else the instruction count of each side and the counts by class. Exit
status 1 if a kernel matching --require-same differs or exists on one side only. Host only: nothing is run.
"""
from __future__ import annotations

import argparse
import re
import sys

from isa_check import disassemble

CLASSES = (("v_mfma", r"v_mfma"), ("ds_", r"ds_"), ("vmem", r"(global|buffer|flat|scratch)_"),
           ("s_waitcnt", r"s_waitcnt"), ("s_barrier", r"s_barrier"))


def kernels(obj: str) -> dict:
    """{symbol: [instruction text, ...]} of an object's device code."""
    out, cur = {}, None
    for line in disassemble(obj).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(" ".join(line.split("//")[0].split()))
    return out


def classes(ins: list) -> str:
    return " ".join(f"{name}={sum(1 for i in ins if re.match(pat, i))}" for name, pat in CLASSES)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("kernel_re", nargs="?", default=".")
    ap.add_argument("--require-same", metavar="REGEX")
    a = ap.parse_args()
    ka, kb = kernels(a.parent), kernels(a.branch)
    failed = 0
    for k in sorted(set(ka) | set(kb)):
        if not re.search(a.kernel_re, k):
            continue
        x, y = ka.get(k), kb.get(k)
        if x == y:
            print(f"{k}: same ({len(x)} instructions)")
            continue
        for tag, ins in (("parent", x), ("branch", y)):
            print(f"{k}: {tag} " + ("absent" if ins is None else f"{len(ins)} instructions  {classes(ins)}"))
        if a.require_same and re.search(a.require_same, k):
            failed += 1
    if failed:
        print(f"isa_diff: {failed} kernel(s) matching {a.require_same!r} differ", file=sys.stderr)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
