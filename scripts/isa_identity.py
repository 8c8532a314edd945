#!/usr/bin/env python3
"""Do two builds of a .hip file hold the same instructions, kernel by kernel?  (CPU only.)

usage: scripts/isa_identity.py OLD.s NEW.s [--only REGEX]

OLD.s / NEW.s are `hipcc --cuda-device-only -S` outputs of the same file at two revisions (the flags of
scripts/resource_usage.sh).  Each kernel's text runs from its `name:` label to its `.Lfunc_end`; comments
and directives are dropped, and local labels (.LBB<f>_<n>) are renumbered in order of appearance, since a
kernel added or removed elsewhere in the file renumbers <f>.  Prints the kernels only one side has and
the kernels whose instructions differ; exit status 1 if a kernel both sides have differs."""
from __future__ import annotations

import re
import subprocess
import sys


def kernels(path: str) -> dict[str, list[str]]:
    out: dict[str, list[str]] = {}
    name, body = None, []
    for raw in open(path, errors="replace"):
        line = raw.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        m = re.match(r"^(_Z\w+|[A-Za-z_]\w*):\s*$", line)
        if m and name is None and not line.startswith(".L"):
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        s = line.strip()
        if s.startswith(".") and not s.startswith(".LBB"):
            continue   # directives
        body.append(s)
    return out


def normalised(body: list[str]) -> list[str]:
    ids: dict[str, str] = {}

    def sub(m):
        return ids.setdefault(m.group(0), f".L{len(ids)}")
    return [re.sub(r"\.LBB\d+_\d+", sub, s) for s in body]


def demangle(names: list[str]) -> dict[str, str]:
    d = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, d))


def main() -> int:
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    only = None
    if "--only" in sys.argv:
        only = re.compile(sys.argv[sys.argv.index("--only") + 1])
        args = [a for a in args if a != only.pattern]
    old, new = kernels(args[0]), kernels(args[1])
    dm = demangle(sorted(set(old) | set(new)))
    keep = [k for k in sorted(set(old) | set(new)) if only is None or only.search(dm[k])]
    both = [k for k in keep if k in old and k in new]
    differ = [k for k in both if normalised(old[k]) != normalised(new[k])]
    for k in keep:
        if k not in new:
            print("only in OLD:", dm[k])
        elif k not in old:
            print("only in NEW:", dm[k])
    for k in differ:
        print("DIFFERS:", dm[k], f"({len(old[k])} -> {len(new[k])} lines)")
    print(f"{len(both)} kernels in both, {len(both) - len(differ)} identical, {len(differ)} differ; "
          f"{sum(k not in old for k in keep)} new, {sum(k not in new for k in keep)} gone")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
