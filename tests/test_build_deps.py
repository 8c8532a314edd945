"""build.py rebuilds the library when any file it is made from changes: every `#include "..."` of a file under
csrc/ that names a file in csrc/ is in the dependency set build_lib compares the library's age with."""
from __future__ import annotations

import re


def test_every_included_csrc_file_is_a_dependency():
    from cpuperformanceraytracer_amd import build
    deps = {build.CSRC / name for name in build.SOURCES + build.HEADERS}
    missing = set()
    for f in sorted(build.CSRC.iterdir()):
        if not f.is_file():
            continue
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read_text(errors="replace"), re.M):
            target = (build.CSRC / inc).resolve()
            if target.is_file() and target.parent == build.CSRC.resolve() and target not in {d.resolve() for d in deps}:
                missing.add(f"{f.name} includes {inc}")
    assert not missing, sorted(missing)
    assert all(d.is_file() for d in deps)
