"""The launch rules (csrc/pt_launch_plan.h), checked without a device by
tests/native/check_launch_plan.cpp against expectations written out there: the split factor and the
default back-claim share per frame count; the schedule step over 601 launches for five rebuild periods
(the first launch records, the second builds, a build always follows a launch that recorded, nothing
else records, the number of builds); the timed arms' order (ABBA / ABCCBA, three rounds, the first
not summed), the arm -> (occupancy, share) table for the diffuse and the env kernel with and without
PT_MI355_BACK -- the table pt_launch_variant reports from; the chained share; and the truth table of
the rule by which a chained launch continues the overlap, with the camera-hit cache's three states at
7 and 8 frames.

How pt_capi.cpp applies the rules sits behind a device: tests/test_gpu_launch_plan.py and
tests/test_gpu_chain.py (the chain counts), tests/test_gpu_regime.py (the arms)."""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_launch_plan_rules(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "check_launch_plan"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{ROOT / 'cpuperformanceraytracer_amd/csrc'}",
                    str(ROOT / "tests/native/check_launch_plan.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
