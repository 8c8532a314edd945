"""The instance pick (csrc/pt_kernel_pick.h), checked without a device by
tests/native/check_kernel_pick.cpp against expectations written out there: the diffuse pools per frame
count (single chunk, multi, ring from 48 frames, never for the env kernel), what the tiled layout and
counted launches exclude, when continuous tiles takes a launch and when the tonemap pass follows; for
v4 the default camera by bits, DEF / DFL / FEXP, every conjunct of the present rule for device jobs and
for the drop-in's calls, and the continuous-tiles threshold at a resident grid of 1536 blocks; for the
batched v4 launches (views, scenes, envs, batch) that every valid (kind, env, layout, fexp) sits at exactly
one of the 44 places of their key list and what is invalid (envs without an env term, the tiled layout, an
unknown env) at none; the grid;
and, over every combination of the facts, that each picked key is in the key lists the instance tables
of pt_kernel.hip and pt_v4.hip are built from (the listed keys that no job reaches are printed).

Which kernel a job really runs sits behind a device: tests/test_gpu_instances.py with the kernel trace
(tests/test_kernel_coverage.py)."""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_kernel_pick_rules(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "check_kernel_pick"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{ROOT / 'cpuperformanceraytracer_amd/csrc'}",
                    str(ROOT / "tests/native/check_kernel_pick.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
