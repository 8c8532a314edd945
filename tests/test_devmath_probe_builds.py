"""tests/native/devmath_probe.hip cross-compiles for gfx950 with the product's parity flags.  The probe
includes every exact-math header twice (device pass with the kernels' macro substitutions, host pass
with the defaults), so a header change that breaks it shows here, without a GPU; what it checks when it
runs is in tests/test_gpu_devmath.py."""
from __future__ import annotations

import subprocess
from pathlib import Path

import pytest

from cpuperformanceraytracer_amd.build import ARCH, PARITY_FLAGS, hipcc

ROOT = Path(__file__).resolve().parents[1]


def test_devmath_probe_builds(tmp_path):
    try:
        cc = hipcc()
    except RuntimeError:
        pytest.skip("no hipcc")
    out = subprocess.run([cc, f"--offload-arch={ARCH}", "-O3", "-std=c++17", *PARITY_FLAGS,
                          str(ROOT / "tests/native/devmath_probe.hip"), "-o", str(tmp_path / "devmath_probe")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
