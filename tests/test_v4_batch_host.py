"""The rules of a batched v4 launch (csrc/pt_v4_batch.h), checked without a device by
tests/native/check_v4_batch.cpp against expectations written out there: the staging block's layout for every
reachable shape (views; scenes; envs with and without scenes; batch with a set, the staged map or no env term,
frames given or not, scenes given or the current scene) at 1 to 1024 views and scenes -- 16-byte offsets, the
documented order, absent sections empty, `need` the end of the last; the fill of a block of exactly `need`
bytes, section by section; and every rejection the five tests/test_abi_v4_*.py files exercise, in their words,
with the calls that break two rules at once, and "nothing to render".

Built twice: plain, and with AddressSanitizer and UBSan, under which a fill that leaves its block fails."""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "cpuperformanceraytracer_amd/csrc"


def _command(exe: Path, extra=()):
    from cpuperformanceraytracer_amd import build
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    try:
        rocm_include = Path(build.hipcc()).resolve().parents[1] / "include"   # (pt_v4.h names hipStream_t)
    except RuntimeError as e:
        pytest.skip(str(e))
    return [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{rocm_include}", f"-I{CSRC}",
            f"-I{ROOT / 'include'}", *extra, str(ROOT / "tests/native/check_v4_batch.cpp"), str(CSRC / "pt_v4_scene.cpp"), "-o", str(exe)]


def test_v4_batch_rules(tmp_path):
    exe = tmp_path / "check_v4_batch"
    subprocess.run(_command(exe), check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def test_v4_batch_rules_sanitized(tmp_path):
    """The same stand-alone program under AddressSanitizer and UBSan: every fill goes into a malloc of exactly `need`
    bytes, so a section that is longer than the layout says ends the run."""
    exe = tmp_path / "check_v4_batch_san"
    built = subprocess.run(_command(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr):
        pytest.skip("this compiler cannot link the sanitizers' runtimes")
    assert built.returncode == 0, built.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
