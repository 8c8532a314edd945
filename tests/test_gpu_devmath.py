"""The DEVICE builds of the exact-math headers, run on the GPU and compared bit for bit with their host
builds (tests/native/devmath_probe.hip).

The CPU tests (test_sincosf / test_libmf / test_invtrig / test_envcert) prove the HOST compile of
pt_sincosf.h, pt_libmf.h, pt_invtrig.h and pt_envcert.h equal to glibc 2.35.  The kernels compile
something else: sincosf_glibc's __HIP_DEVICE_COMPILE__ branch, pt_libmf.h's tables indexed at run time,
pt_invtrig.h / pt_envcert.h with div_guarded / sqrt_guarded / rcp_rn / div_rn / sqrt_rn substituted for
'/' and sqrtf, and pt_exactmath.h's guarded forms, whose fallback is the device compiler's own '/'.
The probe runs exactly that code on the GPU; the reference is always the host side (the headers'
default compile; x86 hardware '/' and sqrt for division, reciprocal and square root).  Sets and their
sizes are listed in MINIMUM below; every one is exhaustive or a fixed generated list, nothing is thinned.

Measured on an MI355X with 16 host threads (profiles/r06/r06zq_devmath_probe.txt), wall time of one
probe process per section: sincos 1.5 s, exp 1.2 s, pow 0.6 s, invtrig 2.7 s, guarded 1.7 s,
envcert 3.7 s; the contracted build's invtrig 2.8 s (5.4 s with its compile).  TIMEOUT is 60 s, more
than fifteen times the slowest: it ends a hang, it does not police speed.

What the first run found (profiles/r06/r06zq_devmath_probe_first_run.txt; fixed in pt_exactmath.h, the
inputs kept in the probe's lists; cost of the fix: profiles/r06/r06zq_guard_fix_isa.txt and
r06zq_bench_ab.txt):
  * sqrt_guarded(+inf) returned NaN (rsq(inf) = 0, inf * 0): the guard now also sends +inf to sqrtf;
    pt_kernel.hip, whose radicands are all finite, calls the earlier one-compare form under the name
    sqrt_finite_guarded (checked here on every finite x >= 0, a negative sample and NaN);
  * div_guarded(a, b) was one ulp off for part of the operands with |a| < 2^-102 and a normal
    quotient (div_rn's remainders underflow): 4325 of the 1.13 M boundary pairs, and through it
    atan2f_glibc on at least 6347 of the 2^25 random pairs (those with raw bit patterns), 292 of the
    exponent-difference pairs and 161 of the window pairs.  The guard now requires |a| >= 2^-100.

Sensitivity: the same probe built with -ffp-contract=fast reports, in section invtrig, at least
17 967 asinf, 4 274 atanf and 10 973 atan2f (random pairs) mismatches (lower bounds: 1024 differing
blocks are examined item by item, each further one counts once) -- the probe can fail.  The other three
atan2f sets (special, expdiff, window) report none under contraction, and that is expected: their
operands are zeros, infinities, NaN or far apart in exponent, so atan2f_glibc returns from its special
cases or from a quotient that is tiny or huge, and the fused a * b + c of its polynomial is not what
decides the result."""
from __future__ import annotations

import re
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from cpuperformanceraytracer_amd.build import ARCH, PARITY_FLAGS, hipcc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests/native/devmath_probe.hip"
TIMEOUT = 60


def _bits(x) -> int:
    return struct.unpack("<I", struct.pack("<f", float(np.float32(x))))[0]


_TWO_PI_HI = np.float32(6.2831855) * np.float32(1.0001)
_SPECIAL = (2 * 16 + 1) ** 2        # +-16 special operands and NaN, crossed
# the least each set must have checked, from its definition
MINIMUM = {
    "sincos": {
        "sincos.0_2pi": _bits(_TWO_PI_HI) + 1,                      # every f32 in [0, 2 pi 1.0001]
        "sincos.negative": _bits(-6.2832) - _bits(-1e-45) + 1,      # every f32 in [-6.2832, -1e-45]
    },
    "exp": {"exp.all": 1 << 32},
    "pow": {
        "pow.gamma": 0x3f800000 - 0x3b000000 + 1,                   # every f32 in [2^-9, 1]
        # the candidates of the fixed generator that pass |y log2 x| < 126: 16 827 254 of 2^25 with glibc's
        # log2; another libm could move only a candidate whose product is within an ulp of 126
        "pow.random": 16_827_000,
    },
    "invtrig": {
        "invtrig.asin": 2 * (0x3f800000 + 1) + 1,                   # |x| <= 1, and a sample above
        "invtrig.atan": 1 << 31,
        "invtrig.atan2.random": 1 << 25,
        "invtrig.atan2.special": _SPECIAL,
        "invtrig.atan2.expdiff": 1 << 20,
        "invtrig.atan2.window": 1 << 20,
    },
    "guarded": {
        "guarded.sqrt": (1 << 31) + 3,                              # x >= 0 and NaN; -0, a negative sample
        "guarded.sqrt_finite": 0x7f800000 + (1 << 16) + 3,          # finite x >= 0; the negative sample; NaNs
        "guarded.div_one_over_x": 1 << 32,
        "guarded.div.class0": 1 << 28,
        "guarded.div.class1": 1 << 28,
        "guarded.div.class2": 1 << 28,
        # 20 b x (20 a + 4129) + 20 a x 4129 operand-boundary pairs, 2^17 small-a pairs, and 7 a per b for
        # the (target, b) of 4 x 2^16 whose a = T b is finite and non-zero: a fixed list (integer generator,
        # no libm) of exactly this many pairs
        "guarded.div.boundary": 1_302_967,
        "guarded.div.special": _SPECIAL,
        "guarded.rcp": 1 << 32,
        "guarded.rcp_nonneg": 0x7e000000 + 1 + 1,                   # [0, 2^125] and NaN
    },
    # 2^23 generated directions, less the few dropped as too short (dd <= 1e-6: about 1e-5 of them), and
    # 10 368 out-of-domain ones
    "envcert": {f"envcert.{k}.{s}": 1 << 23 for k in ("random", "nearest") for s in ("2048x1024", "3x5", "1x1")},
}


def _build(exe: Path, contract: str) -> Path:
    flags = [f"-ffp-contract={contract}" if f.startswith("-ffp-contract=") else f for f in PARITY_FLAGS]
    assert flags != PARITY_FLAGS or contract == "off"
    subprocess.run([hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", *flags, str(SRC), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("devmath") / "devmath_probe", "off")


def _lines(stdout: str) -> dict[str, tuple[int, int]]:
    return {m.group(1): (int(m.group(2)), int(m.group(3)))
            for m in re.finditer(r"^(\S+) checked=(\d+) mismatches=(\d+)$", stdout, re.M)}


@pytest.mark.parametrize("section", list(MINIMUM))
def test_device_build_matches_host(probe, section):
    out = subprocess.run([str(probe), section], capture_output=True, text=True, timeout=TIMEOUT)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    got = _lines(out.stdout)
    assert set(got) == set(MINIMUM[section]), out.stdout
    for name, least in MINIMUM[section].items():
        checked, mismatches = got[name]
        assert mismatches == 0, out.stdout
        assert checked >= least, (name, checked, least)


def test_probe_notices_contraction(tmp_path):
    """The probe can fail: with -ffp-contract=fast in place of =off (the other parity flags unchanged)
    the device fuses pt_invtrig.h's a * b + c, the host (no FMA in the x86-64 baseline) does not."""
    exe = _build(tmp_path / "devmath_probe_contract", "fast")
    out = subprocess.run([str(exe), "invtrig"], capture_output=True, text=True, timeout=TIMEOUT)
    print(out.stdout)
    assert out.returncode == 1, out.stdout + out.stderr
    got = _lines(out.stdout)
    assert set(got) == set(MINIMUM["invtrig"]), out.stdout
    for name in ("invtrig.asin", "invtrig.atan", "invtrig.atan2.random"):
        assert got[name][1] > 0, out.stdout
