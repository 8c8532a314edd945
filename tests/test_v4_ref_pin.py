"""The v4 oracle (oracle/pt_oracle_v4.c, pt_oracle_output.c) pinned to the reference's own v4 code.

tests/golden/v4_ref_*.npz are runs of demofox_path_tracing_optimization_v4.cpp :1-1556 itself, compiled
with GCC behind oracle/ref_v4_shim.h (oracle/build_ref.sh, tests/golden/make_golden_v4.py): RenderTile,
mainImage, GetColorForRay, the texture samplers, InitializeScene / Add*ToScene / PrecomputeQuadData,
OutputToScreen -- under the shipped flags and every flag variant the product exposes.  Bar: BIT-EXACT,
whole images.  What stays unpinned is what the shim substitutes (rcp, rsqrt, the SVML calls -> 1/x,
1/sqrtf, glibc) and MSVC-versus-GCC code generation.

  - from the committed fixtures, always: po.render4 (camera A: the camera oracle of
    v4_camera_oracle.py) == every accumulator, po.tonemap == every pixel fixture, the frame counter;
  - live, when oracle/_ref/ref_v4_* exist: two further sizes (8 x 8 in one tile, 128 x 72 in
    32 x 24 tiles) with other env seeds, so the oracle cannot be fitted to the committed images;
  - the manifest's recorded flag diffs change only the named lines.
"""
from __future__ import annotations

import hashlib
import re

import numpy as np
import pytest

import v4_ref as vr
from conftest import bits_equal, mismatch_report

SCENE = (vr.SCENE_QUADS, vr.SCENE_SPHERES, vr.SCENE_MATS)


def _same_bits(got, want):
    assert bits_equal(got, want), mismatch_report(got, want)


def _fixture_scene(fx):
    return (fx["quads"], fx["spheres"], fx["mats"]) if "quads" in fx else None


@pytest.mark.parametrize("name", list(vr.CASES))
def test_oracle_equals_reference_fixture(name, manifest):
    c = vr.CASES[name]
    fx = vr.load(name)
    m = manifest["v4_ref"]["cases"][name]
    assert hashlib.sha256(fx["acc"].tobytes()).hexdigest() == m["sha256_acc"]
    assert {k: m[k] for k in c} == c, "the fixture was generated for another case"
    if c["cam"]:
        assert tuple(fx["cam"].tolist()) == tuple(np.float32(vr.camera_args(c["cam"])).tolist())
    kind = vr.VARIANTS[c["variant"]][0]
    ref = vr.interleaved(fx["acc"])
    assert np.isfinite(ref).all() and len(np.unique(ref.reshape(-1, 3), axis=0)) > 100   # a traced image
    got = vr.oracle_render(c["variant"], frames=c["frames"], frame0=c["frame0"], env=vr.load_env(kind),
                           scene=_fixture_scene(fx), cam=c["cam"])
    _same_bits(got, ref)
    # iFrame (a static f32, += 1.0f per call) after the run: exact in f32 up to 2^24
    assert fx["iframe"].dtype == np.float32 and float(fx["iframe"][0]) == c["frame0"] + c["frames"]
    if c["screen"]:
        assert np.array_equal(vr.oracle_screen(c["variant"], ref), fx["screen"])
    else:
        assert fx["screen"] is None


def test_edited_scene_covers_what_it_is_for():
    """The edited scene's second quad is neither a parallelogram nor planar, and from both cameras
    every object -- that quad through its top triangle alone, the small sphere, the refractive
    sphere -- is hit by camera rays of the 64 x 48 image (so PrecomputeQuadData's DetTop, v4 :294-297,
    decides pixels of the fixtures)."""
    import ctypes
    import v4_camera_oracle as vo
    V = vr.SCENE_QUADS[1].astype(np.float64)
    assert np.abs(V[3] - (V[0] + V[2] - V[1])).max() > 1.0                        # no parallelogram
    n = np.cross(V[1] - V[0], V[2] - V[0])
    assert abs(np.dot(V[3] - V[0], n / np.linalg.norm(n))) > 0.5                   # not planar
    # DetTop as the reference computes it, dot(cross(V30, V01), N), against the top triangle's own
    # determinant dot(cross(V02, V03), N): far apart here (for a parallelogram they are equal)
    N = n / np.linalg.norm(n)
    det_top = np.dot(np.cross(V[0] - V[3], V[1] - V[0]), N)
    det_own = np.dot(np.cross(V[2] - V[0], V[3] - V[0]), N)
    assert abs(det_top / det_own - 1.0) > 0.25
    L = vo.load()
    scene = vr.oracle_scene()
    bottom_only = vr.oracle_scene(quads=np.stack([vr.SCENE_QUADS[0], vr.SCENE_QUADS[1][[0, 1, 2, 0]]]))
    f3 = ctypes.c_float * 3
    for pos, dist in (((0.0, 0.0, 40.0), 1.0), (vr.camera_args("A")[:3], vr.camera_args("A")[3])):
        hits, top = set(), 0
        for Y in range(vr.H):
            for X in range(vr.W):
                d = np.array([2 * X / vr.W - 1, (2 * (vr.H - 1 - Y) / vr.H - 1) * vr.H / vr.W, -dist])
                d = (d / np.linalg.norm(d)).astype(np.float32)
                mat, mat2 = ctypes.c_int(-1), ctypes.c_int(-1)
                L.pto4_trace_scene(ctypes.byref(scene), f3(*pos), f3(*d), ctypes.byref(mat))
                L.pto4_trace_scene(ctypes.byref(bottom_only), f3(*pos), f3(*d), ctypes.byref(mat2))
                hits.add(mat.value)
                top += mat.value == 1 and mat2.value != 1
        assert {0, 1, 2, 3} <= hits, hits
        assert top >= 20, top


def test_manifest_flag_diffs_change_only_the_named_lines(manifest):
    f = manifest["v4_ref"]["flags"]
    assert f["v4_lines"] == "1-1556" and re.fullmatch(r"[0-9a-f]{64}", f["v4_sha256"])
    assert set(f["variants"]) == set(vr.VARIANTS)
    named = {"shipped": {}, "cubemap": {57: "USE_ENV_CUBEMAP 1"}, "bilinear": {66: "USE_RANDOM_JITTER_TEXTURE_SAMPLING 0"},
             "angle": {65: "USE_UNIT_VECTOR_REJECTION_SAMPLING 0"}, "noenv": {56: "USE_ENV_MAP 0"},
             "exactexp": {64: "USE_FAST_APPROXIMATE_EXP 0"},
             "exactout": {62: "USE_FAST_APPROXIMATE_GAMMA 0", 63: "USE_FAST_APPROXIMATE_ACES_TONEMAP 0"},
             "noaccum": {60: "ACCUMULATE_FRAMES 0"}}
    for name, v in f["variants"].items():
        want = named[name]
        assert {int(k): s for k, s in v["lines"].items()} == {k: "#define " + s for k, s in want.items()}
        assert (v["sha256_patched"] == f["sha256_original"]) == (not want)
        # `diff` output: per changed line "NcN", "< old", "---", "> new"; nothing else
        removed, added, where = [], [], []
        for line in v["diff"].splitlines():
            if line.startswith("< "):
                removed.append(line[2:])
            elif line.startswith("> "):
                added.append(line[2:])
            elif line != "---":
                m = re.fullmatch(r"(\d+)(?:,(\d+))?c(\d+)(?:,(\d+))?", line)
                assert m and m.group(1) == m.group(3) and m.group(2) == m.group(4), line
                where += list(range(int(m.group(1)), int(m.group(2) or m.group(1)) + 1))
        assert where == sorted(want)
        assert added == ["#define " + want[k] for k in sorted(want)]
        # each removed line is the same switch with the other value
        assert removed == ["#define " + want[k][:-1] + str(1 - int(want[k][-1])) for k in sorted(want)]


# ---- live: the binaries of this checkout's oracle/_ref/ ------------------------------------------------
live = pytest.mark.skipif(not vr.ref_available(), reason="oracle/_ref/ref_v4_* not built (no reference here)")

LIVE_SIZES = [(8, 8, 8, 8), (128, 72, 32, 24)]


def _live_env(kind):
    return vr.synth_env(kind, seed_equirect=77, seed_cubemap=78)


@live
@pytest.mark.parametrize("size", LIVE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("variant", list(vr.VARIANTS))
def test_live_variants(variant, size):
    w, h, tw, th = size
    kind = vr.VARIANTS[variant][0]
    env = _live_env(kind)
    r = vr.run_ref(variant, w=w, h=h, tw=tw, th=th, frames=3, env=env, screen=True)
    ref = vr.interleaved(r["acc"], w, h, tw, th)
    _same_bits(vr.oracle_render(variant, w=w, h=h, frames=3, env=env), ref)
    assert float(r["iframe"][0]) == 3.0
    assert np.array_equal(vr.oracle_screen(variant, ref), r["screen"])


@live
@pytest.mark.parametrize("size", LIVE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cam", [None, "A"])
def test_live_edited_scene(cam, size):
    w, h, tw, th = size
    env = _live_env("equirect")
    r = vr.run_ref("shipped", w=w, h=h, tw=tw, th=th, frames=2, frame0=40, env=env, scene=SCENE,
                   cam=vr.camera_args(cam) if cam else None)
    _same_bits(vr.oracle_render("shipped", w=w, h=h, frames=2, frame0=40, env=env, scene=SCENE, cam=cam),
               vr.interleaved(r["acc"], w, h, tw, th))
    assert float(r["iframe"][0]) == 42.0
