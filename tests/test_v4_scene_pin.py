"""Pins the v4 oracle's default scene to the reference's own InitializeScene (v4 :1403-1496).

The v4 renderer's images are pinned by tests/test_v4_ref_pin.py (the reference's own lines compiled
with GCC).  Its scene is also literal data in the reference source: this test reads that
source as text and checks every number of the oracle's scene description against it: the quad vertices
with the scene translation (0, 0, 10) of SCENE 1 (v4 :697, :1406-1408) added where the reference
adds it (not to the striped background, :1431-1434), the seven spheres of the loop (:1469-1494) and
every material field.  The oracle description feeds pt_v4_build_scene and the generated literal
header, which tests/test_oracle_v4.py already checks against each other.

The source itself is not part of this repository: the float literals the patterns below pick out of
it are recorded, as written, in tests/golden/v4_scene_literals.json (`python tests/test_v4_scene_pin.py
SOURCE` writes it from a copy of the file), and the tests read that record.
"""
from __future__ import annotations

import json
import re
import sys
from pathlib import Path

import numpy as np

from oracle import pyoracle as po

LITERALS = Path(__file__).resolve().parent / "golden" / "v4_scene_literals.json"

F = r"(-?\d+(?:\.\d*)?|-?\.\d+)f?"   # a float literal as the reference writes it


def _f32(x: str) -> np.float32:
    return np.float32(float(x))


def extract_literals(src_all: str) -> dict:
    """Every literal of InitializeScene the tests compare, as the strings the source holds."""
    start = src_all.index("void InitializeScene()")
    body = src_all[start:src_all.index("void InitializeCamera()", start)]
    assert re.search(r"#define SCENE 1\b", src_all)
    m = re.search(r"scene\.sceneTranslation = set1x3_ps\(" + F + r", " + F + r", " + F + r"\)", src_all)
    out = {"translation": [m.group(k) for k in (1, 2, 3)]}
    pat = re.compile(r"NewQuadObject\.V(\d) = set1x3_ps\(" + F + r", " + F + r", " + F + r"\)(\s*\+\s*scene\.sceneTranslation)?;")
    out["quad_vertices"] = [{"v": int(m.group(1)), "xyz": [m.group(k) for k in (2, 3, 4)], "translated": bool(m.group(5))}
                            for m in pat.finditer(body)]
    out["quad_materials"] = []
    for blk in re.findall(r"QuadSceneObject NewQuadObject\{ 0 \};(.*?)AddMaterialToScene", body, re.S):
        a = re.search(r"^\s*NewMaterial\.albedo = f32x3\{\s*" + F + r",\s*" + F + r",\s*" + F + r"\s*\};", blk, re.M)
        e = re.search(r"^\s*NewMaterial\.emissive = \(f32x3\{\s*" + F + r",\s*" + F + r",\s*" + F + r"\s*\}\s*\*\s*" + F + r"\);",
                      blk, re.M)
        out["quad_materials"].append({"albedo": [a.group(k) for k in (1, 2, 3)] if a else None,
                                      "emissive_times": [e.group(k) for k in (1, 2, 3, 4)] if e else None})
    body = body[body.index("const i32 c_numSpheres"):]   # the sphere loop
    sp = {"count": int(re.search(r"const i32 c_numSpheres = (\d+);", body).group(1))}
    m = re.search(r"set1x4_ps\(" + F + r" \+ " + F + r" \* \(f32\)\(sphereIndex\), " + F + r", " + F + r", " + F + r"\)"
                  r" \+ scene\.sceneTranslation4", body)
    sp["x0_dx_y_z_r"] = [m.group(k) for k in (1, 2, 3, 4, 5)]
    for name in ("specularChance", "IOR", "refractionChance"):
        sp[name] = re.search(r"NewMaterial\." + name + r" = " + F + ";", body).group(1)
    for name in ("albedo", "emissive", "refractionColor"):
        mm = re.search(r"NewMaterial\." + name + r" = f32x3\{ " + F + ", " + F + ", " + F + r" \};", body)
        sp[name] = [mm.group(k) for k in (1, 2, 3)]
    sm = re.search(r"NewMaterial\.specularColor = f32x3\{ " + F + ", " + F + ", " + F + r" \} \*" + F + ";", body)
    sp["specularColor_times"] = [sm.group(k) for k in (1, 2, 3, 4)]
    out["spheres"] = sp
    return out


def _lit() -> dict:
    return json.loads(LITERALS.read_text())["literals"]


def _translation(lit: dict) -> np.ndarray:
    return np.array([_f32(x) for x in lit["translation"]], np.float32)


def test_quads_match_reference_literals():
    lit = _lit()
    t = _translation(lit)
    verts = [(v["v"], np.array([_f32(x) for x in v["xyz"]], np.float32), v["translated"]) for v in lit["quad_vertices"]]
    assert len(verts) == 16 and [v[0] for v in verts] == [0, 1, 2, 3] * 4
    sc = po.default_scene4()
    assert sc.nquads == 4
    got = np.array(sc.quad, np.float32)[:4]
    for i, (_, v, translated) in enumerate(verts):
        want = (v + t).astype(np.float32) if translated else v   # f32 adds, as set1x3_ps + m256x3
        assert np.array_equal(got[i // 4, i % 4], want), (i, got[i // 4, i % 4], want, translated)
    # the striped background (second quad) is the one the reference leaves untranslated
    assert [v[2] for v in verts[4:8]] == [False] * 4 and all(v[2] for v in verts[:4] + verts[8:])


def test_quad_materials_match_reference_literals():
    blocks = _lit()["quad_materials"]
    assert len(blocks) == 4
    sc = po.default_scene4()
    for q, blk in enumerate(blocks):
        mat = sc.mat[q]
        a, e = blk["albedo"], blk["emissive_times"]
        want_alb = [_f32(x) for x in a] if a else [np.float32(0)] * 3
        assert list(np.array(mat.albedo, np.float32)) == want_alb, (q, list(mat.albedo), want_alb)
        want_em = [np.float32(_f32(x) * _f32(e[3])) for x in e[:3]] if e else [np.float32(0)] * 3
        assert list(np.array(mat.emissive, np.float32)) == want_em, (q, list(mat.emissive), want_em)
        for field in ("spec_chance", "spec_rough", "ior", "refr_chance", "refr_rough"):
            assert getattr(mat, field) == 0.0, (q, field)
        assert list(mat.spec_color) == [0.0] * 3 and list(mat.refr_color) == [0.0] * 3


def test_spheres_and_their_materials_match_reference_literals():
    lit = _lit()
    sp = lit["spheres"]
    n = sp["count"]
    x0, dx, y, z, r = (_f32(x) for x in sp["x0_dx_y_z_r"])
    t = _translation(lit)
    sc = po.default_scene4()
    assert sc.nspheres == n == 7
    vec = {name: [_f32(x) for x in sp[name]] for name in ("albedo", "emissive", "refractionColor")}
    sm = sp["specularColor_times"]
    spec_color = [np.float32(_f32(x) * _f32(sm[3])) for x in sm[:3]]
    for i in range(n):
        # (-18 + 6 * i) in f32, then + sceneTranslation4 (w + 0)
        cx = np.float32(x0 + np.float32(dx * np.float32(i)))
        want = np.array([cx + t[0], y + t[1], z + t[2], r], np.float32)
        assert np.array_equal(np.array(sc.sphere[i], np.float32), want), (i, list(sc.sphere[i]), want)
        mat = sc.mat[4 + i]
        rough = np.float32(np.float32(np.float32(i) / np.float32(n - 1)) * np.float32(0.5))   # :1478
        assert mat.spec_chance == _f32(sp["specularChance"]) and mat.ior == _f32(sp["IOR"])
        assert mat.refr_chance == _f32(sp["refractionChance"])
        assert list(np.array(mat.albedo, np.float32)) == vec["albedo"]
        assert list(np.array(mat.emissive, np.float32)) == vec["emissive"]
        assert list(np.array(mat.refr_color, np.float32)) == vec["refractionColor"]
        assert list(np.array(mat.spec_color, np.float32)) == spec_color
        assert np.float32(mat.spec_rough) == rough and np.float32(mat.refr_rough) == rough, (i, mat.spec_rough, rough)


if __name__ == "__main__":   # python tests/test_v4_scene_pin.py SOURCE: record the literals of that file
    LITERALS.write_text(json.dumps({
        "source": "demofox_path_tracing_optimization_v4.cpp, InitializeScene (:1403-1496) and SCENE 1's translation (:697)",
        "literals": extract_literals(Path(sys.argv[1]).read_text(errors="replace"))}, indent=1) + "\n")
