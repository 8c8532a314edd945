"""The v4 oracle with a settable camera -- test helper (a plain module, like layouts.py).

oracle/pt_oracle_v4.c carries the reference's camera as two literals, each exactly once: the distance
`1.0f / tanf(90.0f * 0.5f * V4_PI / 180.0f)` (InitializeCamera v4 :1500) and the position
`mk(0.0f, 0.0f, 1.0f * 40.0f)` (:1501).  The oracle's sources stay as they are; this module compiles a
copy in which the two expressions read the exported globals pto4_cam_dist / pto4_cam_pos[3] (the way
oracle/build_ref.sh handles its c_numBounces copy), with oracle/Makefile's CFLAGS, into a temporary
directory, and drives it with pyoracle's Params4 / Scene4 / Counts4.  The distance is computed here in
f32 with the reference's own expression and glibc's tanf.
"""
from __future__ import annotations

import atexit
import ctypes
import ctypes.util
import os
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np

from oracle import pyoracle as po

ORACLE = Path(__file__).resolve().parents[1] / "oracle"
DIST_EXPR = "1.0f / tanf(90.0f * 0.5f * V4_PI / 180.0f)"
POS_EXPR = "mk(0.0f, 0.0f, 1.0f * 40.0f)"
V4_PI = np.float32(3.14159265359)   # c_pi (mathutils.h:5), oracle/pt_oracle_v4.c V4_PI

# the issue's camera settings: (position, fov_degrees)
DEFAULT = ((0.0, 0.0, 40.0), 90.0)
CAMERAS = {"A": ((3.0, -2.0, 30.0), 60.0), "B": ((-6.5, 4.25, 55.0), 90.0), "C": ((0.0, -6.0, 22.0), 75.0),
           "D": ((0.0, 0.0, 8.0), 90.0)}

_lib = None


def _cflags() -> list[str]:
    m = re.search(r"^CFLAGS\s*=\s*(.*)$", (ORACLE / "Makefile").read_text(), re.M)
    assert m, "oracle/Makefile has no CFLAGS line"
    return m.group(1).split()


def patched_source() -> str:
    src = (ORACLE / "pt_oracle_v4.c").read_text()
    assert src.count(DIST_EXPR) == 1, f"the camera distance expression occurs {src.count(DIST_EXPR)} times"
    assert src.count(POS_EXPR) == 1, f"the camera position expression occurs {src.count(POS_EXPR)} times"
    src = src.replace(DIST_EXPR, "pto4_cam_dist")
    src = src.replace(POS_EXPR, "mk(pto4_cam_pos[0], pto4_cam_pos[1], pto4_cam_pos[2])")
    assert src.count("pto4_cam_dist") == 1 and src.count("mk(pto4_cam_pos[0]") == 1
    decl = "float pto4_cam_dist = 1.0f;\nfloat pto4_cam_pos[3] = {0.0f, 0.0f, 40.0f};\n"
    k = src.index("static inline v3 mk(")   # file scope, before the first use
    return src[:k] + decl + src[k:]


def load() -> ctypes.CDLL:
    """The patched oracle (built once per process)."""
    global _lib
    if _lib is None:
        tmp = Path(tempfile.mkdtemp(prefix="pto4cam_"))
        atexit.register(shutil.rmtree, tmp, True)
        (tmp / "pt_oracle_v4_cam.c").write_text(patched_source())
        out = tmp / "liboracle_cam.so"
        subprocess.run([os.environ.get("CC", "gcc"), *_cflags(), f"-I{ORACLE}", "-shared", "-o", str(out),
                        str(ORACLE / "pt_oracle.c"), str(ORACLE / "pt_oracle_output.c"), str(tmp / "pt_oracle_v4_cam.c"),
                        "-lm", "-lpthread"], check=True)
        L = ctypes.CDLL(str(out))
        L.pto4_render.argtypes = [ctypes.c_void_p, ctypes.POINTER(po.Params4), ctypes.POINTER(po.Scene4),
                                  ctypes.POINTER(po.Counts4)]
        L.pto4_render.restype = ctypes.c_int
        f3 = ctypes.c_float * 3
        L.pto4_trace_scene.argtypes = [ctypes.POINTER(po.Scene4), f3, f3, ctypes.POINTER(ctypes.c_int)]
        L.pto4_trace_scene.restype = ctypes.c_float
        _lib = L
    return _lib


def lib_path() -> str:
    """The patched oracle's shared library (for native checkers that link it)."""
    return load()._name


def tanf(x) -> np.float32:
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.tanf.argtypes, m.tanf.restype = [ctypes.c_float], ctypes.c_float
    return np.float32(m.tanf(float(np.float32(x))))


def distance(fov_degrees: float) -> np.float32:
    """camera.Distance: 1.0f / tanf(fov * 0.5f * c_pi / 180.0f), every step in f32."""
    a = np.float32(fov_degrees) * np.float32(0.5) * V4_PI / np.float32(180.0)
    assert a.dtype == np.float32
    return np.float32(1.0) / tanf(a)


def set_camera(position=DEFAULT[0], fov_degrees: float = DEFAULT[1]) -> None:
    L = load()
    ctypes.c_float.in_dll(L, "pto4_cam_dist").value = float(distance(fov_degrees))
    pos = (ctypes.c_float * 3).in_dll(L, "pto4_cam_pos")
    for k in range(3):
        pos[k] = float(np.float32(position[k]))


def render4(width: int, height: int, *, camera=DEFAULT, frame_first: int = 1, nframes: int = 1, num_bounces: int = 8,
            row_start: int = 0, row_stride: int = 1, nrows: int | None = None, env_mode: int = po.ENV_EQUIRECT,
            env: np.ndarray | None = None, random_jitter: bool = True, rejection: bool = True,
            scene: po.Scene4 | None = None, buf: np.ndarray | None = None, counts: bool = False):
    """pyoracle.render4 seen by `camera` = (position, fov_degrees)."""
    set_camera(*camera)
    nrows = height if nrows is None else nrows
    if buf is None:
        buf = np.zeros((nrows, width, 3), np.float32)
    assert buf.dtype == np.float32 and buf.flags["C_CONTIGUOUS"] and buf.size >= nrows * width * 3
    p = po.Params4(width, height, row_start, row_stride, nrows, frame_first, nframes, num_bounces,
                   env_mode if env is not None else po.ENV_NONE, int(random_jitter), int(rejection), None,
                   min(os.cpu_count() or 1, 16), 0, 0)
    keep = None
    if env is not None:
        env = np.ascontiguousarray(env, dtype=np.float32)
        keep = (env, po.Env(env.ctypes.data, env.shape[1], env.shape[0]))
        p.env = ctypes.pointer(keep[1])
    c = po.Counts4()
    rc = load().pto4_render(buf.ctypes.data, ctypes.byref(p), ctypes.byref(scene) if scene is not None else None,
                            ctypes.byref(c) if counts else None)
    del keep
    if rc:
        raise ValueError("pto4_render rejected the parameters")
    if counts:
        return buf, {k: int(getattr(c, k)) for k, _ in po.Counts4._fields_}
    return buf


# ---- the test scene: Add*ToScene objects in front of cameras A-C (z <= 16, the nearest camera at 22) ----
# (vertices | centre and radius, material in AddMaterialToScene's argument order; quads first)
QUADS = [np.array([[-10, -8, 2], [10, -8, 2], [10, -8, 16], [-10, -8, 16]], np.float32),     # diffuse floor
         np.array([[-4, 6, 6], [4, 6, 6], [4, 6, 12], [-4, 6, 12]], np.float32)]             # emissive quad
SPHERES = [np.array([-4, -5, 9, 3], np.float32),                                              # diffuse sphere
           np.array([5, -4.5, 11, 3.5], np.float32)]                                          # glass sphere
_Z3 = (0.0, 0.0, 0.0)
MATS = [dict(albedo=(0.7, 0.65, 0.6), emissive=_Z3, spec_chance=0.0, spec_rough=0.0, spec_color=_Z3, ior=1.0,
             refr_chance=0.0, refr_rough=0.0, refr_color=_Z3),
        dict(albedo=_Z3, emissive=(14.0, 12.0, 9.0), spec_chance=0.0, spec_rough=0.0, spec_color=_Z3, ior=1.0,
             refr_chance=0.0, refr_rough=0.0, refr_color=_Z3),
        dict(albedo=(0.3, 0.6, 0.8), emissive=_Z3, spec_chance=0.0, spec_rough=0.0, spec_color=_Z3, ior=1.0,
             refr_chance=0.0, refr_rough=0.0, refr_color=_Z3),
        dict(albedo=(0.9, 0.9, 0.9), emissive=_Z3, spec_chance=0.04, spec_rough=0.05, spec_color=(0.9, 0.9, 0.9), ior=1.5,
             refr_chance=0.9, refr_rough=0.0, refr_color=(0.05, 0.1, 0.02))]


def oracle_scene(quads=QUADS, spheres=SPHERES, mats=MATS) -> po.Scene4:
    s = po.Scene4()
    s.nquads, s.nspheres, s.nmat = len(quads), len(spheres), len(mats)
    for i, q in enumerate(quads):
        for k in range(4):
            for j in range(3):
                s.quad[i][k][j] = float(q[k, j])
    for i, p in enumerate(spheres):
        for j in range(4):
            s.sphere[i][j] = float(p[j])
    for i, m in enumerate(mats):
        M = s.mat[i]
        for k in range(3):
            M.albedo[k], M.emissive[k] = float(m["albedo"][k]), float(m["emissive"][k])
            M.spec_color[k], M.refr_color[k] = float(m["spec_color"][k]), float(m["refr_color"][k])
        M.spec_chance, M.spec_rough, M.ior = m["spec_chance"], m["spec_rough"], m["ior"]
        M.refr_chance, M.refr_rough = m["refr_chance"], m["refr_rough"]
    return s


def edit_scene(pt, quads=QUADS, spheres=SPHERES, mats=MATS) -> None:
    """The same scene through the product's ClearScene / Add*ToScene."""
    pt.ClearScene()
    for m in mats:
        pt.AddMaterialToScene(m["albedo"], m["emissive"], m["spec_chance"], m["spec_rough"], m["spec_color"],
                              m["ior"], m["refr_chance"], m["refr_rough"], m["refr_color"])
    for q in quads:
        pt.AddQuadObjectToScene(q)
    for p in spheres:
        pt.AddSphereObjectToScene(p)


def sky_tiles(rects: np.ndarray, width: int, height: int, position, fov_degrees: float) -> list[tuple[int, int]]:
    """The 8 x 8 pixel tiles (tx, ty) of a width x height image whose every camera ray, under the
    +-0.5 px jitter, lies outside every rectangle of the window (mainImage's slopes, v4 :1092-1113:
    sx = tx / Distance with tx = 2 (X + jx) / W - 1, sy = ty / Distance with ty = (2 (H - 1 - Y + jy) / H - 1) H / W)."""
    d = float(distance(fov_degrees))
    out = []
    for ty in range(0, height, 8):
        for tx in range(0, width, 8):
            x0, x1 = tx - 0.5, min(tx + 7, width - 1) + 0.5
            f0, f1 = height - 1 - min(ty + 7, height - 1) - 0.5, height - 1 - ty + 0.5
            sx = np.array([2 * x0 / width - 1, 2 * x1 / width - 1]) / d
            sy = np.array([2 * f0 / height - 1, 2 * f1 / height - 1]) * (height / width) / d
            if all(sx[1] < r[0] or sx[0] > r[1] or sy[1] < r[2] or sy[0] > r[3] for r in rects):
                out.append((tx // 8, ty // 8))
    return out
