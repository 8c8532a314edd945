"""The reference's own v4 renderer as a test input -- helper (a plain module, like layouts.py).

oracle/build_ref.sh compiles demofox_path_tracing_optimization_v4.cpp :1-1556 inside oracle/ref_v4.cpp
once per flag variant (oracle/_ref/ref_v4_<variant>).  This module names the variants, the cases of
the committed fixtures (tests/golden/v4_ref_*.npz, written by tests/golden/make_golden_v4.py), runs a
binary, and renders a case with the v4 oracle.  GPU tests use only load() and the tables; they never
touch oracle/_ref/.
"""
from __future__ import annotations

import functools
import subprocess
import tempfile
from pathlib import Path

import numpy as np

import v4_camera_oracle as vo
from layouts import tiled_to_interleaved
from oracle import pyoracle as po

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
REF_DIR = ROOT / "oracle" / "_ref"

W, H, TW, TH = 64, 48, 16, 16   # several tiles both ways; 8-lane groups cross the silhouettes
B = 8                           # c_numBounces (v4 :23)

# variant -> (env, po.render4 switches, pt.v4_config switches, po.tonemap switches)
# (global_preprocessor_flags.h :56-66; the changed lines are recorded in manifest.json "v4_ref")
VARIANTS = {
    "shipped":  ("equirect", {}, {}, {}),
    "cubemap":  ("cubemap", {}, {}, {}),
    "bilinear": ("equirect", dict(random_jitter=False), dict(random_jitter=False), {}),
    "angle":    ("equirect", dict(rejection=False), dict(rejection=False), {}),
    "noenv":    ("none", {}, {}, {}),
    "exactexp": ("equirect", dict(fast_exp=False), dict(fast_exp=False), {}),
    "exactout": ("equirect", {}, dict(fast_aces=False, fast_gamma=False), dict(fast_aces=False, fast_gamma=False)),
    "noaccum":  ("equirect", dict(accumulate=False), dict(accumulate_frames=False), {}),
}
ENV_MODE = {"none": po.ENV_NONE, "equirect": po.ENV_EQUIRECT, "cubemap": po.ENV_CUBEMAP}


def synth_env(kind: str, seed_equirect: int = 31, seed_cubemap: int = 32):
    """The seeded synthetic env maps of the GPU tests (test_gpu_v4_camera._tex): 64 x 128 equirect,
    six stacked 16 x 16 faces."""
    def tex(h, w, seed):
        rng = np.random.default_rng(seed)
        return (rng.random((h, w, 3), dtype=np.float32) * 3.0 + 0.01).astype(np.float32)
    if kind == "equirect":
        return tex(64, 128, seed_equirect)
    if kind == "cubemap":
        return tex(6 * 16, 16, seed_cubemap)
    return None


# ---- the edited scene: what InitializeScene's geometry never exercises --------------------------------
# quad 0: a floor; quad 1: NON-PARALLELOGRAM and NON-PLANAR (V3 is off V0 + (V2 - V1) and off the plane
# of V0 V1 V2), emissive, so PrecomputeQuadData's DetTop (v4 :294-297: dot(cross(V30, V01), N), not
# the top triangle's own determinant) decides which rays hit its top half; sphere 0: small radius;
# sphere 1: refractive with absorption.  Materials in object order (quads first), 17 f32 each in
# SceneMaterial's member order.
SCENE_QUADS = np.array([[[-12, -8, 0], [12, -8, 0], [12, -8, 18], [-12, -8, 18]],
                        [[-7, -2, 4], [1, -3, 5], [2.5, 5, 6.5], [-9, 9, 2]]], np.float32)
SCENE_SPHERES = np.array([[6, -7.25, 12, 0.75], [4.5, -4, 9, 3.5]], np.float32)
SCENE_MATS = np.array([
    #  albedo            emissive        sc    sr    spec colour      ior  rc   rr   refraction colour
    [0.7, 0.65, 0.6,   0, 0, 0,        0.0,  0.0,  0, 0, 0,         1.0, 0.0, 0.0, 0, 0, 0],
    [0.2, 0.2, 0.2,    9, 7.5, 6,      0.0,  0.0,  0, 0, 0,         1.0, 0.0, 0.0, 0, 0, 0],
    [0.3, 0.6, 0.8,    0, 0, 0,        0.3,  0.2,  0.9, 0.8, 0.7,   1.3, 0.0, 0.0, 0, 0, 0],
    [0.9, 0.9, 0.9,    0, 0, 0,        0.04, 0.05, 0.9, 0.9, 0.9,   1.5, 0.9, 0.1, 0.05, 0.1, 0.02],
], np.float32)


_MAT_KEYS = ("albedo", "emissive", "spec_chance", "spec_rough", "spec_color", "ior", "refr_chance", "refr_rough",
             "refr_color")


def _mat_dicts(mats) -> list[dict]:
    out = []
    for m in np.asarray(mats, np.float32):
        m = [float(x) for x in m]
        out.append(dict(zip(_MAT_KEYS, (m[0:3], m[3:6], m[6], m[7], m[8:11], m[11], m[12], m[13], m[14:17]))))
    return out


def oracle_scene(quads=SCENE_QUADS, spheres=SCENE_SPHERES, mats=SCENE_MATS) -> po.Scene4:
    return vo.oracle_scene(list(np.asarray(quads, np.float32)), list(np.asarray(spheres, np.float32)), _mat_dicts(mats))


def edit_scene(pt, quads=SCENE_QUADS, spheres=SCENE_SPHERES, mats=SCENE_MATS) -> None:
    """The same scene through the product's ClearScene / Add*ToScene."""
    vo.edit_scene(pt, list(np.asarray(quads, np.float32)), list(np.asarray(spheres, np.float32)), _mat_dicts(mats))


# ---- cases of the committed fixtures --------------------------------------------------------------
# name -> dict(variant, frames, frame0, edited, cam, screen); frames are calls of DemofoxRenderOptV4
# starting from iFrame = frame0 (so the frames rendered are frame0 + 1 .. frame0 + frames)
def _case(variant="shipped", frames=2, frame0=0, edited=False, cam=None, screen=False):
    return dict(variant=variant, frames=frames, frame0=frame0, edited=edited, cam=cam, screen=screen)


CASES = {
    "shipped_f1": _case(frames=1, screen=True),
    "shipped_f2": _case(frames=2),
    "shipped_f4": _case(frames=4, screen=True),
    "shipped_f12": _case(frames=12),                  # more than one 8-frame chunk of the continuous-tiles kernel
    **{f"{v}_f2": _case(variant=v, screen=(v == "exactout")) for v in VARIANTS if v != "shipped"},
    "shipped_f999999": _case(frame0=999999),          # f32 counter, (i32)iFrame seed, 1 / (iFrame + 1)
    "edited_default": _case(edited=True, screen=True),
    "edited_camA": _case(edited=True, cam="A", screen=True),
}


def fixture_path(name: str) -> Path:
    return GOLDEN / f"v4_ref_{name}.npz"


@functools.lru_cache(maxsize=None)
def load(name: str) -> dict:
    """A committed fixture: acc (the reference's tiled accumulator, flat), iframe, screen (or None),
    and the inputs it was rendered from (env, scene arrays, camera).  Read-only arrays."""
    z = np.load(fixture_path(name))
    d = {k: z[k] for k in z.files}
    for a in d.values():
        a.setflags(write=False)
    d.setdefault("screen", None)
    return d


@functools.lru_cache(maxsize=None)
def load_env(kind: str):
    """The env map the fixtures were rendered with ("none": None)."""
    if kind == "none":
        return None
    e = np.load(GOLDEN / f"v4_ref_env_{kind}.npz")["env"]
    e.setflags(write=False)
    return e


def ref_binary(variant: str) -> Path:
    return REF_DIR / f"ref_v4_{variant}"


def ref_available() -> bool:
    return all(ref_binary(v).exists() for v in VARIANTS)


def camera_args(cam):
    """(px, py, pz, distance) of a v4_camera_oracle camera name, the distance as the product and the
    camera oracle compute it (1 / tanf(fov / 2 ...) in f32)."""
    pos, fov = vo.CAMERAS[cam]
    return (*[float(np.float32(p)) for p in pos], float(vo.distance(fov)))


def run_ref(variant: str, *, w=W, h=H, tw=TW, th=TH, frames=1, frame0=0, env=None, scene=None, cam=None,
            screen=False) -> dict:
    """One process of oracle/_ref/ref_v4_<variant>: {"acc", "iframe", "screen"}."""
    with tempfile.TemporaryDirectory(prefix="refv4_") as td:
        td = Path(td)
        args = [str(ref_binary(variant)), f"out={td / 'out.bin'}", f"w={w}", f"h={h}", f"tw={tw}", f"th={th}",
                f"frames={frames}", f"frame0={frame0}", f"screen={int(screen)}"]
        if env is not None:
            np.ascontiguousarray(env, np.float32).tofile(td / "env.f32")
            args += [f"env={td / 'env.f32'}", f"ew={env.shape[1]}", f"eh={env.shape[0]}"]
        if scene is not None:
            quads, spheres, mats = scene
            with open(td / "scene.bin", "wb") as f:
                np.array([len(mats), len(quads), len(spheres)], np.int32).tofile(f)
                np.ascontiguousarray(mats, np.float32).tofile(f)
                np.ascontiguousarray(quads, np.float32).tofile(f)
                np.ascontiguousarray(spheres, np.float32).tofile(f)
            args.append(f"scene={td / 'scene.bin'}")
        if cam is not None:
            args.append("cam=" + ",".join(repr(float(c)) for c in cam))
        subprocess.run(args, check=True)
        raw = (td / "out.bin").read_bytes()
    hdr = np.frombuffer(raw, np.int32, 5)
    assert tuple(hdr[:4]) == (w, h, tw, th)
    n = w * h
    out = {"iframe": np.frombuffer(raw, np.float32, 1, 20).copy(),
           "acc": np.frombuffer(raw, np.float32, n * 3, 24).copy(), "screen": None}
    if hdr[4]:
        out["screen"] = np.frombuffer(raw, np.uint32, n, 24 + n * 12).copy().reshape(h, w)
    return out


def oracle_render(variant: str, *, w=W, h=H, frames=1, frame0=0, env=None, scene=None, cam=None) -> np.ndarray:
    """The v4 oracle's interleaved accumulator of the same run (frames frame0 + 1 .. frame0 + frames on a
    zeroed buffer); with a camera name, the camera oracle of v4_camera_oracle.py."""
    kind, okw, _, _ = VARIANTS[variant]
    kw = dict(frame_first=frame0 + 1, nframes=frames, num_bounces=B, env_mode=ENV_MODE[kind],
              env=env if kind != "none" else None, scene=oracle_scene(*scene) if scene is not None else None)
    if cam is not None:
        assert not (set(okw) - {"random_jitter", "rejection"})
        return vo.render4(w, h, camera=vo.CAMERAS[cam], **kw, **okw)
    return po.render4(w, h, **kw, **okw)


def oracle_screen(variant: str, acc: np.ndarray) -> np.ndarray:
    return po.tonemap(acc, po.PIXEL_XRGB8, **VARIANTS[variant][3])


def interleaved(acc_tiled: np.ndarray, w=W, h=H, tw=TW, th=TH) -> np.ndarray:
    return tiled_to_interleaved(np.asarray(acc_tiled), w, h, tw, th)
