"""A batch of v4 scenes in one launch (pt_v4_render_device_scenes): every view's slice against the camera
oracle of tests/v4_camera_oracle.py rendering that view's scene, BIT-EXACT -- the contract is "what
pt_v4_clear_scene, the description's pt_v4_add_* calls, pt_v4_set_camera and pt_v4_render_device leave on
that slice".

The hazards the cases are shaped around: a persistent wave of the scenes kernel takes tiles of several
views, so everything it derives from the view's scene -- the record pointer, both object counts, the
material rows and their precomputed constants -- has to be taken anew at each tile, and the four waves of a
block are on different scenes at once, so nothing of a scene may be shared by the block.

Scenes: S0 InitializeScene's (from pt_v4_get_scene_desc), S1 the oracle helper's edited scene, S2 S1's
geometry with other materials (an absorbing, rough refractive sphere; a specular, rough floor), S3 quads
only, S4 twelve objects (nine pairwise disjoint spheres), S5 empty.  Cameras: v4_camera_oracle.DEFAULT and
CAMERAS A-D (D lies inside the scenes' depth range: no sky window)."""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np
import pytest

import v4_camera_oracle as vo
from conftest import bits_equal, mismatch_report
from layouts import planar8_to_interleaved
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

import cpuperformanceraytracer_amd as pt  # noqa: E402
from cpuperformanceraytracer_amd import _native as N  # noqa: E402

B = 8
GRID_KNOB = "PT_MI355_V4_VIEWS_GRID"   # pt_init: at most this many blocks (of 4 waves) in a views / scenes launch


def _tex(h, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((h, w, 3), dtype=np.float32) * 3.0 + 0.01).astype(np.float32)


ENVS = {"none": (N.PT_V4_ENV_NONE, po.ENV_NONE, None),
        "equirect": (N.PT_V4_ENV_EQUIRECT, po.ENV_EQUIRECT, _tex(64, 128, 31)),
        "cubemap": (N.PT_V4_ENV_CUBEMAP, po.ENV_CUBEMAP, _tex(6 * 16, 16, 32))}   # six 16 x 16 faces stacked

_Z3 = (0.0, 0.0, 0.0)


def _mat(albedo=_Z3, emissive=_Z3, spec_chance=0.0, spec_rough=0.0, spec_color=_Z3, ior=1.0, refr_chance=0.0, refr_rough=0.0,
         refr_color=_Z3):
    return dict(albedo=albedo, emissive=emissive, spec_chance=spec_chance, spec_rough=spec_rough, spec_color=spec_color, ior=ior,
                refr_chance=refr_chance, refr_rough=refr_rough, refr_color=refr_color)


_WALL = np.array([[-10, -8, 2], [10, -8, 2], [10, 8, 2], [-10, 8, 2]], np.float32)
_S2_MATS = [dict(vo.MATS[0], spec_chance=0.3, spec_rough=0.4, spec_color=(0.8, 0.8, 0.9)), vo.MATS[1], vo.MATS[2],
            dict(vo.MATS[3], ior=1.33, refr_rough=0.2, refr_color=(0.6, 0.2, 0.9))]
_S4_SPHERES = [np.array([x, y, 9.0, 1.8], np.float32) for y in (-5.5, -1.0, 3.5) for x in (-6.0, 0.0, 6.0)]
_S4_MATS = [vo.MATS[0], vo.MATS[1], _mat(albedo=(0.5, 0.5, 0.5))] + [
    (_mat(albedo=(0.2 + 0.08 * k, 0.5, 0.5)), _mat(albedo=(0.6, 0.6, 0.6), spec_chance=0.5, spec_rough=0.1 * k, spec_color=(0.9, 0.7, 0.5)),
     _mat(albedo=(0.9, 0.9, 0.9), spec_chance=0.02, spec_color=(0.8, 0.8, 0.8), ior=1.1 + 0.05 * k, refr_chance=0.95,
          refr_rough=0.03 * k, refr_color=(0.1 * k, 0.3, 0.05)))[k % 3] for k in range(9)]
SCENES = {"S1": (vo.QUADS, vo.SPHERES, vo.MATS),
          "S2": (vo.QUADS, vo.SPHERES, _S2_MATS),
          "S3": (vo.QUADS + [_WALL], [], [vo.MATS[0], vo.MATS[1], _mat(albedo=(0.4, 0.7, 0.3))]),
          "S4": (vo.QUADS + [_WALL], _S4_SPHERES, _S4_MATS),
          "S5": ([], [], [])}
assert len(SCENES["S4"][0]) + len(SCENES["S4"][1]) == 12 and len(_S4_MATS) == 12
assert all(np.linalg.norm(a[:3] - b[:3]) > a[3] + b[3] + 0.5 for i, a in enumerate(_S4_SPHERES) for b in _S4_SPHERES[i + 1:])


def _scene(name: str):
    """The description the product is given: S0 is read back from the product (the default scene)."""
    if name == "S0":   # (only asked for while the current scene is the default one)
        d = pt.v4_get_scene_desc()
        assert (len(d["quads"]), len(d["spheres"]), len(d["materials"])) == (4, 7, 11)
        return d
    q, s, m = SCENES[name]
    return {"quads": q, "spheres": s, "materials": m}


def _camera(cam: str):
    return vo.DEFAULT if cam == "default" else vo.CAMERAS[cam]


@functools.lru_cache(maxsize=None)
def _ref(scene: str, cam: str, w: int, h: int, frames: int, env: str = "equirect", frame_first: int = 1, rows: tuple = (),
         random_jitter: bool = True, rejection: bool = True, fast_exp: bool = True):
    """The camera oracle's accumulator of `scene` seen by `cam`: computed once per case, shared, read-only.
    S0 is the oracle's own InitializeScene (no scene argument), not the product's description of it."""
    _, omode, tex = ENVS[env]
    sc = None if scene == "S0" else vo.oracle_scene(*SCENES[scene])
    r = dict(rows)
    nrows = r.get("nrows", h)
    vo.set_camera(*_camera(cam))
    a = np.zeros((nrows, w, 3), np.float32)
    p = po.Params4(w, h, r.get("row_start", 0), r.get("row_stride", 1), nrows, frame_first, frames, B,
                   omode if tex is not None else po.ENV_NONE, int(random_jitter), int(rejection), None,
                   min(os.cpu_count() or 1, 16), 0, int(not fast_exp))
    keep = None
    if tex is not None:
        keep = po.Env(tex.ctypes.data, tex.shape[1], tex.shape[0])
        p.env = ctypes.pointer(keep)
    assert vo.load().pto4_render(a.ctypes.data, ctypes.byref(p), ctypes.byref(sc) if sc is not None else None, None) == 0
    a.setflags(write=False)
    return a


@pytest.fixture
def lib(monkeypatch):
    """The library initialised under the case's switches (pt_init reads them); the default scene, camera and
    config again, and released, after."""
    def init(env="equirect", edited=False, grid=None, **cfg):
        monkeypatch.delenv(GRID_KNOB, raising=False)
        if grid is not None:
            monkeypatch.setenv(GRID_KNOB, str(grid))
        pt.init(num_bounces=B)
        mode, _, tex = ENVS[env]
        pt.v4_config(env_mode=mode, num_bounces=B, **cfg)
        if tex is not None:
            pt.set_env_map(tex)
        if edited:
            vo.edit_scene(pt)
    yield init
    pt.v4_camera()
    pt.InitializeScene()
    pt.v4_config()
    pt.shutdown()
    monkeypatch.delenv(GRID_KNOB, raising=False)


def _render(views, w, h, frames, *, scenes=None, mapping=None, env="equirect", frame_first=1, buf=None, nrows=None, stream=None, **kw):
    """views: (scene name, camera name) per view -- a scene per view unless `scenes` (names) and `mapping` say otherwise."""
    import torch
    from cpuperformanceraytracer_amd.device import render_v4_device_scenes
    nr = h if nrows is None else nrows
    if buf is None:
        buf = torch.zeros((len(views), nr, w, 3), dtype=torch.float32, device="cuda:0")
    names = [s for s, _ in views] if scenes is None else scenes
    render_v4_device_scenes(buf, [_scene(s) for s in names], [_camera(c) for _, c in views], w, h, mapping, frame_first=frame_first,
                            nframes=frames, num_bounces=B, use_env=env != "none", nrows=nrows, stream=stream, **kw)
    return buf


def _slices(buf, nviews, w, nrows, planar=False):
    import torch
    torch.cuda.synchronize()
    a = buf.cpu().numpy().reshape(nviews, nrows * w * 3)
    return [planar8_to_interleaved(a[v], w, nrows) if planar else a[v].reshape(nrows, w, 3) for v in range(nviews)]


def _same_bits(got, want, what=""):
    assert bits_equal(got, want), f"{what}: {mismatch_report(got, want)}"


def _check(buf, views, w, h, frames, planar=False, nrows=None, **ref):
    from cpuperformanceraytracer_amd.device import check_device_errors
    got = _slices(buf, len(views), w, h if nrows is None else nrows, planar)
    check_device_errors()
    for v, (s, c) in enumerate(views):
        _same_bits(got[v], _ref(s, c, w, h, frames, **ref), f"view {v} (scene {s}, camera {c})")


def _process_state():
    from cpuperformanceraytracer_amd.renderer import v4_scene_tables
    t, nq, ns = v4_scene_tables()
    return t.tobytes(), nq, ns, pt.v4_get_camera(), pt.v4_get_frame()


VIEWS1 = [("S0", "default"), ("S1", "A"), ("S2", "B"), ("S3", "C"), ("S4", "A"), ("S5", "D")]


def _each_slice(lib_init):
    import torch
    from cpuperformanceraytracer_amd.device import render_v4_device
    lib_init()
    before = _process_state()
    _check(_render(VIEWS1, 97, 61, 3), VIEWS1, 97, 61, 3)
    assert _process_state() == before
    # and the next plain job renders the current scene with the current camera
    one = torch.zeros(8 * 8 * 3, dtype=torch.float32, device="cuda:0")
    render_v4_device(one, 8, 8, frame_first=1, nframes=3, num_bounces=B, use_env=True)
    torch.cuda.synchronize()
    _same_bits(one.cpu().numpy().reshape(8, 8, 3), _ref("S0", "default", 8, 8, 3), "pt_v4_render_device after the scenes call")


# ---- 1. each slice is its (scene, camera)'s image ---------------------------------------------------
def test_each_slice_is_its_scenes_image(lib):
    """97 x 61 (ragged both ways), 3 frames, equirect; the process-wide scene, camera and frame counter are as
    before, and a following pt_v4_render_device renders the current (default) scene."""
    _each_slice(lib)


# ---- 2. a wave crosses scenes -----------------------------------------------------------------------
CROSSINGS = {
    # same geometry, other materials: a material row or a MatX row kept across the tile boundary shows
    "materials": [("S1", "A"), ("S2", "A")],
    # object counts falling 12 -> 3 -> 0: a count kept across the boundary traces objects that are not there
    "counts": [("S4", "A"), ("S3", "A"), ("S5", "A")],
    # one scene, with and without a sky window
    "window": [("S1", "A"), ("S1", "D")],
}


@pytest.mark.parametrize("order", sorted(CROSSINGS))
def test_a_wave_crosses_scenes(lib, order):
    """24 x 24 views of 9 tiles, 8 views = 72 tiles on a grid of ONE block (the knob): its four waves are on
    different views -- so different scenes -- at once and each crosses from view to view."""
    lib(grid=1)
    cyc = CROSSINGS[order]
    views = [cyc[k % len(cyc)] for k in range(8)]
    w, h, frames = 24, 24, 3
    assert len(views) * 9 > 4 * 4
    _check(_render(views, w, h, frames), views, w, h, frames)


# ---- 3. the mapping ---------------------------------------------------------------------------------
def test_the_mapping_selects_the_scene(lib):
    lib()
    mapping = [1, 0, 1, 1, 0]
    names = ["S1", "S2"]
    cams = ["A", "B", "C", "default", "D"]
    views = [(names[m], c) for m, c in zip(mapping, cams)]
    _check(_render(views, 40, 24, 3, scenes=names, mapping=mapping), views, 40, 24, 3)


def test_one_scene_equals_the_views_call(lib):
    """nscenes 1, the current (edited) scene's description: accumulators and pixels bit-equal to
    pt_v4_render_device_views on the same cameras -- GPU against GPU."""
    import torch
    from cpuperformanceraytracer_amd.device import render_v4_device_scenes, render_v4_device_views
    lib(edited=True)
    cams = [_camera(c) for c in ("A", "B", "C", "D", "default")]
    w, h, frames = 40, 24, 3
    acc = [torch.zeros((5, h, w, 3), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    pix = [torch.full((5, h, w), 0x12345678, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    kw = dict(frame_first=1, nframes=frames, num_bounces=B, use_env=True)
    render_v4_device_views(acc[0], cams, w, h, pixels=pix[0], **kw)
    render_v4_device_scenes(acc[1], [pt.v4_get_scene_desc()], cams, w, h, [0] * 5, pixels=pix[1], **kw)
    torch.cuda.synchronize()
    assert torch.equal(acc[0].view(torch.int32), acc[1].view(torch.int32))
    assert torch.equal(pix[0], pix[1])
    _same_bits(acc[1][0].cpu().numpy(), _ref("S1", "A", w, h, frames), "view 0 vs oracle")


# ---- 4. every compiled instance -----------------------------------------------------------------------
@pytest.mark.parametrize("fast_exp", [1, 0])
@pytest.mark.parametrize("layout", ["interleaved", "planar8"])
@pytest.mark.parametrize("env", ["none", "equirect", "cubemap"])
def test_instance_matrix(lib, env, layout, fast_exp):
    """40 x 24 x 2 frames, S1 and S2 (whose refractive sphere absorbs: the exp branch)."""
    lib(env=env, fast_exp=fast_exp)
    views = [("S1", "A"), ("S2", "B")]
    planar = layout == "planar8"
    buf = _render(views, 40, 24, 2, env=env, layout=N.PT_LAYOUT_PLANAR8 if planar else N.PT_LAYOUT_INTERLEAVED)
    _check(buf, views, 40, 24, 2, planar=planar, env=env, fast_exp=bool(fast_exp))


@pytest.mark.parametrize("flag", ["random_jitter", "rejection"])
def test_sampling_flags_off(lib, flag):
    lib(**{flag: 0})
    views = [("S2", "A"), ("S1", "B")]
    _check(_render(views, 40, 24, 2), views, 40, 24, 2, **{flag: False})


# ---- 5. chunks, frames and row shards -------------------------------------------------------------------
def test_three_chunks_from_a_late_frame(lib):
    """19 frames (two full LDS chunks and a partial one) from frame 999 990, 16 x 16."""
    lib()
    views = [("S2", "A"), ("S4", "C"), ("S1", "D")]
    _check(_render(views, 16, 16, 19, frame_first=999_990), views, 16, 16, 19, frame_first=999_990)


def test_row_shard(lib):
    lib()
    rows = dict(row_start=3, row_stride=4, nrows=12)   # rows 3, 7, .. 47 of 48
    views = [("S1", "B"), ("S3", "A")]
    buf = _render(views, 64, 48, 3, **rows)
    _check(buf, views, 64, 48, 3, nrows=12, rows=tuple(rows.items()))


# ---- 6. pixels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,fast_gamma", [(N.PT_PIXEL_RGBA8, 1), (N.PT_PIXEL_XRGB8, 1), (N.PT_PIXEL_RGBA8, 0), (N.PT_PIXEL_XRGB8, 0)])
def test_pixels_equal_the_output_stage(lib, fmt, fast_gamma):
    """The fused pair (1, 1) and a non-default pair (the second pass): each pixel slice is the oracle's output
    stage on its accumulator slice, and the accumulators are the oracle's."""
    import torch
    lib(fast_gamma=fast_gamma)
    views = [("S2", "A"), ("S0", "default"), ("S5", "B")]
    w, h = 41, 27
    pix = torch.full((3, h, w), 0x12345678, dtype=torch.int32, device="cuda:0")
    buf = _render(views, w, h, 3, pixels=pix, pixel_format=fmt)
    _check(buf, views, w, h, 3)
    got = pix.cpu().numpy().view(np.uint32)
    for v, (s, c) in enumerate(views):
        want = po.tonemap(_ref(s, c, w, h, 3), fmt, True, bool(fast_gamma))
        assert np.array_equal(got[v], want), f"view {v}: {int((got[v] != want).sum())} pixels differ"


# ---- 7. the table ring ----------------------------------------------------------------------------------
def test_back_to_back_launches_keep_their_tables(lib):
    """Six launches on one stream, six different scene sets (of 2 to 6 scenes: the ring's blocks also grow),
    no synchronisation between them -- two more than the ring has slots.  A slot reused too early shows as
    another launch's scenes."""
    import torch
    lib()
    w, h, frames = 24, 16, 3
    sets = [[("S1", "A"), ("S2", "B")], [("S2", "A"), ("S3", "B"), ("S4", "A")], [("S4", "B"), ("S5", "A")],
            [("S5", "B"), ("S1", "B"), ("S3", "A"), ("S2", "B")], [("S3", "B"), ("S1", "A")],
            [("S2", "A"), ("S4", "B"), ("S1", "B"), ("S5", "A"), ("S3", "A"), ("S4", "A")]]
    descs = {s: _scene(s) for s in SCENES}
    from cpuperformanceraytracer_amd.device import render_v4_device_scenes
    bufs = [torch.zeros((len(v), h, w, 3), dtype=torch.float32, device="cuda:0") for v in sets]
    torch.cuda.synchronize()
    for k, views in enumerate(sets):
        render_v4_device_scenes(bufs[k], [descs[s] for s, _ in views], [_camera(c) for _, c in views], w, h, frame_first=1,
                                nframes=frames, num_bounces=B, use_env=True)
    for k, views in enumerate(sets):
        _check(bufs[k], views, w, h, frames)


# ---- 8. the checked build ---------------------------------------------------------------------------------
def test_no_guard_fires_in_the_checked_build(lib):
    """Test 1 under build/libpt_checked.so (PT_MI355_LIB names it, as tests/test_gpu_guards.py expects): the
    scene-index and object-count guards of the scenes kernel stay silent (_check asks check_device_errors)."""
    if "checked" not in os.environ.get("PT_MI355_LIB", ""):
        pytest.skip("PT_MI355_LIB does not name the checked build")
    assert N.load().pt_build_checked() == 1
    _each_slice(lib)
