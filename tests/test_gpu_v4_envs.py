"""A batch of v4 env maps in one launch (pt_v4_render_device_envs): every view's slice against the camera
oracle of tests/v4_camera_oracle.py rendering that view's scene under that view's texture, BIT-EXACT -- the
contract is "what pt_set_env_map(that texture), the scene's pt_v4_add_* calls, pt_v4_set_camera and
pt_v4_render_device leave on that slice".

The hazards the cases are shaped around: a persistent wave of the envs kernel goes from one
view's tiles to the next view's, so the texture's pointer, width and height have to be replaced together at
every tile -- a new pointer with old dimensions, an old pointer with new dimensions or nothing replaced are
the three ways to get it wrong; the deferred env misses of a tile carry no texture and must be drained
before the wave leaves the tile; and the four waves of a block are on different textures at once.

Every set lists its SMALLEST textures first: all textures of a set share one device allocation, so
dimensions kept from a larger texture index into the following textures of the same allocation -- a wrong
value, found by the comparison, never an access outside the allocation.

Scenes: S0 InitializeScene's (the current scene, scenes=None) and S1 / S2 / S4 / S5 as in
tests/test_gpu_v4_scenes.py (restated here).  Cameras: v4_camera_oracle.DEFAULT and CAMERAS A-D (D lies
inside the scenes' depth range: no sky window)."""
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
GRID_KNOB = "PT_MI355_V4_VIEWS_GRID"   # pt_init: at most this many blocks (of 4 waves) in a views / scenes / envs launch


def _tex(h, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((h, w, 3), dtype=np.float32) * 3.0 + 0.01).astype(np.float32)


# (h, w), smallest first; e32a and e32b have one shape and other content: only the pointer tells them apart
EQUIRECT = {"e1x1": _tex(1, 1, 41), "e2x2": _tex(2, 2, 42), "e9x1": _tex(9, 1, 43), "e3x5": _tex(3, 5, 44),
            "e32a": _tex(32, 64, 45), "e32b": _tex(32, 64, 46), "e64": _tex(64, 128, 47)}
CUBEMAP = {"c1": _tex(6 * 1, 1, 51), "c4": _tex(6 * 4, 4, 52), "c16": _tex(6 * 16, 16, 53)}   # six faces stacked
TEX = {**EQUIRECT, **CUBEMAP}
MODES = {"equirect": (N.PT_V4_ENV_EQUIRECT, po.ENV_EQUIRECT), "cubemap": (N.PT_V4_ENV_CUBEMAP, po.ENV_CUBEMAP)}
for _pool in (EQUIRECT, CUBEMAP):
    _n = [t.size for t in _pool.values()]
    assert _n == sorted(_n), "smallest textures first"

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
          "S4": (vo.QUADS + [_WALL], _S4_SPHERES, _S4_MATS),
          "S5": ([], [], [])}


def _scene(name: str):
    q, s, m = SCENES[name]
    return {"quads": q, "spheres": s, "materials": m}


def _camera(cam: str):
    return vo.DEFAULT if cam == "default" else vo.CAMERAS[cam]


@functools.lru_cache(maxsize=None)
def _ref(scene: str, cam: str, tex: str, w: int, h: int, frames: int, frame_first: int = 1, rows: tuple = (),
         random_jitter: bool = True, fast_exp: bool = True):
    """The camera oracle's accumulator of `scene` (S0: its own InitializeScene) seen by `cam` under texture
    `tex`, read as its pool's mode: computed once per case, shared, read-only."""
    omode = po.ENV_CUBEMAP if tex in CUBEMAP else po.ENV_EQUIRECT
    t = TEX[tex]
    sc = None if scene == "S0" else vo.oracle_scene(*SCENES[scene])
    r = dict(rows)
    nrows = r.get("nrows", h)
    vo.set_camera(*_camera(cam))
    a = np.zeros((nrows, w, 3), np.float32)
    p = po.Params4(w, h, r.get("row_start", 0), r.get("row_stride", 1), nrows, frame_first, frames, B, omode, int(random_jitter), 1,
                   None, min(os.cpu_count() or 1, 16), 0, int(not fast_exp))
    keep = po.Env(t.ctypes.data, t.shape[1], t.shape[0])
    p.env = ctypes.pointer(keep)
    assert vo.load().pto4_render(a.ctypes.data, ctypes.byref(p), ctypes.byref(sc) if sc is not None else None, None) == 0
    a.setflags(write=False)
    return a


@pytest.fixture
def lib(monkeypatch):
    """The library initialised under the case's switches (pt_init reads them), with NO process-wide env map
    unless the case sets one; the default camera and config again, every set closed, and released, after."""
    sets = []

    def init(mode="equirect", grid=None, **cfg):
        monkeypatch.delenv(GRID_KNOB, raising=False)
        if grid is not None:
            monkeypatch.setenv(GRID_KNOB, str(grid))
        pt.init(num_bounces=B)
        pt.v4_config(env_mode=MODES[mode][0], num_bounces=B, **cfg)

        def make(names):
            from cpuperformanceraytracer_amd.device import make_v4_env_set
            sets.append(make_v4_env_set([TEX[n] for n in names]))
            return sets[-1]
        return make
    yield init
    for s in sets:
        s.close()
    pt.v4_camera()
    pt.InitializeScene()
    pt.v4_config()
    pt.shutdown()
    monkeypatch.delenv(GRID_KNOB, raising=False)


def _render(envs, views, w, h, frames, *, env_of_view=None, scenes=None, scene_of_view=None, frame_first=1, buf=None, nrows=None,
            **kw):
    """views: (scene name, camera name, texture name) per view; `scenes`: scene names, or None for the current scene."""
    import torch
    from cpuperformanceraytracer_amd.device import render_v4_device_envs
    nr = h if nrows is None else nrows
    if buf is None:
        buf = torch.zeros((len(views), nr, w, 3), dtype=torch.float32, device="cuda:0")
    render_v4_device_envs(buf, envs, [_camera(c) for _, c, _ in views], w, h, env_of_view,
                          None if scenes is None else [_scene(s) for s in scenes], scene_of_view, frame_first=frame_first,
                          nframes=frames, num_bounces=B, nrows=nrows, **kw)
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
    for v, (s, c, t) in enumerate(views):
        _same_bits(got[v], _ref(s, c, t, w, h, frames, **ref), f"view {v} (scene {s}, camera {c}, texture {t})")


def _mapped(names, order):
    """(env_of_view, texture name per view) for the set `names` visited in `order`."""
    return [names.index(t) for t in order], order


# ---- 1, 2. a wave crosses textures ---------------------------------------------------------------------
# the view order puts each stale-texture case on a view boundary: e64 -> e1x1 (dimensions kept: past the
# texture), e1x1 -> e64 (dimensions kept: texel 0 only; pointer kept: e1x1's neighbours), e32a -> e32b (only
# the pointer differs)
CROSSINGS = {
    "equirect": (list(EQUIRECT), ["e64", "e1x1", "e64", "e32a", "e32b", "e2x2", "e3x5", "e9x1"]),
    "cubemap": (list(CUBEMAP), ["c16", "c1", "c16", "c4", "c1", "c4", "c16", "c1"]),
}
CROSS_CAMS = ["A", "D", "B", "D", "C", "D", "default", "D"]   # with and without a sky window, alternating


def _crossing(lib, mode, random_jitter):
    make = lib(mode=mode, grid=1, random_jitter=random_jitter)
    names, order = CROSSINGS[mode]
    env_of_view, texs = _mapped(names, order)
    views = [("S0", c, t) for c, t in zip(CROSS_CAMS, texs)]
    w, h, frames = 24, 16, 9
    assert len(views) * 6 == 48 > 4 * 4
    buf = _render(make(names), views, w, h, frames, env_of_view=env_of_view)
    _check(buf, views, w, h, frames, random_jitter=bool(random_jitter))


@pytest.mark.parametrize("random_jitter", [1, 0], ids=["random", "bilinear"])
def test_a_wave_crosses_envs(lib, random_jitter):
    """8 views of 24 x 16 (6 tiles each, 48 entries) on a grid of ONE block (the knob): its four waves are on
    different views -- so different textures -- at once and each crosses from view to view.  9 frames are two
    chunks: the miss queue fills and drains twice per tile.  The current (default) scene, scenes=None."""
    _crossing(lib, "equirect", random_jitter)


@pytest.mark.parametrize("random_jitter", [1, 0], ids=["random", "bilinear"])
def test_a_wave_crosses_cubemaps(lib, random_jitter):
    _crossing(lib, "cubemap", random_jitter)


# ---- 3. everything per view ---------------------------------------------------------------------------
PER_VIEW_SCENES = ["S1", "S2", "S4", "S5"]
PER_VIEW = [("S1", "A", "e32a"), ("S2", "B", "e1x1"), ("S4", "C", "e64"), ("S5", "A", "e3x5"), ("S1", "B", "e32a"),
            ("S2", "C", "e2x2")]   # views 0 and 4 share a texture (and a scene)


def _per_view_maps():
    names = list(EQUIRECT)
    return names, [names.index(t) for _, _, t in PER_VIEW], [PER_VIEW_SCENES.index(s) for s, _, _ in PER_VIEW]


@pytest.mark.parametrize("fmt", [N.PT_PIXEL_RGBA8, N.PT_PIXEL_XRGB8])
def test_camera_scene_and_env_per_view(lib, fmt):
    """6 views of 40 x 24 at the default grid, a scene, a camera and a texture each; the pixels are the oracle's
    output stage on the oracle's slices."""
    import torch
    make = lib()
    names, emap, smap = _per_view_maps()
    w, h, frames = 40, 24, 3
    pix = torch.full((len(PER_VIEW), h, w), 0x12345678, dtype=torch.int32, device="cuda:0")
    buf = _render(make(names), PER_VIEW, w, h, frames, env_of_view=emap, scenes=PER_VIEW_SCENES, scene_of_view=smap, pixels=pix,
                  pixel_format=fmt)
    _check(buf, PER_VIEW, w, h, frames)
    got = pix.cpu().numpy().view(np.uint32)
    for v, (s, c, t) in enumerate(PER_VIEW):
        want = po.tonemap(_ref(s, c, t, w, h, frames), fmt, True, True)
        assert np.array_equal(got[v], want), f"view {v}: {int((got[v] != want).sum())} pixels differ"


def test_exact_exp_planar8(lib):
    make = lib(fast_exp=0)
    names, emap, smap = _per_view_maps()
    buf = _render(make(names), PER_VIEW, 40, 24, 3, env_of_view=emap, scenes=PER_VIEW_SCENES, scene_of_view=smap,
                  layout=N.PT_LAYOUT_PLANAR8)
    _check(buf, PER_VIEW, 40, 24, 3, planar=True, fast_exp=False)


@pytest.mark.parametrize("fast_exp", [1, 0])
@pytest.mark.parametrize("layout", ["interleaved", "planar8"])
@pytest.mark.parametrize("mode", ["equirect", "cubemap"])
def test_instance_matrix(lib, mode, layout, fast_exp):
    """Every compiled instance: 40 x 24 x 2 frames, S1 and S2 (whose refractive sphere absorbs: the exp branch)."""
    make = lib(mode=mode, fast_exp=fast_exp)
    names = list(EQUIRECT if mode == "equirect" else CUBEMAP)
    views = [("S1", "A", names[-1]), ("S2", "B", names[1])]
    planar = layout == "planar8"
    buf = _render(make(names), views, 40, 24, 2, env_of_view=[len(names) - 1, 1], scenes=["S1", "S2"],
                  layout=N.PT_LAYOUT_PLANAR8 if planar else N.PT_LAYOUT_INTERLEAVED)
    _check(buf, views, 40, 24, 2, planar=planar, fast_exp=bool(fast_exp))


# ---- 4. product against product------------------------------------------------------------------------
def test_one_call_equals_the_calls_one_by_one(lib):
    """3 views of 16 x 16 through one call, and pt_set_env_map + pt_v4_set_camera + pt_v4_render_device one by
    one on separate buffers -- GPU against GPU; afterwards the process-wide env map renders what it rendered
    before the call."""
    import torch
    from cpuperformanceraytracer_amd.device import render_v4_device
    make = lib()
    w = h = 16
    frames = 3
    kw = dict(frame_first=1, nframes=frames, num_bounces=B, use_env=True)
    views = [("S0", "A", "e2x2"), ("S0", "D", "e64"), ("S0", "B", "e32b")]

    def plain(tex, cam):
        one = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        pt.set_env_map(TEX[tex])
        pt.v4_camera(*_camera(cam))
        render_v4_device(one, w, h, **kw)
        torch.cuda.synchronize()
        return one
    singles = [plain(t, c) for _, c, t in views]
    before = plain("e3x5", "C")   # the process-wide env map and camera from here on
    state = (pt.v4_get_camera(), pt.v4_get_frame())
    batch = _render(make([t for _, _, t in views]), views, w, h, frames)
    torch.cuda.synchronize()
    for v, one in enumerate(singles):
        assert torch.equal(batch[v].view(torch.int32), one.view(torch.int32)), f"view {v}"
    assert (pt.v4_get_camera(), pt.v4_get_frame()) == state
    after = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    render_v4_device(after, w, h, **kw)
    torch.cuda.synchronize()
    assert torch.equal(after.view(torch.int32), before.view(torch.int32))
    _same_bits(after.cpu().numpy(), _ref("S0", "C", "e3x5", w, h, frames), "pt_v4_render_device after the envs call")


# ---- 5. what is rejected ----------------------------------------------------------------------------------
def test_rejected_mappings_and_modes(lib):
    import torch
    make = lib()
    envs = make(["e2x2", "e3x5"])
    views = [("S0", "A", "e2x2")] * 3
    buf = torch.full((3, 8, 8, 3), 7.0, dtype=torch.float32, device="cuda:0")

    def rejected(**kw):
        with pytest.raises(N.PtError) as e:
            _render(envs, views, 8, 8, 2, buf=buf, **kw)
        assert e.value.code == N.PT_EINVAL, str(e.value)
        return str(e.value)
    assert "2 textures" in rejected() and "3 views" in rejected()   # no env_of_view: count != nviews
    assert "view 1" in rejected(env_of_view=[0, -1, 1])
    assert "view 2" in rejected(env_of_view=[0, 1, 2])              # == count
    rejected(env_of_view=[0, 1, 0], use_env=False)
    pt.v4_config(env_mode=N.PT_V4_ENV_NONE, num_bounces=B)
    rejected(env_of_view=[0, 1, 0])
    pt.v4_config(env_mode=N.PT_V4_ENV_EQUIRECT, num_bounces=B)
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all()), "a rejected call wrote the buffer"
    ok = [("S0", "A", "e2x2"), ("S0", "A", "e3x5"), ("S0", "A", "e2x2")]
    _check(_render(envs, ok, 8, 8, 2, env_of_view=[0, 1, 0]), ok, 8, 8, 2)


# ---- 6. the life of a set ---------------------------------------------------------------------------------
def test_a_freed_set_leaves_no_record(lib):
    """A set is closed and another made with other shapes (most likely in the same memory): the next launch
    reads the new set's records."""
    make = lib()
    first = make(["e2x2", "e32a", "e64"])
    views = [("S0", "A", "e64"), ("S0", "B", "e2x2"), ("S0", "C", "e32a")]
    _check(_render(first, views, 16, 16, 2, env_of_view=[2, 0, 1]), views, 16, 16, 2)
    first.close()
    first.close()   # (harmless)
    with pytest.raises(N.PtError):
        _render(first, views, 16, 16, 2, env_of_view=[2, 0, 1])
    second = make(["e1x1", "e9x1", "e32b"])
    views = [("S0", "A", "e32b"), ("S0", "B", "e1x1"), ("S0", "C", "e9x1")]
    _check(_render(second, views, 16, 16, 2, env_of_view=[2, 0, 1]), views, 16, 16, 2)


def test_two_sets_on_two_streams(lib):
    import torch
    make = lib()
    a, b = make(["e3x5", "e32a"]), make(["e2x2", "e64"])
    va = [("S0", "A", "e3x5"), ("S0", "B", "e32a")]
    vb = [("S0", "A", "e2x2"), ("S0", "B", "e64")]
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    bufs = [torch.zeros((2, 16, 24, 3), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    _render(a, va, 24, 16, 3, buf=bufs[0], stream=sa)
    _render(b, vb, 24, 16, 3, buf=bufs[1], stream=sb)
    _check(bufs[0], va, 24, 16, 3)
    _check(bufs[1], vb, 24, 16, 3)


# ---- 7. row shards and late frames -------------------------------------------------------------------------
def test_row_shard_from_a_late_frame(lib):
    make = lib()
    rows = dict(row_start=1, row_stride=2, nrows=12)   # rows 1, 3, .. 23 of 24
    views = [("S1", "B", "e3x5"), ("S2", "A", "e64")]
    buf = _render(make(["e3x5", "e64"]), views, 40, 24, 3, scenes=["S1", "S2"], frame_first=999_990, **rows)
    _check(buf, views, 40, 24, 3, nrows=12, rows=tuple(rows.items()), frame_first=999_990)


# ---- 8. the checked build ------------------------------------------------------------------------------------
def test_no_guard_fires_in_the_checked_build(lib):
    """The crossing test under build/libpt_checked.so (PT_MI355_LIB names it, as tests/test_gpu_guards.py
    expects): the env-index and record guards of the envs kernel stay silent (_check asks check_device_errors)."""
    if "checked" not in os.environ.get("PT_MI355_LIB", ""):
        pytest.skip("PT_MI355_LIB does not name the checked build")
    assert N.load().pt_build_checked() == 1
    _crossing(lib, "equirect", 1)
