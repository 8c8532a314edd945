"""A batch of v4 cameras in one launch (pt_v4_render_device_views): every view's slice against the camera
oracle of tests/v4_camera_oracle.py, BIT-EXACT -- the contract is "what pt_v4_set_camera + pt_v4_render_device
on that slice would leave", and test_gpu_v4_camera.py holds that path to the same oracle.

The hazard the cases are shaped around: a persistent wave of the views kernel takes tiles of several views,
so everything it derives from the camera (ray origin, distance, whether there is a sky window, its
rectangles) has to be taken anew at each tile.  Cameras A-D: v4_camera_oracle.CAMERAS (D lies inside the
scenes' depth range: no sky window).
"""
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
GRID_KNOB = "PT_MI355_V4_VIEWS_GRID"   # pt_init: at most this many blocks (of 4 waves) in a views launch


def _tex(h, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((h, w, 3), dtype=np.float32) * 3.0 + 0.01).astype(np.float32)


ENVS = {"none": (N.PT_V4_ENV_NONE, po.ENV_NONE, None),
        "equirect": (N.PT_V4_ENV_EQUIRECT, po.ENV_EQUIRECT, _tex(64, 128, 31)),
        "cubemap": (N.PT_V4_ENV_CUBEMAP, po.ENV_CUBEMAP, _tex(6 * 16, 16, 32))}   # six 16 x 16 faces stacked


def _camera(cam: str):
    return vo.DEFAULT if cam == "default" else vo.CAMERAS[cam]


@functools.lru_cache(maxsize=None)
def _ref(cam: str, w: int, h: int, frames: int, env: str = "equirect", edited: bool = False, random_jitter: bool = True,
         rows: tuple = (), fast_exp: bool = True):
    """The camera oracle's accumulator of frames 1 .. frames seen by `cam`: computed once per case and
    shared, read-only.  fast_exp False: the same library and camera globals with Params4.exact_exp set
    (v4_camera_oracle.render4 has no switch for it)."""
    _, omode, tex = ENVS[env]
    scene = vo.oracle_scene() if edited else None
    r = dict(rows)
    if fast_exp:
        a = vo.render4(w, h, camera=_camera(cam), nframes=frames, num_bounces=B, env=tex, env_mode=omode,
                       random_jitter=random_jitter, scene=scene, **r)
    else:
        vo.set_camera(*_camera(cam))
        nrows = r.get("nrows", h)
        a = np.zeros((nrows, w, 3), np.float32)
        p = po.Params4(w, h, r.get("row_start", 0), r.get("row_stride", 1), nrows, 1, frames, B,
                       omode if tex is not None else po.ENV_NONE, int(random_jitter), 1, None, min(os.cpu_count() or 1, 16), 0, 1)
        keep = None
        if tex is not None:
            keep = po.Env(tex.ctypes.data, tex.shape[1], tex.shape[0])
            p.env = ctypes.pointer(keep)
        assert vo.load().pto4_render(a.ctypes.data, ctypes.byref(p), ctypes.byref(scene) if scene is not None else None, None) == 0
    a.setflags(write=False)
    return a


@pytest.fixture
def lib(monkeypatch):
    """The library initialised under the case's switches (pt_init reads them); the default scene again,
    and released, after.  The process-wide camera is never set here: it stays the default one."""
    def init(env="equirect", edited=False, grid=None, ct=False, **cfg):
        monkeypatch.delenv(GRID_KNOB, raising=False)
        monkeypatch.delenv("PT_MI355_V4_CT", raising=False)
        if grid is not None:
            monkeypatch.setenv(GRID_KNOB, str(grid))
        if ct:
            monkeypatch.setenv("PT_MI355_V4_CT", "1")
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
    monkeypatch.delenv("PT_MI355_V4_CT", raising=False)


def _views(cams, w, h, frames, *, env="equirect", frame_first=1, buf=None, nrows=None, stream=None, **kw):
    import torch
    from cpuperformanceraytracer_amd.device import render_v4_device_views
    nr = h if nrows is None else nrows
    if buf is None:
        buf = torch.zeros((len(cams), nr, w, 3), dtype=torch.float32, device="cuda:0")
    render_v4_device_views(buf, [_camera(c) for c in cams], w, h, frame_first=frame_first, nframes=frames, num_bounces=B,
                           use_env=env != "none", nrows=nrows, stream=stream, **kw)
    return buf


def _slices(buf, nviews, w, nrows, planar=False):
    import torch
    torch.cuda.synchronize()
    a = buf.cpu().numpy().reshape(nviews, nrows * w * 3)
    return [planar8_to_interleaved(a[v], w, nrows) if planar else a[v].reshape(nrows, w, 3) for v in range(nviews)]


def _same_bits(got, want, what=""):
    assert bits_equal(got, want), f"{what}: {mismatch_report(got, want)}"


DEFAULT_CAMERA = {"position": (0.0, 0.0, 40.0), "fov_degrees": 90.0, "distance": 1.0}


# ---- 1. equal to one launch per view ----------------------------------------------------------------
def test_each_slice_is_its_cameras_image(lib):
    """97 x 61 (ragged both ways), 3 frames (less than a chunk), equirect 64 x 128, the default scene."""
    lib()
    cams = ["default", "A", "B", "C"]
    got = _slices(_views(cams, 97, 61, 3), 4, 97, 61)
    for v, c in enumerate(cams):
        _same_bits(got[v], _ref(c, 97, 61, 3), f"view {v} (camera {c})")
    assert pt.v4_get_camera() == DEFAULT_CAMERA
    assert pt.v4_get_frame() == 0


# ---- 2. a wave crosses views ------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["A", "D"])
def test_a_wave_crosses_views(lib, first):
    """16 x 8 (2 tiles per view), 11 frames (a full chunk and a partial one), the edited scene, cameras A
    (a window with whole sky tiles) and D (no window) alternating, 9 views = 18 tiles on a grid of ONE
    block (the knob): 4 waves, whose first tiles are tiles 0-3 -- views 0 and 1.  Both of those see
    `first`, and the rest alternate, so every tile of the other camera is taken by a wave that came from a
    tile of `first`: with a window to without (first A), and back (first D).  A camera kept across the
    tile boundary renders those slices wrong."""
    lib(edited=True, grid=1)
    other = "D" if first == "A" else "A"
    cams = [first, first] + [other if k % 2 == 0 else first for k in range(7)]
    w, h, frames = 16, 8, 11
    assert len(cams) * 2 > 1 * 4   # more tiles than the launch has waves
    got = _slices(_views(cams, w, h, frames), len(cams), w, h)
    for v, c in enumerate(cams):
        _same_bits(got[v], _ref(c, w, h, frames, "equirect", True), f"view {v} (camera {c})")


# ---- 3. a row-sharded job, planar8 -------------------------------------------------------------------
def test_row_shard_planar8_cubemap_bilinear(lib):
    lib(env="cubemap", random_jitter=False)
    rows = dict(row_start=1, row_stride=3, nrows=21)   # rows 1, 4, .. 61 of 64
    cams = ["C", "A"]
    buf = _views(cams, 96, 64, 8, env="cubemap", layout=N.PT_LAYOUT_PLANAR8, **rows)
    got = _slices(buf, 2, 96, 21, planar=True)
    for v, c in enumerate(cams):
        _same_bits(got[v], _ref(c, 96, 64, 8, "cubemap", False, False, tuple(rows.items())), f"view {v} (camera {c})")


# ---- 4. accumulation continues -----------------------------------------------------------------------
def test_two_launches_accumulate(lib):
    lib()
    cams = ["B", "default", "A"]
    buf = _views(cams, 40, 24, 3)
    _views(cams, 40, 24, 5, frame_first=4, buf=buf)
    got = _slices(buf, 3, 40, 24)
    for v, c in enumerate(cams):
        _same_bits(got[v], _ref(c, 40, 24, 8), f"view {v} (camera {c})")


# ---- 5. the view table is not reused while a launch reads it ------------------------------------------
def test_back_to_back_launches_keep_their_tables(lib):
    """Two launches on one stream with different camera lists and buffers and no synchronisation between
    them, a third right after on a second stream: each reads its own view table."""
    import torch
    lib()
    w, h, frames = 48, 32, 8
    lists = [["A", "B", "C", "default"], ["C", "default", "A", "B"], ["B", "A"]]
    s2 = torch.cuda.Stream()
    bufs = [torch.zeros((len(c), h, w, 3), dtype=torch.float32, device="cuda:0") for c in lists]
    torch.cuda.synchronize()
    _views(lists[0], w, h, frames, buf=bufs[0])
    _views(lists[1], w, h, frames, buf=bufs[1])
    _views(lists[2], w, h, frames, buf=bufs[2], stream=s2)
    for k, cams in enumerate(lists):
        got = _slices(bufs[k], len(cams), w, h)
        for v, c in enumerate(cams):
            _same_bits(got[v], _ref(c, w, h, frames), f"launch {k} view {v} (camera {c})")


# ---- 6. pixels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,fast_gamma", [(N.PT_PIXEL_RGBA8, 1), (N.PT_PIXEL_XRGB8, 1), (N.PT_PIXEL_RGBA8, 0)])
def test_pixels_equal_the_output_stage(lib, fmt, fast_gamma):
    """97 x 61 x 8 frames, cameras [A, default]: each pixel slice equals tonemap_device on its accumulator
    slice (fast_gamma 0: the second-pass path), and the accumulators are the oracle's."""
    import torch
    from cpuperformanceraytracer_amd.device import tonemap_device
    lib(fast_gamma=fast_gamma)
    cams = ["A", "default"]
    w, h = 97, 61
    pix = torch.full((2, h, w), 0x12345678, dtype=torch.int32, device="cuda:0")
    buf = _views(cams, w, h, 8, pixels=pix, pixel_format=fmt)
    got = _slices(buf, 2, w, h)
    for v, c in enumerate(cams):
        _same_bits(got[v], _ref(c, w, h, 8), f"view {v} (camera {c})")
        want = torch.zeros((h, w), dtype=torch.int32, device="cuda:0")
        tonemap_device(buf[v], w, h, want, pixel_format=fmt)
        torch.cuda.synchronize()
        assert torch.equal(pix[v], want), f"view {v}: {int((pix[v] != want).sum())} pixels differ"


# ---- 7. boundaries -------------------------------------------------------------------------------------
def test_one_view_equals_render_v4_device(lib):
    import torch
    from cpuperformanceraytracer_amd.device import render_v4_device
    lib()
    w, h = 97, 61
    got = _slices(_views(["C"], w, h, 3), 1, w, h)[0]
    pt.v4_camera(*vo.CAMERAS["C"])
    one = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda:0")
    render_v4_device(one, w, h, frame_first=1, nframes=3, num_bounces=B, use_env=True)
    torch.cuda.synchronize()
    _same_bits(got, one.cpu().numpy().reshape(h, w, 3), "views vs render_v4_device")
    _same_bits(got, _ref("C", w, h, 3), "views vs oracle")


def test_a_views_launch_restarts_a_live_chain(lib):
    """256 x 160 (640 tiles: scheduled, so chained launches continue): six chained 8-frame launches, a views
    launch on the same stream, one more chained launch -- which restarts; the chained accumulator is the
    oracle's 56 frames and the views' slices are their cameras' images."""
    import torch
    from cpuperformanceraytracer_amd.device import JobLauncher, chain_counts, check_device_errors
    lib(ct=True)
    w, h = 256, 160
    buf = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda:0")
    chained = JobLauncher(buf, w, h, nframes=8, num_bounces=B, use_env=True, v4=True, chain=True, stream=torch.cuda.current_stream())
    c0 = chain_counts()
    for k in range(6):
        chained(1 + 8 * k)
    c1 = chain_counts()
    assert c1["continued"] - c0["continued"] >= 1, (c0, c1)   # the chain was live
    vbuf = _views(["A", "C"], 24, 16, 3)
    chained(49)
    c2 = chain_counts()
    assert (c2["restarts"] - c1["restarts"], c2["continued"] - c1["continued"]) == (1, 0), (c1, c2)
    torch.cuda.synchronize()
    check_device_errors()
    _same_bits(buf.cpu().numpy().reshape(h, w, 3), po.render4(w, h, nframes=56, num_bounces=B, env=ENVS["equirect"][2]), "chained")
    got = _slices(vbuf, 2, 24, 16)
    for v, c in enumerate(["A", "C"]):
        _same_bits(got[v], _ref(c, 24, 16, 3), f"view {v} (camera {c})")


# ---- 8. every compiled views instance --------------------------------------------------------------------
@pytest.mark.parametrize("fast_exp", [1, 0])
@pytest.mark.parametrize("layout", ["interleaved", "planar8"])
@pytest.mark.parametrize("env", ["none", "equirect", "cubemap"])
def test_instance_matrix(lib, env, layout, fast_exp):
    lib(env=env, fast_exp=fast_exp)
    cams = ["A", "B"]
    planar = layout == "planar8"
    buf = _views(cams, 24, 16, 3, env=env, layout=N.PT_LAYOUT_PLANAR8 if planar else N.PT_LAYOUT_INTERLEAVED)
    got = _slices(buf, 2, 24, 16, planar=planar)
    for v, c in enumerate(cams):
        _same_bits(got[v], _ref(c, 24, 16, 3, env, fast_exp=bool(fast_exp)), f"view {v} (camera {c})")
