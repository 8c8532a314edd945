"""The settable v4 camera on the GPU (pt_v4_set_camera): every v4 entry point with cameras other than
the default one, both kernels (the per-tile pool and, with PT_MI355_V4_CT=1, the continuous-tiles one),
the default scene and an Add*ToScene scene that leaves whole tiles in the sky window (pt_v4_skywin.h).

Bar: BIT-EXACT whole images against the v4 oracle with its two camera literals replaced by globals
(tests/v4_camera_oracle.py; at the default camera it is the unpatched oracle, test_v4_camera_host.py).
Cameras (v4_camera_oracle.CAMERAS): A (3, -2, 30) 60 deg, B (-6.5, 4.25, 55) 90 deg, C (0, -6, 22) 75 deg,
D (0, 0, 8) 90 deg -- inside the scenes' depth range, so without a sky window.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import v4_camera_oracle as vo
from conftest import bits_equal, mismatch_report
from layouts import tiled_to_interleaved
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

import cpuperformanceraytracer_amd as pt  # noqa: E402
from cpuperformanceraytracer_amd import _native as N  # noqa: E402

B = 8


def _tex(h, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((h, w, 3), dtype=np.float32) * 3.0 + 0.01).astype(np.float32)


ENVS = {"none": (N.PT_V4_ENV_NONE, po.ENV_NONE, None),
        "equirect": (N.PT_V4_ENV_EQUIRECT, po.ENV_EQUIRECT, _tex(64, 128, 31)),
        "cubemap": (N.PT_V4_ENV_CUBEMAP, po.ENV_CUBEMAP, _tex(6 * 16, 16, 32))}   # six 16 x 16 faces stacked


@functools.lru_cache(maxsize=None)
def _ref(cam: str, w: int, h: int, frames: int, env: str = "equirect", edited: bool = False, random_jitter: bool = True,
         rows: tuple = ()):
    """The patched oracle's accumulator of frames 1 .. frames seen by camera `cam` (computed once per
    case, read-only)."""
    _, omode, tex = ENVS[env]
    a = vo.render4(w, h, camera=vo.DEFAULT if cam == "default" else vo.CAMERAS[cam], nframes=frames, num_bounces=B,
                   env=tex, env_mode=omode, random_jitter=random_jitter, scene=vo.oracle_scene() if edited else None,
                   **dict(rows))
    a.setflags(write=False)
    return a


@pytest.fixture
def lib(monkeypatch):
    """The library initialised under the case's switches (pt_init reads them); the default camera and
    scene again, and released, after."""
    def init(ct=False, env="equirect", edited=False, cam="default", **cfg):
        monkeypatch.delenv("PT_MI355_V4_CT", raising=False)
        if ct:
            monkeypatch.setenv("PT_MI355_V4_CT", "1")   # the continuous-tiles kernel for launches of >= 8 frames
        pt.init(num_bounces=B)
        mode, _, tex = ENVS[env]
        pt.v4_config(env_mode=mode, num_bounces=B, **cfg)
        if tex is not None:
            pt.set_env_map(tex)
        if edited:
            vo.edit_scene(pt)
        pt.v4_camera(*(vo.DEFAULT if cam == "default" else vo.CAMERAS[cam]))
    yield init
    pt.v4_camera()
    pt.InitializeScene()
    pt.shutdown()
    monkeypatch.delenv("PT_MI355_V4_CT", raising=False)


def _render(w, h, frames, *, env="equirect", frame_first=1, buf=None, chain=False, **rows):
    import torch
    from cpuperformanceraytracer_amd.device import JobLauncher, render_v4_device
    nrows = rows.get("nrows", h)
    if buf is None:
        buf = torch.zeros(nrows * w * 3, dtype=torch.float32, device="cuda:0")
    if chain:
        JobLauncher(buf, w, h, nframes=frames, num_bounces=B, use_env=env != "none", v4=True, chain=True,
                    stream=torch.cuda.current_stream(), **rows)(frame_first)
    else:
        render_v4_device(buf, w, h, frame_first=frame_first, nframes=frames, num_bounces=B, use_env=env != "none", **rows)
    return buf


def _image(buf, w, nrows):
    import torch
    torch.cuda.synchronize()
    return buf.cpu().numpy().reshape(nrows, w, 3)


def _same_bits(got, want):
    assert bits_equal(got, want), mismatch_report(got, want)


# ---- 1. the default camera set explicitly is the default camera -----------------------------------
@pytest.mark.parametrize("ct", [False, True])
def test_default_camera_identity(lib, ct):
    """97 x 61 x 8 frames with the default camera set through the API: the unpatched oracle's image
    (the literal-camera instances; ct: the continuous-tiles one with its sky-frame prefix)."""
    lib(ct=ct, cam="default")
    assert pt.v4_get_camera() == {"position": (0.0, 0.0, 40.0), "fov_degrees": 90.0, "distance": 1.0}
    got = _image(_render(97, 61, 8), 97, 61)
    _same_bits(got, po.render4(97, 61, nframes=8, num_bounces=B, env=ENVS["equirect"][2]))


# ---- 2. the per-tile kernel, default scene ---------------------------------------------------------
@pytest.mark.parametrize("cam", ["A", "B", "C"])
def test_per_tile_kernel_default_scene(lib, cam):
    """97 x 61 x 3 frames (fewer than a chunk: the per-tile pool kernel), equirect 64 x 128: InitializeScene's
    geometry through the generic instances, with the sky window of (scene, camera)."""
    lib(cam=cam)
    assert pt.v4_sky_window()[0] == 11
    _same_bits(_image(_render(97, 61, 3), 97, 61), _ref(cam, 97, 61, 3))


# ---- 3. the continuous-tiles kernel, default scene -------------------------------------------------
def test_ct_kernel_camera_a_three_chunks(lib):
    lib(ct=True, cam="A")
    _same_bits(_image(_render(130, 70, 17), 130, 70), _ref("A", 130, 70, 17))


def test_ct_kernel_camera_c_cubemap_bilinear(lib):
    lib(ct=True, cam="C", env="cubemap", random_jitter=False)
    _same_bits(_image(_render(96, 64, 8, env="cubemap"), 96, 64), _ref("C", 96, 64, 8, "cubemap", False, False))


# ---- 4. the test scene: sky tiles at A, no window at D ----------------------------------------------
@pytest.mark.parametrize("ct", [False, True])
@pytest.mark.parametrize("cam", ["A", "D"])
def test_edited_scene(lib, cam, ct):
    """The Add*ToScene scene of v4_camera_oracle.py at 97 x 61: from A whole tiles lie outside every
    rectangle of the window (asserted), so waves skip TestSceneTrace (per-tile: 3 frames; continuous
    tiles: 8 frames, the sky-frame prefix); from D, inside the scene, there is no window."""
    lib(ct=ct, cam=cam, edited=True)
    n, rects = pt.v4_sky_window()
    if cam == "A":
        assert n == 4 and len(vo.sky_tiles(rects, 97, 61, *vo.CAMERAS["A"])) >= 1
    else:
        assert n == -1
    frames = 8 if ct else 3
    _same_bits(_image(_render(97, 61, frames), 97, 61), _ref(cam, 97, 61, frames, "equirect", True))


def test_edited_scene_counts_skipped_traces(lib):
    """The counted launch of the test scene from A: image and segment / escape counts as the oracle's,
    and some camera rays did skip their trace (sky_skipped) -- the window is consulted."""
    import torch
    from cpuperformanceraytracer_amd.device import count_v4_device
    lib(cam="A", edited=True)
    buf = torch.zeros(61 * 97 * 3, dtype=torch.float32, device="cuda:0")
    counts = count_v4_device(buf, 97, 61, frame_first=1, nframes=3, num_bounces=B, use_env=True)
    _same_bits(_image(buf, 97, 61), _ref("A", 97, 61, 3, "equirect", True))
    _, want = vo.render4(97, 61, camera=vo.CAMERAS["A"], nframes=3, num_bounces=B, env=ENVS["equirect"][2],
                         scene=vo.oracle_scene(), counts=True)
    assert counts["segments"] == want["segments"] and counts["escaped"] == want["escaped"], (counts, want)
    assert counts["sky_skipped"] > 0, counts


# ---- 5. a row shard --------------------------------------------------------------------------------
def test_row_shard_camera_b(lib):
    rows = dict(row_start=1, row_stride=3, nrows=20)   # rows 1, 4, .. 58 of 61
    lib(cam="B")
    got = _image(_render(97, 61, 3, **rows), 97, 20)
    _same_bits(got, _ref("B", 97, 61, 3, rows=tuple(rows.items())))


# ---- 6. the fused output stage ---------------------------------------------------------------------
def test_device_present_camera_a(lib):
    """pt_v4_render_device_present, 96 x 64 x 8 frames (the continuous-tiles kernel's generic presenting
    instance): the accumulator is the oracle's, the pixels po.tonemap of it."""
    import torch
    from cpuperformanceraytracer_amd.device import render_v4_device_present
    lib(ct=True, cam="A")
    buf = torch.zeros(64 * 96 * 3, dtype=torch.float32, device="cuda:0")
    pix = torch.full((64 * 96,), 0x12345678, dtype=torch.int32, device="cuda:0")
    render_v4_device_present(buf, pix, 96, 64, frame_first=1, nframes=8, num_bounces=B, use_env=True,
                             pixel_format=N.PT_PIXEL_RGBA8)
    ref = _ref("A", 96, 64, 8)
    _same_bits(_image(buf, 96, 64), ref)
    got = pix.cpu().numpy().view(np.uint32).reshape(64, 96)
    want = po.tonemap(ref, po.PIXEL_RGBA8)
    assert np.array_equal(got, want), f"{int((got != want).sum())} pixels differ"


# ---- 7. the drop-in ---------------------------------------------------------------------------------
def test_drop_in_camera_a(lib):
    """DemofoxRenderOptV4 (pt_render_opt_v4) on a host buffer, 64 x 48 in 16 x 16 tiles, 2 calls, with
    screen pixels: the tiled accumulator and OutputToScreen's pixels as the oracle's."""
    lib(cam="A")
    w, h, tw, th = 64, 48, 16, 16
    env = ENVS["equirect"][2]
    tex = pt.texture(env, env.shape[1], env.shape[0], 3)
    buf = np.zeros(w * h * 3, np.float32)
    screen = np.zeros(w * h, np.uint32)
    for _ in range(2):
        pt.DemofoxRenderOptV4(buf, w, h, w // tw, h // th, tw, th, 3, tex, screen)
    assert pt.v4_get_frame() == 2
    ref = _ref("A", w, h, 2)
    _same_bits(tiled_to_interleaved(buf, w, h, tw, th), ref)
    assert np.array_equal(screen.reshape(h, w), po.tonemap(ref, po.PIXEL_XRGB8))


# ---- 8. chained launches ---------------------------------------------------------------------------
def test_chain_restarts_after_a_camera_change(lib):
    """Two chained 8-frame launches at 96 x 64, the camera changed from A to C between them: the
    oracle's two-step sequence on one accumulator, and the second launch restarted the chain."""
    import torch
    from cpuperformanceraytracer_amd.device import chain_counts, check_device_errors
    lib(ct=True, cam="A")
    w, h = 96, 64
    c0 = chain_counts()
    buf = _render(w, h, 8, chain=True)
    pt.v4_camera(*vo.CAMERAS["C"])
    _render(w, h, 8, frame_first=9, buf=buf, chain=True)
    torch.cuda.synchronize()
    check_device_errors()
    c1 = chain_counts()
    # (96 tiles are fewer than the scheduler's minimum of 512, pt_launch_plan.h kSchedMinTiles: chained
    # calls of this geometry are plain launches and count as neither kind -- the live chain is the next test)
    assert c1["continued"] == c0["continued"], (c0, c1)
    env = ENVS["equirect"][2]
    ref = _ref("A", w, h, 8).copy()
    ref = vo.render4(w, h, camera=vo.CAMERAS["C"], frame_first=9, nframes=8, num_bounces=B, env=env, buf=ref)
    _same_bits(_image(buf, w, h), ref)


def test_camera_change_ends_a_live_chain(lib):
    """A geometry large enough to be scheduled (256 x 160: 640 tiles), so that chained launches do continue:
    six 8-frame launches from A (some continued), the camera changed to C, two more.  The launch after the
    change restarted; the image is the oracle's sequence."""
    import torch
    from cpuperformanceraytracer_amd.device import chain_counts, check_device_errors
    lib(ct=True, cam="A")
    w, h = 256, 160
    c0 = chain_counts()
    buf = None
    for k in range(6):
        buf = _render(w, h, 8, frame_first=1 + 8 * k, buf=buf, chain=True)
    c1 = chain_counts()
    assert c1["continued"] - c0["continued"] >= 1, (c0, c1)   # the chain was live
    pt.v4_camera(*vo.CAMERAS["C"])
    _render(w, h, 8, frame_first=49, buf=buf, chain=True)
    c2 = chain_counts()
    assert (c2["restarts"] - c1["restarts"], c2["continued"] - c1["continued"]) == (1, 0), (c1, c2)
    _render(w, h, 8, frame_first=57, buf=buf, chain=True)
    torch.cuda.synchronize()
    check_device_errors()
    env = ENVS["equirect"][2]
    ref = _ref("A", w, h, 48).copy()
    ref = vo.render4(w, h, camera=vo.CAMERAS["C"], frame_first=49, nframes=16, num_bounces=B, env=env, buf=ref)
    _same_bits(_image(buf, w, h), ref)
