"""The v4 kernels against the reference's own v4 code: tests/golden/v4_ref_*.npz are runs of
demofox_path_tracing_optimization_v4.cpp :1-1556 itself (tests/golden/make_golden_v4.py; what its GCC
build substitutes is listed in oracle/ref_v4_shim.h).  Only tests/golden/ is read here.

Bar: BIT-EXACT -- the tiled accumulator RenderTile wrote, OutputToScreen's pixels, the frame counter.
Image 64 x 48 in 16 x 16 tiles, 8 bounces; every case is one or a few launches.

  drop-in  DemofoxRenderOptV4 (pt_render_opt_v4), one call per frame: shipped flags at 1 and 4 calls,
           every pt_v4_config variant, the edited scene (a non-parallelogram non-planar quad, a small
           sphere, a refractive sphere) from the default camera and from camera A;
  device   render_v4_device: one 4-frame launch (the per-tile kernel); the same with PT_MI355_V4_CT=1
           (the continuous-tiles kernel takes only launches of a whole 8-frame chunk,
           pt_kernel_pick.h pt_pick_v4_ct_takes, so 4 frames stay with the per-tile kernel); one
           12-frame launch and a 4 + 8-frame pair under PT_MI355_V4_CT=1 (the continuous-tiles kernel: a
           whole chunk and a short one; a chunk that starts at frame 5); frames 1 000 000 - 1 000 001.
"""
from __future__ import annotations

import numpy as np
import pytest

import v4_camera_oracle as vo
import v4_ref as vr
from conftest import bits_equal, mismatch_report

pytestmark = pytest.mark.gpu

import cpuperformanceraytracer_amd as pt  # noqa: E402
from cpuperformanceraytracer_amd import _native as N  # noqa: E402

W, H, TW, TH, B = vr.W, vr.H, vr.TW, vr.TH, vr.B
PT_ENV = {"none": N.PT_V4_ENV_NONE, "equirect": N.PT_V4_ENV_EQUIRECT, "cubemap": N.PT_V4_ENV_CUBEMAP}


def _same_bits(got, want):
    assert bits_equal(got, want), mismatch_report(got, want)


@pytest.fixture
def lib(monkeypatch):
    """The library initialised under the case's switches (pt_init reads them); the default camera and
    scene again, and released, after.  Returns the case's env map."""
    def init(name, ct=False):
        c = vr.CASES[name]
        fx = vr.load(name)
        kind, _, cfg, _ = vr.VARIANTS[c["variant"]]
        monkeypatch.delenv("PT_MI355_V4_CT", raising=False)
        if ct:
            monkeypatch.setenv("PT_MI355_V4_CT", "1")
        pt.init(num_bounces=B)
        pt.v4_config(env_mode=PT_ENV[kind], num_bounces=B, **cfg)
        env = vr.load_env(kind)
        if env is not None:
            pt.set_env_map(env)
        if c["edited"]:
            vr.edit_scene(pt, fx["quads"], fx["spheres"], fx["mats"])
        if c["cam"]:
            pt.v4_camera(*vo.CAMERAS[c["cam"]])
            got = pt.v4_get_camera()
            assert (*np.float32(got["position"]).tolist(), float(np.float32(got["distance"]))) == tuple(fx["cam"].tolist())
        return c, fx, env
    yield init
    pt.v4_camera()
    pt.InitializeScene()
    pt.shutdown()
    monkeypatch.delenv("PT_MI355_V4_CT", raising=False)


# ---- the drop-in ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in vr.CASES if n not in ("shipped_f12", "shipped_f999999")])
def test_drop_in_equals_reference(lib, name):
    """DemofoxRenderOptV4 called as the reference host calls it, frames times on a zeroed buffer with a
    screen buffer: the tiled accumulator, the pixels and the frame counter of the reference's run."""
    c, fx, env = lib(name)
    tex = pt.texture(env, env.shape[1], env.shape[0], 3) if env is not None else None
    buf = np.zeros(W * H * 3, np.float32)
    screen = np.zeros(W * H, np.uint32)
    for _ in range(c["frames"]):
        pt.DemofoxRenderOptV4(buf, W, H, W // TW, H // TH, TW, TH, 3, tex, screen)
    _same_bits(vr.interleaved(buf), vr.interleaved(fx["acc"]))
    assert np.array_equal(buf.view(np.uint32), fx["acc"].view(np.uint32))   # the tiled bytes themselves
    assert float(pt.v4_get_frame()) == float(fx["iframe"][0])
    if fx["screen"] is not None:
        assert np.array_equal(screen.reshape(H, W), fx["screen"]), \
            f"{int((screen.reshape(H, W) != fx['screen']).sum())} pixels differ"


def test_drop_in_frame_999999(lib):
    """iFrame 999 999 before the first of two calls: the f32 counter, the (i32)iFrame seed and the
    blend factor 1 / (iFrame + 1) at frames 1 000 000 and 1 000 001."""
    c, fx, env = lib("shipped_f999999")
    tex = pt.texture(env, env.shape[1], env.shape[0], 3)
    buf = np.zeros(W * H * 3, np.float32)
    pt.v4_set_frame(c["frame0"])
    for _ in range(c["frames"]):
        pt.DemofoxRenderOptV4(buf, W, H, W // TW, H // TH, TW, TH, 3, tex, None)
    _same_bits(vr.interleaved(buf), vr.interleaved(fx["acc"]))
    assert float(pt.v4_get_frame()) == float(fx["iframe"][0]) == 1000001.0


# ---- device jobs ----------------------------------------------------------------------------------
def _launch(frames, frame_first=1, buf=None):
    import torch
    from cpuperformanceraytracer_amd.device import render_v4_device
    if buf is None:
        buf = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda:0")
    render_v4_device(buf, W, H, frame_first=frame_first, nframes=frames, num_bounces=B, use_env=True)
    return buf


def _image(buf):
    import torch
    torch.cuda.synchronize()
    return buf.cpu().numpy().reshape(H, W, 3)


@pytest.mark.parametrize("ct", [False, True])
def test_device_four_frames_one_launch(lib, ct):
    _, fx, _ = lib("shipped_f4", ct=ct)
    _same_bits(_image(_launch(4)), vr.interleaved(fx["acc"]))


def test_device_ct_kernel_twelve_frames_one_launch(lib):
    """PT_MI355_V4_CT=1, 12 frames in one launch: the continuous-tiles kernel, a whole chunk and a
    short one."""
    _, fx, _ = lib("shipped_f12", ct=True)
    _same_bits(_image(_launch(12)), vr.interleaved(fx["acc"]))


def test_device_ct_kernel_chunk_from_frame_five(lib):
    """Frames 1-4 by the per-tile kernel, then frames 5-12 by the continuous-tiles kernel on the same
    accumulator: its chunk starts off frame 1 and blends into what is there."""
    _, fx4, _ = lib("shipped_f4", ct=True)
    buf = _launch(4)
    _same_bits(_image(buf), vr.interleaved(fx4["acc"]))
    _launch(8, frame_first=5, buf=buf)
    _same_bits(_image(buf), vr.interleaved(vr.load("shipped_f12")["acc"]))


def test_device_frame_999999(lib):
    c, fx, _ = lib("shipped_f999999")
    _same_bits(_image(_launch(c["frames"], frame_first=c["frame0"] + 1)), vr.interleaved(fx["acc"]))


@pytest.mark.parametrize("name", ["edited_default", "edited_camA"])
def test_device_edited_scene(lib, name):
    """The edited scene through a device job (the generic instances and, from camera A, the sky window
    derived from PrecomputeQuadData's DetTop, pt_v4_skywin.h)."""
    c, fx, _ = lib(name)
    _same_bits(_image(_launch(c["frames"])), vr.interleaved(fx["acc"]))
