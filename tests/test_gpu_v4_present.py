"""The output stage fused into v4 device jobs (pt_v4_render_device_present).

Contract (include/pt_mi355.h): the accumulator ends bit for bit as pt_v4_render_device leaves it, and
`pixels` (nrows x width u32, row k = the job's row k) equals pt_tonemap_device on that accumulator.
Launches of 8 or more frames that run the continuous-tiles kernel (small images: PT_MI355_V4_CT=1)
with the default tonemap flags write the pixels in the kernel's presenting instances (pt_v4.hip
pt_v4_ct_kernel<..., PRESENT>); every other launch converts in a second pass.  Bar: BIT-EXACT whole
images against oracle/pt_oracle_v4.c (render4) and oracle/pt_oracle_output.c (tonemap).
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from conftest import bits_equal, mismatch_report
from layouts import interleaved_to_planar8
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

import cpuperformanceraytracer_amd as pt  # noqa: E402
from cpuperformanceraytracer_amd import _native as N  # noqa: E402

W, H, B = 72, 40, 8                                   # 9 x 5 tiles of 8 x 8 pixels
ROWS = dict(row_start=1, row_stride=3, nrows=13)      # rows 1, 4, .. 37: 9 x 2 tiles, the last 5 rows high
S, LAUNCHES = 16, 2                                   # two chunks of 8 frames per launch; frames 1 .. 32
FORMATS = [N.PT_PIXEL_RGBA8, N.PT_PIXEL_XRGB8]
LAYOUTS = [N.PT_LAYOUT_INTERLEAVED, N.PT_LAYOUT_PLANAR8]
POISON = 0x12345678                                   # a pixel word no launch has written


def _tex(h, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((h, w, 3), dtype=np.float32) * 3.0 + 0.01).astype(np.float32)


ENVS = {"none": (N.PT_V4_ENV_NONE, po.ENV_NONE, None),
        "equirect": (N.PT_V4_ENV_EQUIRECT, po.ENV_EQUIRECT, _tex(32, 64, 5)),
        "cubemap": (N.PT_V4_ENV_CUBEMAP, po.ENV_CUBEMAP, _tex(6 * 16, 16, 6))}   # six 16 x 16 faces stacked

# the edited scene (ClearScene / Add*ToScene): a floor, a light and a glass sphere -- (vertices | centre
# and radius, material) in AddMaterialToScene's argument order
QUADS = [np.array([[-25, -12, -5], [25, -12, -5], [25, -12, 30], [-25, -12, 30]], np.float32),
         np.array([[-6, 11, 8], [6, 11, 8], [6, 11, 18], [-6, 11, 18]], np.float32)]
SPHERES = [np.array([0, -4, 14, 6], np.float32)]
MATS = [dict(albedo=(0.7, 0.6, 0.5), emissive=(0, 0, 0), spec_chance=0.1, spec_rough=0.4, spec_color=(0.9, 0.9, 0.9),
             ior=1.0, refr_chance=0.0, refr_rough=0.0, refr_color=(0, 0, 0)),
        dict(albedo=(0, 0, 0), emissive=(12, 10, 8), spec_chance=0.0, spec_rough=0.0, spec_color=(0, 0, 0),
             ior=1.0, refr_chance=0.0, refr_rough=0.0, refr_color=(0, 0, 0)),
        dict(albedo=(0.9, 0.3, 0.3), emissive=(0, 0, 0), spec_chance=0.05, spec_rough=0.1, spec_color=(0.8, 0.8, 0.8),
             ior=1.3, refr_chance=0.8, refr_rough=0.2, refr_color=(0.1, 0.4, 0.2))]


def _oracle_scene():
    s = po.Scene4()
    s.nquads, s.nspheres, s.nmat = len(QUADS), len(SPHERES), len(MATS)
    for i, q in enumerate(QUADS):
        for k in range(4):
            for j in range(3):
                s.quad[i][k][j] = float(q[k, j])
    for i, p in enumerate(SPHERES):
        for j in range(4):
            s.sphere[i][j] = float(p[j])
    for i, m in enumerate(MATS):
        M = s.mat[i]
        for k in range(3):
            M.albedo[k], M.emissive[k] = float(m["albedo"][k]), float(m["emissive"][k])
            M.spec_color[k], M.refr_color[k] = float(m["spec_color"][k]), float(m["refr_color"][k])
        M.spec_chance, M.spec_rough, M.ior = m["spec_chance"], m["spec_rough"], m["ior"]
        M.refr_chance, M.refr_rough = m["refr_chance"], m["refr_rough"]
    return s


def _edit_scene():
    pt.ClearScene()
    for m in MATS:
        pt.AddMaterialToScene(m["albedo"], m["emissive"], m["spec_chance"], m["spec_rough"], m["spec_color"],
                              m["ior"], m["refr_chance"], m["refr_rough"], m["refr_color"])
    for q in QUADS:
        pt.AddQuadObjectToScene(q)
    for p in SPHERES:
        pt.AddSphereObjectToScene(p)


@functools.lru_cache(maxsize=None)
def _ref(env: str, edited: bool, frames: int = S * LAUNCHES, w: int = W, h: int = H, rows: bool = True):
    """The oracle's accumulator of frames 1 .. frames (interleaved; computed once per case, read-only)."""
    _, omode, tex = ENVS[env]
    a = po.render4(w, h, nframes=frames, num_bounces=B, env=tex, env_mode=omode,
                   scene=_oracle_scene() if edited else None, **(ROWS if rows else {}))
    a.setflags(write=False)
    return a


@pytest.fixture
def lib(monkeypatch):
    """The library initialised under the case's switches (pt_init reads them), released after."""
    def init(ct=True, no_ct=False, env="none", edited=False, **cfg):
        for k in ("PT_MI355_NO_CT", "PT_MI355_CT_WAVES", "PT_MI355_V4_CT"):
            monkeypatch.delenv(k, raising=False)
        if ct:
            monkeypatch.setenv("PT_MI355_V4_CT", "1")
        if no_ct:
            monkeypatch.setenv("PT_MI355_NO_CT", "1")
        pt.init(num_bounces=B)
        mode, _, tex = ENVS[env]
        pt.v4_config(env_mode=mode, num_bounces=B, **cfg)
        if tex is not None:
            pt.set_env_map(tex)
        if edited:
            _edit_scene()
    yield init
    pt.InitializeScene()
    pt.shutdown()


def _series(present, fmt=N.PT_PIXEL_RGBA8, *, layout=N.PT_LAYOUT_INTERLEAVED, env="none", frames=S, launches=LAUNCHES,
            w=W, h=H, rows=ROWS, start=None, slack=0):
    """`launches` launches of `frames` frames from frame 1 on an accumulator that starts as `start`
    (zeros); returns (accumulator as stored, pixels nrows x w or None, the `slack` words after them)."""
    import torch
    from cpuperformanceraytracer_amd.device import render_v4_device, render_v4_device_present
    nrows = rows.get("nrows", h)
    buf = (torch.zeros(nrows * w * 3, dtype=torch.float32, device="cuda:0") if start is None
           else torch.from_numpy(np.ascontiguousarray(start, np.float32).reshape(-1).copy()).to("cuda:0"))
    pix = torch.full((nrows * w + slack,), POISON, dtype=torch.int32, device="cuda:0")
    for k in range(launches):
        kw = dict(frame_first=1 + k * frames, nframes=frames, num_bounces=B, layout=layout, use_env=env != "none", **rows)
        if present:
            render_v4_device_present(buf, pix, w, h, pixel_format=fmt, **kw)
        else:
            render_v4_device(buf, w, h, **kw)
    torch.cuda.synchronize()
    p = pix.cpu().numpy().view(np.uint32)
    return buf.cpu().numpy(), (p[: nrows * w].reshape(nrows, w) if present else None), p[nrows * w:]


def _stored(ref, layout):
    return ref.reshape(-1) if layout == N.PT_LAYOUT_INTERLEAVED else interleaved_to_planar8(ref)


def _same_bits(got, want):
    assert bits_equal(got, want), mismatch_report(got, want)


# ---- 1. the fused path against the oracle --------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_fused_default_scene_matches_oracle_and_plain(lib, fmt, layout):
    lib()
    ref = _ref("none", False)
    acc, pix, _ = _series(True, fmt, layout=layout)
    _same_bits(acc, _stored(ref, layout))
    assert np.array_equal(pix, po.tonemap(ref, fmt)), f"{int((pix != po.tonemap(ref, fmt)).sum())} pixels differ"
    plain, _, _ = _series(False, layout=layout)
    _same_bits(acc, plain)


# ---- 2. env modes and the edited scene -----------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("env,edited", [("equirect", False), ("cubemap", False), ("equirect", True), ("cubemap", True),
                                        ("none", True)])
def test_fused_env_modes_and_edited_scene(lib, env, edited, layout):
    """Default flags; the edited scene reaches the generic-scene presenting instances (("none", True):
    theirs with the ambient miss term)."""
    lib(env=env, edited=edited)
    fmt = N.PT_PIXEL_XRGB8 if edited else N.PT_PIXEL_RGBA8
    ref = _ref(env, edited)
    acc, pix, _ = _series(True, fmt, layout=layout, env=env)
    _same_bits(acc, _stored(ref, layout))
    assert np.array_equal(pix, po.tonemap(ref, fmt)), f"{int((pix != po.tonemap(ref, fmt)).sum())} pixels differ"


# ---- 3. the fallback pass ------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["three_frames", "no_ct", "exact_tonemap", "zero_frames"])
def test_fallback_pass(lib, case):
    """Launches the presenting instances do not take: fewer than a chunk of frames, the per-tile pool
    (PT_MI355_NO_CT=1), tonemap flags the fused kernels do not carry, nothing to render."""
    tone = {}
    kw = {}
    if case == "three_frames":
        lib()
        kw = dict(frames=3, launches=1)
        ref = _ref("none", False, 3)
    elif case == "no_ct":
        lib(ct=False, no_ct=True)
        ref = _ref("none", False)
    elif case == "exact_tonemap":
        tone = dict(fast_aces=False, fast_gamma=False)
        lib(**tone)
        ref = _ref("none", False)
    else:   # an accumulator that already holds values is converted, nothing rendered
        lib()
        ref = _ref("none", False)
        kw = dict(frames=0, launches=1, start=ref)
    for fmt in FORMATS:
        acc, pix, _ = _series(True, fmt, **kw)
        want = po.tonemap(ref, fmt, **tone)
        assert np.array_equal(pix, want), f"{case}: {int((pix != want).sum())} pixels differ"
        _same_bits(acc, ref.reshape(-1))
        plain, _, _ = _series(False, **kw)
        _same_bits(acc, plain)


# ---- 4. ragged width -----------------------------------------------------------------------------
RW, RH, RS = 76, 24, 16   # 9.5 tile columns: the last column's tiles hold 4 pixel columns


def _ragged():
    ref = _ref("none", False, RS, RW, RH, False)
    acc, pix, after = _series(True, N.PT_PIXEL_RGBA8, frames=RS, launches=1, w=RW, h=RH, rows={}, slack=64)
    _same_bits(acc, ref.reshape(-1))
    want = po.tonemap(ref, N.PT_PIXEL_RGBA8)
    assert not (pix == POISON).any(), f"{int((pix == POISON).sum())} pixels never written"
    assert np.array_equal(pix, want), f"{int((pix != want).sum())} pixels differ"
    assert (after == POISON).all(), "words after the nrows x width pixels were written"


def test_ragged_width_every_pixel_written(lib):
    """Width 76 (interleaved layout): every pixel of the buffer is written and correct, none after it."""
    lib()
    _ragged()


def test_ragged_width_checked_build(lib):
    """The same case against the checked library (-DPT_CHECKED=1): its PT_G_PIXOUT guard reports any
    presented pixel outside nrows x width as PT_EKERNEL."""
    from cpuperformanceraytracer_amd.device import check_device_errors
    if N.load().pt_build_checked() != 1:
        pytest.skip("the library under test is not the checked build (build.build_checked(), then the suite "
                    "with PT_MI355_LIB=build/libpt_checked.so, as for test_gpu_guards.py)")
    lib()
    _ragged()
    check_device_errors()


# ---- 5. errors -----------------------------------------------------------------------------------
def test_errors(lib):
    import torch
    from cpuperformanceraytracer_amd.device import _job, _stream, render_v4_device_present
    lib()
    nrows = ROWS["nrows"]
    buf = torch.zeros(nrows * W * 3, dtype=torch.float32, device="cuda:0")
    pix = torch.zeros(nrows * W, dtype=torch.int32, device="cuda:0")
    job = _job(buf, W, H, ROWS["row_start"], ROWS["row_stride"], nrows, 1, S, B, N.PT_LAYOUT_INTERLEAVED)
    L = N.load()
    assert L.pt_v4_render_device_present(ctypes.byref(job), None, N.PT_PIXEL_RGBA8, _stream(None)) == N.PT_EINVAL
    assert L.pt_v4_render_device_present(ctypes.byref(job), pix.data_ptr(), 7, _stream(None)) == N.PT_EINVAL
    kw = dict(frame_first=1, nframes=S, num_bounces=B, **ROWS)
    with pytest.raises(N.PtError) as ei:
        render_v4_device_present(buf, pix, W, H, pixel_format=7, **kw)
    assert ei.value.code == N.PT_EINVAL
    with pytest.raises(N.PtError):   # (_check_pixels: not on the buffer's device)
        render_v4_device_present(buf, torch.zeros(nrows * W, dtype=torch.int32), W, H, **kw)
    with pytest.raises(N.PtError):   # (too few words)
        render_v4_device_present(buf, pix[:-1], W, H, **kw)
    with pytest.raises(N.PtError):   # (not 32-bit words)
        render_v4_device_present(buf, torch.zeros(nrows * W, dtype=torch.int16, device="cuda:0"), W, H, **kw)
    torch.cuda.synchronize()
    assert not buf.any().item() and not pix.any().item()   # (nothing was launched)
