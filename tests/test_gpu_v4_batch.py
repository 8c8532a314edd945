"""Everything per view in one launch (pt_v4_render_device_batch): every view's slice against the camera oracle
of tests/v4_camera_oracle.py rendering that view's scene under that view's texture over that view's OWN frame
range, BIT-EXACT -- the contract is "what pt_set_env_map (or the ambient), the scene's pt_v4_add_* calls,
pt_v4_set_camera and pt_v4_render_device with frame_first = frames[v].frame_first and nframes =
frames[v].nframes leave on that slice".

The hazards the cases are shaped around: a persistent wave of the batch kernel goes from a view
of 9 frames (two chunks; kChunk is 8) to one of 1, to one of 0, to one of 17, so the chunk loop and the two
places that take the next queue entry must agree about the count (a disagreement shows as an unrendered tile);
first frame and count must come from one record (a stale first frame renders the right number of frames from
the wrong seeds); a view of 0 frames keeps its accumulator bit for bit, also when accumulate_frames is 0, and
still gets its pixels; and the four waves of a block are on four ranges at once.

Scenes, cameras and textures are those of tests/test_gpu_v4_envs.py."""
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
from test_gpu_v4_envs import CUBEMAP, EQUIRECT, GRID_KNOB, SCENES, TEX, _camera, _scene

pytestmark = pytest.mark.gpu

import cpuperformanceraytracer_amd as pt  # noqa: E402
from cpuperformanceraytracer_amd import _native as N  # noqa: E402

B = 8
MODES = {"none": N.PT_V4_ENV_NONE, "equirect": N.PT_V4_ENV_EQUIRECT, "cubemap": N.PT_V4_ENV_CUBEMAP}
LAST = (1 << 24) - 1   # the largest first frame pt_v4_render_device admits for 1 frame


def _pattern(nviews, nrows, w):
    """A start accumulator no render produces by chance: a displayable image (positive, finite) whose neighbouring
    elements all differ."""
    n = nviews * nrows * w * 3
    return ((np.arange(n, dtype=np.float32) % 251.0) * np.float32(0.0173) + np.float32(0.01)).reshape(nviews, nrows, w, 3)


@functools.lru_cache(maxsize=None)
def _ref(scene, cam, tex, w, h, frame_first, frames, start=None, accumulate=True, rows=(), fast_exp=True):
    """The camera oracle's accumulator after frames [frame_first, +frames) of `scene` (S0: InitializeScene's)
    seen by `cam` under texture `tex` (None: the ambient), begun from `start` (bytes of nrows x w x 3 f32; None:
    zeros).  0 frames: `start` itself.  Computed once per case, shared, read-only."""
    r = dict(rows)
    nrows = r.get("nrows", h)
    a = np.zeros((nrows, w, 3), np.float32) if start is None else np.frombuffer(start, np.float32).reshape(nrows, w, 3).copy()
    if frames > 0:
        omode = po.ENV_NONE if tex is None else po.ENV_CUBEMAP if tex in CUBEMAP else po.ENV_EQUIRECT
        sc = None if scene == "S0" else vo.oracle_scene(*SCENES[scene])
        vo.set_camera(*_camera(cam))
        p = po.Params4(w, h, r.get("row_start", 0), r.get("row_stride", 1), nrows, frame_first, frames, B, omode, 1, 1, None,
                       min(os.cpu_count() or 1, 16), int(not accumulate), int(not fast_exp))
        keep = None
        if tex is not None:
            keep = po.Env(TEX[tex].ctypes.data, TEX[tex].shape[1], TEX[tex].shape[0])
            p.env = ctypes.pointer(keep)
        assert vo.load().pto4_render(a.ctypes.data, ctypes.byref(p), ctypes.byref(sc) if sc is not None else None, None) == 0
    a.setflags(write=False)
    return a


@pytest.fixture
def lib(monkeypatch):
    """The library initialised under the case's switches (pt_init reads them), with NO process-wide env map
    unless the case sets one; the default camera, scene and config again, every set closed, and released, after."""
    sets = []

    def init(mode="equirect", grid=None, **cfg):
        monkeypatch.delenv(GRID_KNOB, raising=False)
        if grid is not None:
            monkeypatch.setenv(GRID_KNOB, str(grid))
        pt.init(num_bounces=B)
        pt.v4_config(env_mode=MODES[mode], num_bounces=B, **cfg)

        def make(names):
            from cpuperformanceraytracer_amd.device import make_v4_env_set
            sets.append(make_v4_env_set([TEX[n] for n in names]))
            return sets[-1]
        return make
    yield init
    for s in sets:
        s.close()
    pt.set_env_map(None)
    pt.v4_camera()
    pt.InitializeScene()
    pt.v4_config()
    pt.shutdown()
    monkeypatch.delenv(GRID_KNOB, raising=False)


def _render(views, w, h, frames, *, envs=None, names=None, scenes=None, buf=None, start=None, nrows=None, **kw):
    """views: (scene name, camera name, texture name or None) per view; `frames`: (frame_first, nframes) per view or
    None; `names`: the set's texture names (the mapping is made from the views); `scenes`: scene names, or None for
    the current scene.  The accumulator begins as `start` (nviews x nrows x w x 3) or zeros."""
    import torch
    from cpuperformanceraytracer_amd.device import render_v4_device_batch
    nr = h if nrows is None else nrows
    if buf is None:
        buf = torch.zeros((len(views), nr, w, 3), dtype=torch.float32, device="cuda:0")
        if start is not None:
            buf.copy_(torch.from_numpy(np.ascontiguousarray(start)))
    render_v4_device_batch(buf, [_camera(c) for _, c, _ in views], w, h, frames=frames, envs=envs,
                           env_of_view=None if envs is None else [names.index(t) for _, _, t in views],
                           scenes=None if scenes is None else [_scene(s) for s in scenes],
                           scene_of_view=None if scenes is None else [scenes.index(s) for s, _, _ in views],
                           num_bounces=B, nrows=nrows, **kw)
    return buf


def _slices(buf, nviews, w, nrows, planar=False):
    import torch
    torch.cuda.synchronize()
    a = buf.cpu().numpy().reshape(nviews, nrows * w * 3)
    return [planar8_to_interleaved(a[v], w, nrows) if planar else a[v].reshape(nrows, w, 3) for v in range(nviews)]


def _same_bits(got, want, what=""):
    assert bits_equal(got, want), f"{what}: {mismatch_report(got, want)}"


def _expected(views, w, h, frames, start=None, **ref):
    return [_ref(s, c, t, w, h, ff, n, None if start is None else np.ascontiguousarray(start[v]).tobytes(), **ref)
            for v, ((s, c, t), (ff, n)) in enumerate(zip(views, frames))]


def _check(buf, views, w, h, frames, start=None, planar=False, nrows=None, **ref):
    """Every slice against the oracle over that view's own range; returns the expected slices."""
    from cpuperformanceraytracer_amd.device import check_device_errors
    got = _slices(buf, len(views), w, h if nrows is None else nrows, planar)
    check_device_errors()
    want = _expected(views, w, h, frames, start, **ref)
    for v, (view, fr) in enumerate(zip(views, frames)):
        _same_bits(got[v], want[v], f"view {v} {view}, frames {fr}")
    return want


def _check_pixels(pix, want, fmt=N.PT_PIXEL_RGBA8, fast_aces=True, fast_gamma=True):
    """Each pixel slice is the oracle's output stage on the expected accumulator slice."""
    got = pix.cpu().numpy().view(np.uint32)
    for v, a in enumerate(want):
        w = po.tonemap(a, fmt, fast_aces, fast_gamma)
        assert np.array_equal(got[v], w), f"view {v}: {int((got[v] != w).sum())} pixels differ"


# ---- 1, 2. a wave crosses ranges ----------------------------------------------------------------------------
CROSS_FRAMES = [(1, 9), (100, 1), (5, 0), (2, 17), (1, 8), (1, 0), (33, 7), (LAST, 1)]
CROSS_NAMES = ["e3x5", "e32a"]   # two textures
CROSS_SCENES = ["S1", "S2"]      # two scenes
CROSS_VIEWS = [("S1", "A", "e32a"), ("S2", "D", "e3x5"), ("S1", "B", "e3x5"), ("S2", "D", "e32a"), ("S1", "C", "e3x5"),
               ("S2", "D", "e32a"), ("S1", "default", "e32a"), ("S2", "D", "e3x5")]   # D: no sky window


def _crossing(lib, accumulate):
    import torch
    make = lib(grid=1, accumulate_frames=accumulate)
    w, h = 24, 16
    assert len(CROSS_VIEWS) * 6 == 48 > 4 * 4   # more entries than the one block has waves: every wave crosses views
    start = _pattern(len(CROSS_VIEWS), h, w)   # (accumulating views blend into it, as the oracle does from the same start)
    pix = torch.full((len(CROSS_VIEWS), h, w), 0x12345678, dtype=torch.int32, device="cuda:0")
    buf = _render(CROSS_VIEWS, w, h, CROSS_FRAMES, envs=make(CROSS_NAMES), names=CROSS_NAMES, scenes=CROSS_SCENES, start=start,
                  pixels=pix)
    want = _check(buf, CROSS_VIEWS, w, h, CROSS_FRAMES, start=start, accumulate=bool(accumulate))
    for v in (2, 5):   # 0 frames: the pattern, bit for bit
        _same_bits(want[v], start[v], f"the oracle of view {v}")
    _check_pixels(pix, want)


def test_a_wave_crosses_ranges(lib):
    """8 views of 24 x 16 (6 tiles each, 48 entries) on a grid of ONE block (the knob): its four waves are on
    different views -- so different ranges -- at once, and each goes through counts 9, 1, 0, 17, 8, 0, 7, 1 with first
    frames 1, 100, 5, 2, 1, 1, 33 and 2^24 - 1.  Cameras with and without a sky window, two scenes, two textures;
    every slice and every pixel slice is compared; the 0-frame slices hold a pattern and come back bit-equal."""
    _crossing(lib, 1)


def test_a_wave_crosses_ranges_without_accumulation(lib):
    """accumulate_frames 0 stores the last frame's colour -- and loads nothing, so the 0-frame slice is the one the
    body would overwrite with zeros: it must be unchanged and its pixels packed from it.  Every slice begins as
    the pattern, which the rendered views overwrite."""
    _crossing(lib, 0)


# ---- 3. progressive: one view restarts while the others continue ---------------------------------------------------
def test_progressive_restart_of_one_view(lib):
    import torch
    make = lib()
    names = ["e3x5", "e32a", "e64"]
    views = [("S0", "A", "e32a"), ("S0", "B", "e3x5"), ("S0", "C", "e64")]
    w, h = 24, 16
    envs = make(names)
    first = [(1, 8)] * 3
    buf = _render(views, w, h, first, envs=envs, names=names)
    after1 = _check(buf, views, w, h, first)
    # view 0 continues, view 1 is zeroed by the caller and restarts, view 2 rests
    buf[1].zero_()
    second = [(9, 4), (1, 8), (9, 0)]
    pix = torch.zeros((3, h, w), dtype=torch.int32, device="cuda:0")
    _render(views, w, h, second, envs=envs, names=names, buf=buf, pixels=pix)
    start = np.stack([after1[0], np.zeros_like(after1[1]), after1[2]])
    want = _check(buf, views, w, h, second, start=start)
    _same_bits(want[0], _ref("S0", "A", "e32a", w, h, 1, 12), "8 + 4 frames are 12 frames")
    _same_bits(want[1], after1[1], "a restarted view repeats its first 8 frames")
    _check_pixels(pix, want)


# ---- 4. frames=None is the envs / scenes call --------------------------------------------------------------------
def test_no_ranges_equals_the_envs_and_scenes_calls(lib):
    """GPU against GPU, bit for bit: the batch call with frames=None against render_v4_device_envs, and (one
    process-wide map) against render_v4_device_scenes, on the same inputs; and against the oracle."""
    import torch
    from cpuperformanceraytracer_amd.device import render_v4_device_envs, render_v4_device_scenes
    make = lib()
    names = ["e2x2", "e32b"]
    scenes = ["S1", "S4"]
    views = [("S1", "A", "e32b"), ("S4", "D", "e2x2"), ("S1", "B", "e2x2")]
    w, h, ff, n = 20, 12, 3, 9
    envs = make(names)
    cams = [_camera(c) for _, c, _ in views]
    smap, emap = [scenes.index(s) for s, _, _ in views], [names.index(t) for _, _, t in views]
    a = _render(views, w, h, None, envs=envs, names=names, scenes=scenes, frame_first=ff, nframes=n)
    _check(a, views, w, h, [(ff, n)] * 3)
    b = torch.zeros_like(a)
    render_v4_device_envs(b, envs, cams, w, h, emap, [_scene(s) for s in scenes], smap, frame_first=ff, nframes=n, num_bounces=B)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "batch (frames=None) != envs call"
    # one shared map: envs=None reads pt_set_env_map's texture, as the scenes call does
    pt.set_env_map(TEX["e3x5"])
    shared = [(s, c, "e3x5") for s, c, _ in views]
    a = _render(shared, w, h, None, scenes=scenes, use_env=True, frame_first=ff, nframes=n)
    _check(a, shared, w, h, [(ff, n)] * 3)
    b = torch.zeros_like(a)
    render_v4_device_scenes(b, [_scene(s) for s in scenes], cams, w, h, smap, frame_first=ff, nframes=n, num_bounces=B, use_env=True)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "batch (frames=None, envs=None) != scenes call"


# ---- 5. envs=None with a process-wide map -----------------------------------------------------------------------
def test_process_wide_map_is_read_and_left_alone(lib):
    import torch
    from cpuperformanceraytracer_amd.device import render_v4_device
    lib()
    w = h = 16
    pt.set_env_map(TEX["e32a"])
    pt.v4_camera(*_camera("C"))
    kw = dict(frame_first=1, nframes=3, num_bounces=B, use_env=True)
    before = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    render_v4_device(before, w, h, **kw)
    state = (pt.v4_get_camera(), pt.v4_get_frame())
    views = [("S0", "A", "e32a"), ("S0", "D", "e32a"), ("S0", "B", "e32a")]
    frames = [(4, 9), (1, 0), (70, 1)]
    _check(_render(views, w, h, frames, use_env=True), views, w, h, frames)
    assert (pt.v4_get_camera(), pt.v4_get_frame()) == state
    after = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    render_v4_device(after, w, h, **kw)
    torch.cuda.synchronize()
    assert torch.equal(after.view(torch.int32), before.view(torch.int32)), "the process-wide map or camera changed"
    _same_bits(after.cpu().numpy(), _ref("S0", "C", "e32a", w, h, 1, 3), "pt_v4_render_device after the batch call")
    # without use_env the same call renders the ambient, map or no map
    amb = [(s, c, None) for s, c, _ in views]
    _check(_render(amb, w, h, frames, use_env=False), amb, w, h, frames)


# ---- 6. every instance ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast_exp", [1, 0])
@pytest.mark.parametrize("layout", ["interleaved", "planar8"])
@pytest.mark.parametrize("mode", ["none", "equirect", "cubemap"])
def test_instance_matrix(lib, mode, layout, fast_exp):
    """Every compiled instance on two views of 20 x 12 (ragged tiles in both directions; planar8 needs width % 8 ==
    0: 24 x 12) with ranges (3, 9) and (1, 1); S2's refractive sphere absorbs: the exp branch."""
    make = lib(mode=mode, fast_exp=fast_exp)
    names = None if mode == "none" else list(EQUIRECT if mode == "equirect" else CUBEMAP)[1:3]
    views = [("S1", "A", names[1] if names else None), ("S2", "B", names[0] if names else None)]
    planar = layout == "planar8"
    w, h = (24 if planar else 20), 12
    frames = [(3, 9), (1, 1)]
    buf = _render(views, w, h, frames, envs=make(names) if names else None, names=names, scenes=["S1", "S2"],
                  layout=N.PT_LAYOUT_PLANAR8 if planar else N.PT_LAYOUT_INTERLEAVED)
    _check(buf, views, w, h, frames, planar=planar, fast_exp=bool(fast_exp))


def test_second_pass_pixels_with_a_resting_view(lib):
    """A tonemap pair other than the default: the pixels come from the second pass over all slices, with a view of
    0 frames in the batch -- its pixels are those of its untouched accumulator."""
    import torch
    make = lib(fast_aces=0, fast_gamma=0)
    names = ["e3x5", "e32a"]
    views = [("S0", "A", "e32a"), ("S0", "B", "e3x5"), ("S0", "D", "e32a")]
    w, h = 20, 12
    frames = [(3, 9), (9, 0), (1, 1)]
    start = _pattern(3, h, w)
    pix = torch.zeros((3, h, w), dtype=torch.int32, device="cuda:0")
    buf = _render(views, w, h, frames, envs=make(names), names=names, start=start, pixels=pix, pixel_format=N.PT_PIXEL_XRGB8)
    want = _check(buf, views, w, h, frames, start=start)
    _check_pixels(pix, want, N.PT_PIXEL_XRGB8, False, False)


# ---- 7. partial rows ----------------------------------------------------------------------------------------------
def test_row_shard_with_ranges(lib):
    make = lib()
    rows = dict(row_start=1, row_stride=2, nrows=8)   # rows 1, 3, .. 15 of 16
    names = ["e3x5", "e64"]
    views = [("S1", "B", "e3x5"), ("S2", "A", "e64"), ("S1", "D", "e64")]
    frames = [(999_990, 3), (1, 0), (7, 9)]
    buf = _render(views, 24, 16, frames, envs=make(names), names=names, scenes=["S1", "S2"], **rows)
    _check(buf, views, 24, 16, frames, nrows=8, rows=tuple(rows.items()))


# ---- 8. the four calls share one staging ring ---------------------------------------------------------------------
VIEW_RING = 4   # pt_capi.cpp kViewRing: the slots of the ring the views, scenes, envs and batch calls stage through


def test_interleaved_kinds_share_the_staging_ring(lib):
    """kViewRing + 2 batched calls back to back on one stream, no synchronisation between them, cycling through the
    views, scenes and batch calls (no env term is configured, so no envs call): the fifth and sixth reuse the
    slots of the first and second, which another KIND filled -- a block of another layout.  Each call has its own
    accumulator and its own pair of cameras, so a slot rewritten while its launch still read it, or a table read
    at another kind's offsets, shows as another image.  After one synchronisation each accumulator equals, bit for
    bit, the same call issued alone on a fresh accumulator (GPU against GPU; the oracle has the other tests)."""
    import torch
    from cpuperformanceraytracer_amd.device import render_v4_device_batch, render_v4_device_scenes, render_v4_device_views
    lib(mode="none")
    w, h, nv = 24, 16, 2
    kw = dict(frame_first=1, nframes=2, num_bounces=B)
    two = [_scene("S1"), _scene("S2")]
    kinds = [lambda buf, cams: render_v4_device_views(buf, cams, w, h, **kw),
             lambda buf, cams: render_v4_device_scenes(buf, two, cams, w, h, **kw),
             lambda buf, cams: render_v4_device_batch(buf, cams, w, h, frames=[(1, 2), (1, 2)], scenes=two, scene_of_view=[0, 1],
                                                      num_bounces=B)]
    pairs = [("A", "B"), ("C", "D"), ("default", "A"), ("B", "C"), ("D", "default"), ("A", "C")]
    assert len(pairs) == VIEW_RING + 2 and all(pairs[i] != pairs[i - VIEW_RING] for i in range(VIEW_RING, len(pairs)))
    calls = [(kinds[i % len(kinds)], [_camera(c) for c in pair]) for i, pair in enumerate(pairs)]
    together = [torch.zeros((nv, h, w, 3), dtype=torch.float32, device="cuda:0") for _ in calls]
    alone = [torch.zeros_like(t) for t in together]
    torch.cuda.synchronize()
    for (call, cams), buf in zip(calls, together):
        call(buf, cams)
    torch.cuda.synchronize()
    for (call, cams), buf in zip(calls, alone):
        call(buf, cams)
        torch.cuda.synchronize()
    from cpuperformanceraytracer_amd.device import check_device_errors
    check_device_errors()
    for i, (t, a) in enumerate(zip(together, alone)):
        assert bool((a != 0).any()), f"call {i} rendered nothing"
        assert torch.equal(t.view(torch.int32), a.view(torch.int32)), f"call {i} ({pairs[i]}): back to back != alone"
    assert not torch.equal(together[0].view(torch.int32), together[3].view(torch.int32)), "two views calls, other cameras"


def test_views_call_with_use_env_and_no_env_term_is_a_state_error(lib):
    """The views call keeps its own rule on the shared host path: use_env under env mode NONE is PT_ESTATE (the
    batch call renders the ambient there, the envs call says PT_EINVAL).  Code and text as the views call reported
    them when it still had a body of its own (recorded from that revision's library); nothing is written."""
    import torch
    from cpuperformanceraytracer_amd.device import render_v4_device_views
    lib(mode="none")
    buf = torch.full((1, 8, 8, 3), 7.0, dtype=torch.float32, device="cuda:0")
    with pytest.raises(N.PtError) as e:
        render_v4_device_views(buf, [_camera("A")], 8, 8, frame_first=1, nframes=2, num_bounces=B, use_env=True)
    assert e.value.code == N.PT_ESTATE and "use_env with v4 env mode NONE" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all()), "a rejected call wrote the buffer"


# ---- 9. what is rejected (with a live set: the checks a CPU cannot reach) ---------------------------------------------
def test_rejected_with_a_live_set(lib):
    import torch
    make = lib()
    names = ["e2x2", "e3x5"]
    envs = make(names)
    views = [("S0", "A", "e2x2"), ("S0", "B", "e3x5")]
    buf = torch.full((2, 8, 8, 3), 7.0, dtype=torch.float32, device="cuda:0")

    def rejected(frames=((1, 2), (1, 2)), **kw):
        with pytest.raises(N.PtError) as e:
            _render(views, 8, 8, list(frames), envs=envs, names=names, buf=buf, **kw)
        assert e.value.code == N.PT_EINVAL, str(e.value)
        return str(e.value)
    assert "env term" in rejected(use_env=False)
    pt.v4_config(env_mode=N.PT_V4_ENV_NONE, num_bounces=B)
    assert "env term" in rejected()
    pt.v4_config(env_mode=N.PT_V4_ENV_EQUIRECT, num_bounces=B)
    assert "view 1" in rejected(frames=((1, 2), (0, 2)))
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all()), "a rejected call wrote the buffer"
