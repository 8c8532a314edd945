"""pt_v4_render_device_batch at the drop-in boundary: exported, bound, the struct's layout as ctypes sees it,
and every argument check fired before any GPU work -- none of this needs a GPU.  The accumulator pointer is
a made-up non-null address: a rejected call, and a call with nothing to render, never touches it."""
from __future__ import annotations

import ctypes
import subprocess

import pytest

NAME = "pt_v4_render_device_batch"
FAKE_BUF = 0x1000   # never dereferenced
FAKE_SET = 0x2000   # never dereferenced: not a live env set
CAM = ((0.0, 0.0, 40.0), 90.0)
MAX_FRAME = 1 << 24   # frame_first + nframes may reach it, as in pt_v4_render_device


@pytest.fixture(scope="module")
def lib_path():
    from cpuperformanceraytracer_amd import build
    try:
        return build.build_lib()
    except (RuntimeError, subprocess.CalledProcessError) as e:   # pragma: no cover - toolchain missing
        pytest.skip(f"cannot build libpt_mi355.so: {e}")


@pytest.fixture
def N(lib_path):
    from cpuperformanceraytracer_amd import _native
    _native.load()
    return _native


def _job(N, **kw):
    f = dict(buf=FAKE_BUF, width=24, height=16, row_start=0, row_stride=1, nrows=16, layout=N.PT_LAYOUT_INTERLEAVED,
             frame_first=1, nframes=8, num_bounces=8, use_env=0)
    f.update(kw)
    return N.PtDeviceJob(*[f[k] for k, _ in N.PtDeviceJob._fields_])


def _call(N, job=None, *, nviews=3, frames=None, batch="make", **fields):
    """(rc, message) of one call; `frames`: (frame_first, nframes) per view, or None; `fields`: pt_v4_batch members."""
    keep = [(N.PtV4Camera * max(nviews, 1))(*[N.PtV4Camera((ctypes.c_float * 3)(*CAM[0]), CAM[1]) for _ in range(max(nviews, 1))])]
    b = N.PtV4Batch()
    b.cams, b.nviews = keep[0], nviews
    if frames is not None:
        keep.append((N.PtV4FrameRange * len(frames))(*[N.PtV4FrameRange(a, n) for a, n in frames]))
        b.frames = keep[-1]
    for k, v in fields.items():
        if isinstance(v, list):
            keep.append((ctypes.c_int32 * len(v))(*v))
            v = keep[-1]
        setattr(b, k, v)
    L = N.load()
    rc = L.pt_v4_render_device_batch(ctypes.byref(job if job is not None else _job(N)), ctypes.byref(b) if batch == "make" else batch,
                                     None)
    return rc, L.pt_last_error().decode()


# ---- the boundary ------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_bound(lib_path, N):
    assert hasattr(ctypes.CDLL(str(lib_path)), NAME)
    assert NAME in N.EXPORTED_SYMBOLS
    f = getattr(N.load(), NAME)
    assert f.restype is ctypes.c_int32
    assert list(f.argtypes) == [ctypes.POINTER(N.PtDeviceJob), ctypes.POINTER(N.PtV4Batch), ctypes.c_void_p]


def test_struct_layout(N):
    """The layout a C compiler gives pt_v4_batch / pt_v4_frame_range on LP64 (include/pt_mi355.h)."""
    r = N.PtV4FrameRange
    assert ctypes.sizeof(r) == 8 and (r.frame_first.offset, r.nframes.offset) == (0, 4)
    b = N.PtV4Batch
    want = {"cams": 0, "nviews": 8, "frames": 16, "scenes": 24, "nscenes": 32, "scene_of_view": 40, "envs": 48, "env_of_view": 56,
            "pixels": 64, "format": 72}
    assert [k for k, _ in b._fields_] == list(want)
    assert {k: getattr(b, k).offset for k in want} == want
    assert ctypes.sizeof(b) == 80


def test_python_entry_point_exists():
    import inspect

    from cpuperformanceraytracer_amd import device
    p = inspect.signature(device.render_v4_device_batch).parameters
    assert list(p)[:4] == ["buf", "cameras", "width", "height"]
    for k in ("frames", "scenes", "scene_of_view", "envs", "env_of_view", "pixels"):
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is None, k
    for k in ("num_bounces", "row_start", "row_stride", "nrows", "layout", "use_env", "pixel_format", "stream"):
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY, k


# ---- rejected before any GPU work ---------------------------------------------------------------------------
def test_null_batch_and_null_job(N):
    rc, msg = _call(N, batch=None)
    assert rc == N.PT_EINVAL and "batch" in msg, msg
    L = N.load()
    b = N.PtV4Batch()
    assert L.pt_v4_render_device_batch(None, ctypes.byref(b), None) == N.PT_EINVAL


def test_what_the_scenes_and_envs_calls_reject(N):
    assert _call(N, _job(N, buf=None))[0] == N.PT_EINVAL
    rc, msg = _call(N, nviews=0)
    assert rc == N.PT_EINVAL and "nviews" in msg, msg
    rc, msg = _call(N, cams=None)
    assert rc == N.PT_EINVAL and "camera" in msg, msg
    rc, msg = _call(N, pixels=0x3000, format=77)
    assert rc == N.PT_EINVAL and "format" in msg, msg
    rc, msg = _call(N, _job(N, frame_first=0))            # frames NULL: the job's own range is every view's
    assert rc == N.PT_EINVAL and "frame range" in msg, msg
    rc, msg = _call(N, _job(N, use_env=1), envs=FAKE_SET)   # not a live set
    assert rc == N.PT_EINVAL and "env set" in msg, msg


@pytest.mark.parametrize("bad,word", [((0, 1), "[0, +1)"), ((1, -1), "+-1)"), ((MAX_FRAME, 1), f"[{MAX_FRAME}, +1)"),
                                      ((MAX_FRAME - 7, 8), "+8)"), ((0xFFFFFFFF, 2), "+2)")])
@pytest.mark.parametrize("view", [0, 2])
def test_a_bad_range_names_its_view(N, bad, word, view):
    frames = [(1, 8), (5, 0), (3, 9)]
    frames[view] = bad
    rc, msg = _call(N, frames=frames)
    assert rc == N.PT_EINVAL and f"view {view}" in msg and word in msg, msg


def test_with_ranges_the_jobs_own_range_is_not_read(N):
    """frames given: a job range pt_v4_render_device would reject is ignored (every view has 0 frames: PT_OK)."""
    rc, msg = _call(N, _job(N, frame_first=0, nframes=-3), frames=[(1, 0)] * 3)
    assert rc == N.PT_OK, msg


def test_the_largest_ranges_are_accepted(N):
    """frame_first + nframes == 2^24 is what pt_v4_render_device admits; 0 frames everywhere: no launch, PT_OK."""
    rc, msg = _call(N, frames=[(MAX_FRAME, 0), (MAX_FRAME - 1, 0), (1, 0)])
    assert rc == N.PT_OK, msg


def test_envs_without_an_env_term(N):
    """envs != NULL without an env term (here use_env 0) is rejected as in the envs call.  The term is checked
    before the set is looked at, so the made-up handle is not the reason; a NULL set with use_env 0 is the
    ambient."""
    rc, msg = _call(N, _job(N, use_env=0), envs=FAKE_SET)
    assert rc == N.PT_EINVAL and "env term" in msg and "use_env 0" in msg, msg
    rc, msg = _call(N, _job(N, use_env=0), envs=FAKE_SET, env_of_view=[0, 0, 0], frames=[(1, 8)] * 3)
    assert rc == N.PT_EINVAL and "env term" in msg, msg
    rc, msg = _call(N, _job(N, use_env=0), frames=[(1, 0)] * 3)
    assert rc == N.PT_OK, msg


def test_current_scene_with_scene_arguments(N):
    rc, msg = _call(N, nscenes=1)
    assert rc == N.PT_EINVAL and "nscenes" in msg, msg
    rc, msg = _call(N, scene_of_view=[0, 0, 0])
    assert rc == N.PT_EINVAL and "scene_of_view" in msg, msg


def test_no_env_set_with_a_mapping(N):
    rc, msg = _call(N, env_of_view=[0, 0, 0])
    assert rc == N.PT_EINVAL and "env_of_view" in msg, msg
    rc, msg = _call(N, _job(N, use_env=1), env_of_view=[0, 0, 0])
    assert rc == N.PT_EINVAL and "env_of_view" in msg, msg


# ---- accepted, with nothing to render: PT_OK and no GPU work --------------------------------------------------
def test_null_frames_is_accepted(N):
    """frames NULL: the job's range for every view -- here 0 frames, then 0 rows: the whole-call shortcut."""
    before = N.load().pt_initialized_device()   # (-1 unless another test of this process left the library initialised)
    rc, msg = _call(N, _job(N, nframes=0))
    assert rc == N.PT_OK, msg
    rc, msg = _call(N, _job(N, nrows=0))
    assert rc == N.PT_OK, msg
    assert N.load().pt_initialized_device() == before, "the shortcut initialised a device"


def test_all_zero_frames_returns_ok_without_a_launch(N):
    before = N.load().pt_initialized_device()
    rc, msg = _call(N, frames=[(1, 0), (100, 0), (7, 0)])
    assert rc == N.PT_OK, msg
    rc, msg = _call(N, _job(N, nrows=0), frames=[(1, 8), (100, 1), (7, 17)])
    assert rc == N.PT_OK, msg
    assert N.load().pt_initialized_device() == before, "the shortcut initialised a device"
