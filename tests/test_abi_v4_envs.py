"""pt_v4_make_env_set, pt_v4_free_env_set and pt_v4_render_device_envs at the drop-in boundary: exported,
bound, every argument check of the set fired before any GPU work with *out untouched, and the process-wide
scene, camera and frame counter untouched by rejected calls -- none of this needs a GPU.  The accumulator
pointer is a made-up non-null address: a rejected call never touches it."""
from __future__ import annotations

import ctypes
import subprocess

import numpy as np
import pytest

NAMES = ("pt_v4_make_env_set", "pt_v4_free_env_set", "pt_v4_render_device_envs")
FAKE_BUF = 0x1000   # never dereferenced
CAM = ((0.0, 0.0, 40.0), 90.0)
UNTOUCHED = 0x5a5a5a5a   # *out before every rejected pt_v4_make_env_set


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
    f = dict(buf=FAKE_BUF, width=256, height=144, row_start=0, row_stride=1, nrows=144, layout=N.PT_LAYOUT_INTERLEAVED,
             frame_first=1, nframes=8, num_bounces=8, use_env=1)
    f.update(kw)
    return N.PtDeviceJob(*[f[k] for k, _ in N.PtDeviceJob._fields_])


def _texs(N, n, keep):
    """n valid 2 x 2 textures (their arrays appended to `keep`)."""
    arr = (N.PtTexture * n)()
    for i in range(n):
        a = np.full((2, 2, 3), 0.5, np.float32)
        keep.append(a)
        arr[i] = N.PtTexture(a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 2, 2, 3)
    return arr


def _make(N, texs, n, out="fresh"):
    """(rc, message, *out afterwards) of pt_v4_make_env_set."""
    o = ctypes.c_void_p(UNTOUCHED)
    rc = N.load().pt_v4_make_env_set(texs, n, ctypes.byref(o) if out == "fresh" else out)
    return rc, N.load().pt_last_error().decode(), o.value


def _state(N):
    """(scene tables, camera, frame counter, initialised device) of the process."""
    L = N.load()
    nq, ns = ctypes.c_int32(), ctypes.c_int32()
    need = L.pt_v4_get_scene_tables(None, 0, ctypes.byref(nq), ctypes.byref(ns))
    assert need > 0
    t = np.zeros(need, np.float32)
    assert L.pt_v4_get_scene_tables(t.ctypes.data, need, ctypes.byref(nq), ctypes.byref(ns)) == need
    c, d = N.PtV4Camera(), ctypes.c_float()
    assert L.pt_v4_get_camera(ctypes.byref(c), ctypes.byref(d)) == N.PT_OK
    return t.tobytes(), nq.value, ns.value, tuple(c.position), c.fov_degrees, d.value, L.pt_v4_get_frame(), L.pt_initialized_device()


def _render_null_set(N, job=None, nviews=1):
    cams = (N.PtV4Camera * nviews)(*[N.PtV4Camera((ctypes.c_float * 3)(*CAM[0]), CAM[1]) for _ in range(nviews)])
    rc = N.load().pt_v4_render_device_envs(ctypes.byref(job if job is not None else _job(N)), None, None, None, 0, None, cams,
                                           nviews, None, 0, None)
    return rc, N.load().pt_last_error().decode()


# ---- the boundary ------------------------------------------------------------------------------------------
def test_symbols_are_exported(lib_path):
    L = ctypes.CDLL(str(lib_path))
    for name in NAMES:
        assert hasattr(L, name), name


def test_prototypes_are_bound(N):
    for name in NAMES:
        assert name in N.EXPORTED_SYMBOLS
    L = N.load()
    i32, vp = ctypes.c_int32, ctypes.c_void_p
    assert L.pt_v4_make_env_set.restype is i32
    assert list(L.pt_v4_make_env_set.argtypes) == [ctypes.POINTER(N.PtTexture), i32, ctypes.POINTER(vp)]
    assert L.pt_v4_free_env_set.restype is None and list(L.pt_v4_free_env_set.argtypes) == [vp]
    assert L.pt_v4_render_device_envs.restype is i32
    assert list(L.pt_v4_render_device_envs.argtypes) == [ctypes.POINTER(N.PtDeviceJob), vp, ctypes.POINTER(i32),
                                                         ctypes.POINTER(N.PtV4SceneDesc), i32, ctypes.POINTER(i32),
                                                         ctypes.POINTER(N.PtV4Camera), i32, vp, i32, vp]


def test_python_entry_points_exist():
    import inspect

    from cpuperformanceraytracer_amd import device
    p = inspect.signature(device.render_v4_device_envs).parameters
    assert list(p)[:8] == ["buf", "envs", "cameras", "width", "height", "env_of_view", "scenes", "scene_of_view"]
    assert all(p[k].default is None for k in ("env_of_view", "scenes", "scene_of_view"))
    for k in ("frame_first", "nframes", "num_bounces", "row_start", "row_stride", "nrows", "layout", "use_env", "pixels",
              "pixel_format", "stream"):
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert callable(device.make_v4_env_set)


# ---- pt_v4_make_env_set: every rejection before any GPU work, *out untouched -----------------------------
def test_make_rejects_null_arguments(N):
    keep = []
    rc, msg, out = _make(N, None, 1)
    assert rc == N.PT_EINVAL and "texture" in msg and out == UNTOUCHED
    rc, msg, _ = _make(N, _texs(N, 1, keep), 1, out=None)
    assert rc == N.PT_EINVAL and "result" in msg


@pytest.mark.parametrize("n", [0, -1, 1025])
def test_make_rejects_a_count_out_of_range(N, n):
    keep = []
    assert N.PT_V4_MAX_VIEWS == 1024
    rc, msg, out = _make(N, _texs(N, 1025, keep), n)
    assert rc == N.PT_EINVAL and str(n) in msg and out == UNTOUCHED, msg


@pytest.mark.parametrize("field,value,word", [("data", None, "data"), ("width", 0, "size"), ("components", 4, "components")])
def test_make_names_the_bad_texture(N, field, value, word):
    keep = []
    texs = _texs(N, 5, keep)
    if field == "data":
        texs[3].data = ctypes.POINTER(ctypes.c_float)()
    else:
        setattr(texs[3], field, value)
    rc, msg, out = _make(N, texs, 5)
    assert rc == N.PT_EINVAL and "texture 3" in msg and word in msg and out == UNTOUCHED, msg


def test_free_null_is_harmless(N):
    N.load().pt_v4_free_env_set(None)
    N.load().pt_v4_free_env_set(None)


# ---- pt_v4_render_device_envs ------------------------------------------------------------------------------
def test_render_rejects_a_null_set(N):
    rc, msg = _render_null_set(N)
    assert rc == N.PT_EINVAL and "env set" in msg, msg
    # what the scenes call rejects is rejected here too: a job without a buffer, no views
    assert _render_null_set(N, _job(N, buf=None))[0] == N.PT_EINVAL
    rc, msg = _render_null_set(N, nviews=0)
    assert rc == N.PT_EINVAL and "nviews" in msg


def test_render_rejects_the_current_scene_with_scene_arguments(N):
    """scenes NULL means the current scene: nscenes must be 0 and scene_of_view NULL."""
    cams = (N.PtV4Camera * 1)(N.PtV4Camera((ctypes.c_float * 3)(*CAM[0]), CAM[1]))
    L = N.load()
    assert L.pt_v4_render_device_envs(ctypes.byref(_job(N)), None, None, None, 1, None, cams, 1, None, 0, None) == N.PT_EINVAL
    assert "nscenes" in L.pt_last_error().decode()
    m = (ctypes.c_int32 * 1)(0)
    assert L.pt_v4_render_device_envs(ctypes.byref(_job(N)), None, None, None, 0, m, cams, 1, None, 0, None) == N.PT_EINVAL
    assert "scene_of_view" in L.pt_last_error().decode()


def test_rejected_calls_leave_the_process_state_and_the_gpu_alone(N):
    L = N.load()
    assert L.pt_v4_initialize_scene() == N.PT_OK
    before = _state(N)
    keep = []
    assert _make(N, None, 1)[0] == N.PT_EINVAL
    assert _make(N, _texs(N, 1, keep), 0)[0] == N.PT_EINVAL
    bad = _texs(N, 2, keep)
    bad[1].height = 0
    assert _make(N, bad, 2)[0] == N.PT_EINVAL
    assert _render_null_set(N)[0] == N.PT_EINVAL
    assert _render_null_set(N, _job(N, nframes=0))[0] == N.PT_EINVAL   # (checked before the nothing-to-render shortcut)
    L.pt_v4_free_env_set(None)
    assert _state(N) == before
