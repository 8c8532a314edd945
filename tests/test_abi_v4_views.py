"""pt_v4_render_device_views at the drop-in boundary: exported, bound, and every argument check fires
before any GPU work -- so none of this needs a GPU.  The accumulator pointer is a made-up non-null
address: a rejected call and a call with nothing to render never touch it."""
from __future__ import annotations

import ctypes
import subprocess

import pytest

NAME = "pt_v4_render_device_views"
FAKE_BUF = 0x1000   # never dereferenced


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


def _job(N, width=256, height=144, nrows=144, nframes=8, **kw):
    f = dict(buf=FAKE_BUF, width=width, height=height, row_start=0, row_stride=1, nrows=nrows, layout=N.PT_LAYOUT_INTERLEAVED,
             frame_first=1, nframes=nframes, num_bounces=8, use_env=0)
    f.update(kw)
    return N.PtDeviceJob(*[f[k] for k, _ in N.PtDeviceJob._fields_])


def _cams(N, cams):
    return (N.PtV4Camera * len(cams))(*[N.PtV4Camera((ctypes.c_float * 3)(*p), fov) for p, fov in cams])


def _call(N, job, cams, nviews=None, pixels=None, fmt=0):
    arr = _cams(N, cams) if cams is not None else None
    n = len(cams) if nviews is None else nviews
    rc = N.load().pt_v4_render_device_views(ctypes.byref(job), arr, n, pixels, fmt, None)
    return rc, N.load().pt_last_error().decode()


def _get_camera(N):
    c, d = N.PtV4Camera(), ctypes.c_float()
    assert N.load().pt_v4_get_camera(ctypes.byref(c), ctypes.byref(d)) == N.PT_OK
    return tuple(c.position), c.fov_degrees, d.value


CAM = ((0.0, 0.0, 40.0), 90.0)


def test_symbol_is_exported(lib_path):
    assert hasattr(ctypes.CDLL(str(lib_path)), NAME)


def test_prototype_is_bound(N):
    assert NAME in N.EXPORTED_SYMBOLS and N.PT_V4_MAX_VIEWS == 1024
    fn = getattr(N.load(), NAME)
    assert fn.restype is ctypes.c_int32
    assert list(fn.argtypes) == [ctypes.POINTER(N.PtDeviceJob), ctypes.POINTER(N.PtV4Camera), ctypes.c_int32,
                                 ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]


def test_python_entry_point_exists():
    import inspect

    from cpuperformanceraytracer_amd import device
    p = inspect.signature(device.render_v4_device_views).parameters
    assert list(p)[:4] == ["buf", "cameras", "width", "height"]
    for k in ("frame_first", "nframes", "num_bounces", "row_start", "row_stride", "nrows", "layout", "use_env", "pixels",
              "pixel_format", "stream"):
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert p["num_bounces"].default == 8 and p["pixels"].default is None


def test_null_cameras(N):
    rc, msg = _call(N, _job(N), None, nviews=2)
    assert rc == N.PT_EINVAL and "camera" in msg


@pytest.mark.parametrize("nviews", [0, -1, 1025])
def test_view_count_out_of_range(N, nviews):
    rc, msg = _call(N, _job(N), [CAM], nviews=nviews)
    assert rc == N.PT_EINVAL and "nviews" in msg


def test_tile_entries_out_of_range(N):
    """1024 views of 16384 x 8192 pixels are 2^31 tile entries; a queue entry carries 30 bits.  One tile
    row fewer per view than the limit allows (8192 x 8184: 1024 x 1047552 entries) passes that check --
    with nothing to render, so no GPU is needed to see it pass."""
    cams = [CAM] * 1024
    rc, msg = _call(N, _job(N, width=16384, height=8192, nrows=8192), cams)
    assert rc == N.PT_EINVAL and "tile" in msg
    rc, msg = _call(N, _job(N, width=8192, height=8184, nrows=8184, nframes=0), cams)
    assert rc == N.PT_OK, msg
    rc, msg = _call(N, _job(N, width=8192, height=8192, nrows=8192, nframes=0), cams)   # 1024 x 2^20 = 2^30 > 2^30 - 1
    assert rc == N.PT_EINVAL and "tile" in msg


def test_unknown_pixel_format(N):
    rc, msg = _call(N, _job(N), [CAM], pixels=ctypes.c_void_p(0x2000), fmt=7)
    assert rc == N.PT_EINVAL and "format" in msg
    rc, msg = _call(N, _job(N, nframes=0), [CAM], pixels=None, fmt=7)   # no pixels: the format is not looked at
    assert rc == N.PT_OK, msg


def test_invalid_job(N):
    rc, _ = _call(N, _job(N, buf=None), [CAM])
    assert rc == N.PT_EINVAL
    rc, _ = _call(N, _job(N, layout=N.PT_LAYOUT_TILED_PLANAR8), [CAM])
    assert rc == N.PT_EINVAL
    assert N.load().pt_v4_render_device_views(None, _cams(N, [CAM]), 1, None, 0, None) == N.PT_EINVAL


def test_the_first_failing_check_is_reported(N):
    """Calls that break two rules at once name the earlier one: job, camera array, view count, pixel format, tile
    entries, each camera, and only then "nothing to render" (which use_env does not disturb).  Codes and texts as
    the call reported them when it still had a body of its own (recorded from that revision's library)."""
    pix = ctypes.c_void_p(0x2000)
    huge = dict(width=16384, height=8192, nrows=8192)
    bad = ((0.0, 0.0, 40.0), 180.0)
    assert _call(N, _job(N, buf=None), None, nviews=0) == (N.PT_EINVAL, "null device job/buffer")
    assert _call(N, _job(N), None, nviews=0) == (N.PT_EINVAL, "null camera array")
    assert _call(N, _job(N), [CAM], nviews=0, pixels=pix, fmt=7) == (N.PT_EINVAL, "nviews 0 outside [1, 1024]")
    assert _call(N, _job(N, **huge), [CAM] * 1024, pixels=pix, fmt=7) == (N.PT_EINVAL, "unknown pixel format 7")
    assert _call(N, _job(N, **huge), [bad] * 1024) == (N.PT_EINVAL, "1024 views x 2097152 tiles exceed the tile queue's 1073741823 entries")
    assert _call(N, _job(N, nframes=0), [CAM, bad]) == (N.PT_EINVAL, "view 1: fov_degrees 180 outside (0, 180)")
    assert _call(N, _job(N, frame_first=0), [CAM]) == (N.PT_EINVAL, "frame range [0, +8) invalid")
    assert _call(N, _job(N, nframes=0, use_env=1), [CAM])[0] == N.PT_OK
    assert _call(N, _job(N, nrows=0, use_env=1), [CAM])[0] == N.PT_OK


def test_a_rejected_view_is_named_and_the_global_camera_is_untouched(N):
    before = _get_camera(N)
    cams = [CAM, ((3.0, -2.0, 30.0), 60.0), ((0.0, 0.0, 40.0), 180.0), CAM]
    rc, msg = _call(N, _job(N), cams)
    assert rc == N.PT_EINVAL and "view 2" in msg and "fov" in msg, msg
    assert _get_camera(N) == before
    rc, msg = _call(N, _job(N), [CAM, ((0.0, float("nan"), 1.0), 90.0)])
    assert rc == N.PT_EINVAL and "view 1" in msg, msg
    assert _get_camera(N) == before


def test_nothing_to_render_is_ok_and_leaves_the_global_camera(N):
    before = _get_camera(N)
    frame = N.load().pt_v4_get_frame()
    rc, msg = _call(N, _job(N, nframes=0), [((3.0, -2.0, 30.0), 60.0), ((0.0, -6.0, 22.0), 75.0)])
    assert rc == N.PT_OK, msg
    assert _get_camera(N) == before and N.load().pt_v4_get_frame() == frame
