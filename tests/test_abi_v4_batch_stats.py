"""pt_v4_render_device_batch_stats at the drop-in boundary: exported, bound, the record's layout as ctypes sees
it, and every argument check fired before any GPU work -- none of this needs a GPU.  The accumulator and the
statistics pointer are made-up non-null addresses: a rejected call never touches them."""
from __future__ import annotations

import ctypes
import subprocess

import pytest

NAME = "pt_v4_render_device_batch_stats"
FAKE_BUF = 0x1000     # never dereferenced
FAKE_STATS = 0x4000   # never dereferenced
CAM = ((0.0, 0.0, 40.0), 90.0)
MAX_FRAME = 1 << 24


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


def _call(N, job="make", *, nviews=3, frames=None, batch="make", stats=FAKE_STATS, **fields):
    """(rc, message) of one call; `frames`: (frame_first, nframes) per view, or None; `fields`: pt_v4_batch members."""
    keep = [(N.PtV4Camera * nviews)(*[N.PtV4Camera((ctypes.c_float * 3)(*CAM[0]), CAM[1]) for _ in range(nviews)])]
    b = N.PtV4Batch()
    b.cams, b.nviews = keep[0], nviews
    if frames is not None:
        keep.append((N.PtV4FrameRange * len(frames))(*[N.PtV4FrameRange(a, n) for a, n in frames]))
        b.frames = keep[-1]
    for k, v in fields.items():
        setattr(b, k, v)
    L = N.load()
    j = _job(N) if job == "make" else job
    rc = getattr(L, NAME)(ctypes.byref(j) if j is not None else None, ctypes.byref(b) if batch == "make" else batch, stats, None)
    return rc, L.pt_last_error().decode()


def test_symbol_is_exported_and_bound(lib_path, N):
    assert hasattr(ctypes.CDLL(str(lib_path)), NAME)
    assert NAME in N.EXPORTED_SYMBOLS
    f = getattr(N.load(), NAME)
    assert f.restype is ctypes.c_int32
    assert list(f.argtypes) == [ctypes.POINTER(N.PtDeviceJob), ctypes.POINTER(N.PtV4Batch), ctypes.c_void_p, ctypes.c_void_p]


def test_record_layout(N):
    """The layout a C compiler gives pt_v4_view_stats on LP64 (include/pt_mi355.h): 16 bytes, 0 / 8 / 12."""
    s = N.PtV4ViewStats
    assert ctypes.sizeof(s) == 16
    assert [k for k, _ in s._fields_] == ["sum_delta", "changed", "max_delta"]
    assert (s.sum_delta.offset, s.changed.offset, s.max_delta.offset) == (0, 8, 12)
    assert (s.sum_delta.size, s.changed.size, s.max_delta.size) == (8, 4, 4)


def test_the_batch_struct_is_unchanged(N):
    """The new call takes the pt_v4_batch existing callers build: 80 bytes, `format` last at 72."""
    assert ctypes.sizeof(N.PtV4Batch) == 80 and N.PtV4Batch.format.offset == 72


def test_python_entry_points_exist():
    import inspect

    from cpuperformanceraytracer_amd import device
    p = inspect.signature(device.render_v4_device_batch).parameters
    assert p["stats"].kind is inspect.Parameter.KEYWORD_ONLY and p["stats"].default is None
    a = inspect.signature(device.render_v4_adaptive).parameters
    assert list(a)[:4] == ["buf", "cameras", "width", "height"]
    assert a["max_frames"].kind is inspect.Parameter.KEYWORD_ONLY and a["max_frames"].default is inspect.Parameter.empty
    assert (a["frames_per_round"].default, a["tol"].default, a["patience"].default) == (8, 0, 1)
    doc = " ".join(device.render_v4_adaptive.__doc__.split())
    assert "display criterion, not a variance bound" in doc


def test_null_stats_null_job_null_batch(N):
    before = N.load().pt_initialized_device()
    rc, msg = _call(N, stats=None)
    assert rc == N.PT_EINVAL and "statistics" in msg, msg
    rc, msg = _call(N, stats=None, frames=[(1, 0)] * 3)   # also when nothing would render
    assert rc == N.PT_EINVAL and "statistics" in msg, msg
    rc, msg = _call(N, job=None)
    assert rc == N.PT_EINVAL and "device job" in msg, msg
    rc, msg = _call(N, batch=None)
    assert rc == N.PT_EINVAL and "batch" in msg, msg
    assert N.load().pt_initialized_device() == before, "a rejected call initialised a device"


def test_what_the_batch_call_rejects(N):
    before = N.load().pt_initialized_device()
    assert _call(N, _job(N, buf=None))[0] == N.PT_EINVAL
    rc, msg = _call(N, nviews=0, cams=None)
    assert rc == N.PT_EINVAL, msg
    rc, msg = _call(N, pixels=0x3000, format=77)
    assert rc == N.PT_EINVAL and "format" in msg, msg
    rc, msg = _call(N, _job(N, frame_first=0))
    assert rc == N.PT_EINVAL and "frame range" in msg, msg
    rc, msg = _call(N, nscenes=1)
    assert rc == N.PT_EINVAL and "nscenes" in msg, msg
    assert N.load().pt_initialized_device() == before, "a rejected call initialised a device"


@pytest.mark.parametrize("bad,word", [((0, 1), "[0, +1)"), ((1, -1), "+-1)"), ((MAX_FRAME, 1), f"[{MAX_FRAME}, +1)"),
                                      ((MAX_FRAME - 7, 8), "+8)")])
@pytest.mark.parametrize("view", [0, 2])
def test_a_bad_range_still_names_its_view(N, bad, word, view):
    frames = [(1, 8), (5, 0), (3, 9)]
    frames[view] = bad
    rc, msg = _call(N, frames=frames)
    assert rc == N.PT_EINVAL and f"view {view}" in msg and word in msg, msg
