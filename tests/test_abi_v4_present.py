"""pt_v4_render_device_present at the drop-in boundary: exported by libpt_mi355.so, declared in
include/pt_mi355.h and bound in _native.py with pt_render_device_present's prototype.  No GPU needed:
no compute call is made."""
from __future__ import annotations

import ctypes
import subprocess

import pytest

NAME = "pt_v4_render_device_present"


@pytest.fixture(scope="module")
def lib_path():
    from cpuperformanceraytracer_amd import build
    try:
        return build.build_lib()
    except (RuntimeError, subprocess.CalledProcessError) as e:   # pragma: no cover - toolchain missing
        pytest.skip(f"cannot build libpt_mi355.so: {e}")


def test_symbol_is_exported(lib_path):
    assert hasattr(ctypes.CDLL(str(lib_path)), NAME)


def test_prototype_is_bound(lib_path):
    from cpuperformanceraytracer_amd import _native as N
    assert NAME in N.EXPORTED_SYMBOLS
    fn, twin = getattr(N.load(), NAME), N.load().pt_render_device_present
    assert fn.restype is ctypes.c_int32
    assert list(fn.argtypes) == [ctypes.POINTER(N.PtDeviceJob), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    assert list(fn.argtypes) == list(twin.argtypes) and fn.restype is twin.restype


def test_python_entry_point_exists():
    import inspect

    from cpuperformanceraytracer_amd import device
    p = inspect.signature(device.render_v4_device_present).parameters
    assert list(p)[:4] == ["buf", "pixels", "width", "height"]
    for k in ("frame_first", "nframes", "num_bounces", "row_start", "row_stride", "nrows", "layout", "use_env",
              "pixel_format", "stream"):
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert p["num_bounces"].default == 8
