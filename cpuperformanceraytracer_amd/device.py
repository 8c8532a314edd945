"""Device-resident rendering on torch tensors (HBM in, HBM out; the bench and multi-GPU path).

PyTorch is plumbing here: it owns the device allocation and the stream; the work is the HIP
kernel in libpt_mi355.so, reached through pt_render_device / pt_count_device.
"""
from __future__ import annotations

import ctypes

from . import _native as N


def ensure_backend(device_index: int, num_bounces: int = 4) -> None:
    """Initialise libpt_mi355 on `device_index` (the torch device of this rank) if it is not
    initialised yet.  The library state (env map, schedules, pinned buffer, frame counters) is per
    process; a device job runs on the logical device holding its buffer, and a job on a device the
    library was not initialised with raises PtError(PT_ESTATE) instead of silently re-initialising
    (renderer.init(devices=[...]) drives several GPUs from one process; bench.py and shard.py run one
    process per GPU).  The caller's current HIP device is restored after an initialisation."""
    from . import renderer
    cur = renderer.initialized_devices()
    if device_index in cur:
        return
    if cur:
        raise N.PtError(N.PT_ESTATE, "ensure_backend",
                        f"libpt_mi355 is initialised on devices {cur}; a job on device {device_index} needs "
                        "renderer.init(devices=[...]) naming it, or its own process")
    import torch
    prev = torch.cuda.current_device()
    try:
        renderer.init(num_bounces=num_bounces, device=device_index)
    finally:
        torch.cuda.set_device(prev)


def set_env_map(env, device_index: int = 0, num_bounces: int = 4) -> None:
    """Copy an env map (H x W x 3 f32, row 0 = bottom, as LoadTexture returns it) into HBM for
    device jobs with use_env=True; None releases it."""
    ensure_backend(device_index, num_bounces)
    from .renderer import set_env_map as _set
    _set(env)


def _job(buf, width: int, height: int, row_start: int, row_stride: int, nrows: int, frame_first: int,
         nframes: int, num_bounces: int, layout: int, use_env: bool = False) -> N.PtDeviceJob:
    import torch
    if not isinstance(buf, torch.Tensor) or buf.device.type != "cuda":
        raise N.PtError(N.PT_EINVAL, "render_device", "buf must be a device (cuda/hip) tensor")
    if buf.dtype != torch.float32 or not buf.is_contiguous():
        raise N.PtError(N.PT_EINVAL, "render_device", "buf must be contiguous float32")
    if buf.numel() < nrows * width * 3:
        raise N.PtError(N.PT_EINVAL, "render_device", f"buf holds {buf.numel()} < {nrows}x{width}x3 floats")
    ensure_backend(buf.device.index if buf.device.index is not None else torch.cuda.current_device(), num_bounces)
    return N.PtDeviceJob(buf.data_ptr(), width, height, row_start, row_stride, nrows, layout, frame_first,
                         nframes, num_bounces, 1 if use_env else 0)


def _stream(stream):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def render_device(buf, width: int, height: int, *, frame_first: int, nframes: int, num_bounces: int,
                  row_start: int = 0, row_stride: int = 1, nrows: int | None = None,
                  layout: int = N.PT_LAYOUT_INTERLEAVED, use_env: bool = False, stream=None,
                  chain: bool = False) -> None:
    """Accumulate frames [frame_first, frame_first+nframes) of global rows row_start + k*row_stride
    (k < nrows) into `buf` (nrows x width x 3 f32, in HBM).  Asynchronous on `stream`.
    use_env: miss radiance from the env map of set_env_map (config 4) instead of the ambient.
    chain: pt_render_device_chain -- this launch may overlap the previous chained launch of the same
    geometry on `stream` (same result; nothing enqueued on `stream` since that call may be needed)."""
    nrows = height if nrows is None else nrows
    job = _job(buf, width, height, row_start, row_stride, nrows, frame_first, nframes, num_bounces, layout, use_env)
    fn = "pt_render_device_chain" if chain else "pt_render_device"
    N.check(getattr(N.load(), fn)(ctypes.byref(job), _stream(stream)), fn)


def chain_counts() -> dict:
    """pt_chain_counts: chained launches since init that restarted / continued the overlap."""
    r, c = ctypes.c_uint64(0), ctypes.c_uint64(0)
    N.check(N.load().pt_chain_counts(ctypes.byref(r), ctypes.byref(c)), "pt_chain_counts")
    return {"restarts": int(r.value), "continued": int(c.value)}


def render_device_present(buf, pixels, width: int, height: int, *, frame_first: int, nframes: int,
                          num_bounces: int, row_start: int = 0, row_stride: int = 1, nrows: int | None = None,
                          layout: int = N.PT_LAYOUT_INTERLEAVED, use_env: bool = False,
                          pixel_format: int = N.PT_PIXEL_RGBA8, stream=None) -> None:
    """render_device with the output stage fused into the render (pt_render_device_present): also
    writes the job's rows as packed 8-bit pixels (nrows x width int32/uint32 device tensor `pixels`,
    PT_PIXEL_RGBA8 = OutputToFile, PT_PIXEL_XRGB8 = OutputToScreen) -- equal to render_device followed
    by the standalone output stage on those rows.  Asynchronous on `stream`."""
    nrows = height if nrows is None else nrows
    job = _job(buf, width, height, row_start, row_stride, nrows, frame_first, nframes, num_bounces, layout, use_env)
    _check_pixels(pixels, width * nrows, buf)
    N.check(N.load().pt_render_device_present(ctypes.byref(job), pixels.data_ptr(), pixel_format, _stream(stream)),
            "pt_render_device_present")


def launch_variant(buf, width: int, height: int, *, nframes: int, num_bounces: int, row_start: int = 0,
                   row_stride: int = 1, nrows: int | None = None, layout: int = N.PT_LAYOUT_INTERLEAVED,
                   use_env: bool = False) -> dict:
    """The continuous-tiles launch variant of this job's geometry (pt_launch_variant): waves per SIMD
    (0: not decided yet) and the back-claim share in percent."""
    nrows = height if nrows is None else nrows
    job = _job(buf, width, height, row_start, row_stride, nrows, 1, nframes, num_bounces, layout, use_env)
    w, b = ctypes.c_int32(0), ctypes.c_int32(0)
    N.check(N.load().pt_launch_variant(ctypes.byref(job), ctypes.byref(w), ctypes.byref(b)), "pt_launch_variant")
    return {"waves_per_simd": int(w.value), "back_claim_pct": int(b.value)}


CAM_CACHE_STATES = ("none", "empty", "filled", "settled")   # PT_CAM_CACHE_*


def cam_cache_query(buf, width: int, height: int, *, nframes: int, num_bounces: int, row_start: int = 0,
                    row_stride: int = 1, nrows: int | None = None, layout: int = N.PT_LAYOUT_INTERLEAVED,
                    use_env: bool = False, stream=None) -> dict:
    """The camera-hit cache of this job's geometry and launch length on `stream` (pt_cam_cache_query):
    its state ("none": such launches trace their camera rays) and the records the device's last
    count_device launch compared with the hits it traced."""
    nrows = height if nrows is None else nrows
    job = _job(buf, width, height, row_start, row_stride, nrows, 1, nframes, num_bounces, layout, use_env)
    s, c = ctypes.c_int32(0), ctypes.c_uint64(0)
    N.check(N.load().pt_cam_cache_query(ctypes.byref(job), _stream(stream), ctypes.byref(s), ctypes.byref(c)),
            "pt_cam_cache_query")
    return {"state": CAM_CACHE_STATES[int(s.value)], "compared": int(c.value)}


def tonemap_device(buf, width: int, nrows: int, pixels, *, layout: int = N.PT_LAYOUT_INTERLEAVED,
                   pixel_format: int = N.PT_PIXEL_RGBA8, stream=None) -> None:
    """The standalone output stage (pt_tonemap_device) on an HBM accumulator of nrows x width pixels
    into `pixels` (nrows x width 32-bit words).  Asynchronous on `stream`."""
    _check_pixels(pixels, width * nrows, buf)
    N.check(N.load().pt_tonemap_device(buf.data_ptr(), width, nrows, layout, 0, 0, pixels.data_ptr(), pixel_format,
                                       _stream(stream)), "pt_tonemap_device")


def _check_pixels(pixels, n: int, buf) -> None:
    import torch
    if not isinstance(pixels, torch.Tensor) or pixels.device != buf.device:
        raise N.PtError(N.PT_EINVAL, "render_device_present", "pixels must be a tensor on the buffer's device")
    if pixels.element_size() != 4 or not pixels.is_contiguous() or pixels.numel() < n:
        raise N.PtError(N.PT_EINVAL, "render_device_present", f"pixels must hold >= {n} contiguous 32-bit words")


def count_device(buf, width: int, height: int, *, frame_first: int, nframes: int, num_bounces: int,
                 row_start: int = 0, row_stride: int = 1, nrows: int | None = None,
                 layout: int = N.PT_LAYOUT_INTERLEAVED, use_env: bool = False, stream=None) -> dict:
    """Like render_device (it does render into buf) but also counts the work: traced segments,
    issued lane-slots, samples, escaped paths.  Synchronous."""
    nrows = height if nrows is None else nrows
    job = _job(buf, width, height, row_start, row_stride, nrows, frame_first, nframes, num_bounces, layout, use_env)
    out = N.PtWorkCounts()
    N.check(N.load().pt_count_device(ctypes.byref(job), _stream(stream), ctypes.byref(out)), "pt_count_device")
    return {"segments": out.segments, "lane_slots": out.lane_slots, "samples": out.samples, "escaped": out.escaped,
            "primary": out.primary, "quad_fallbacks": out.quad_fallbacks, "sky_skipped": out.sky_skipped}


class JobLauncher:
    """A prepared device job: the argument checks and the ctypes job are built once, and each call
    enqueues one render (pt_render_device, or pt_v4_render_device with v4=True) changing only
    frame_first -- a launch then costs the host a few microseconds instead of the tens a full
    render_device call spends in Python (the bench's timed loop; bench.py)."""

    def __init__(self, buf, width: int, height: int, *, nframes: int, num_bounces: int, row_start: int = 0,
                 row_stride: int = 1, nrows: int | None = None, layout: int = N.PT_LAYOUT_INTERLEAVED,
                 use_env: bool = False, stream=None, v4: bool = False, pixels=None,
                 pixel_format: int = N.PT_PIXEL_RGBA8, chain: bool = False):
        nrows = height if nrows is None else nrows
        self._buf = buf   # (kept alive with the job that points at it)
        self.job = _job(buf, width, height, row_start, row_stride, nrows, 1, nframes, num_bounces, layout, use_env)
        L = N.load()
        self._ref = ctypes.byref(self.job)
        self._stream = _stream(stream)
        if pixels is not None:   # the fused output stage (pt_render_device_present / pt_v4_render_device_present)
            _check_pixels(pixels, width * nrows, buf)
            self._pixels = pixels
            self._what = "pt_v4_render_device_present" if v4 else "pt_render_device_present"
            fn, args = getattr(L, self._what), (self._ref, pixels.data_ptr(), pixel_format, self._stream)
        else:
            # chain: pt_render_device_chain / pt_v4_render_device_chain, consecutive launches overlap
            self._what = ("pt_v4_render_device" if v4 else "pt_render_device") + ("_chain" if chain else "")
            fn = getattr(L, self._what)
            args = (self._ref, self._stream)
        self._fn, self._args = fn, args

    def __call__(self, frame_first: int) -> None:
        if frame_first < 1:
            raise N.PtError(N.PT_EINVAL, self._what, "frame_first must be >= 1")
        self.job.frame_first = frame_first
        rc = self._fn(*self._args)
        if rc != N.PT_OK:
            N.check(rc, self._what)


def check_device_errors() -> None:
    """Raise PtError(PT_EKERNEL) if a device-resident launch since the last check abandoned a tile
    (pt_check_device_errors).  Call after synchronising the streams the jobs ran on."""
    N.check(N.load().pt_check_device_errors(), "pt_check_device_errors")


def render_v4_device(buf, width: int, height: int, *, frame_first: int, nframes: int, num_bounces: int = 8,
                     row_start: int = 0, row_stride: int = 1, nrows: int | None = None,
                     layout: int = N.PT_LAYOUT_INTERLEAVED, use_env: bool = False, stream=None) -> None:
    """The v4 renderer on an HBM-resident accumulator (see render_device); use_env selects the env
    mode of renderer.v4_config with the map of set_env_map.  Asynchronous on `stream`."""
    nrows = height if nrows is None else nrows
    job = _job(buf, width, height, row_start, row_stride, nrows, frame_first, nframes, num_bounces, layout, use_env)
    N.check(N.load().pt_v4_render_device(ctypes.byref(job), _stream(stream)), "pt_v4_render_device")


def render_v4_device_present(buf, pixels, width: int, height: int, *, frame_first: int, nframes: int,
                             num_bounces: int = 8, row_start: int = 0, row_stride: int = 1, nrows: int | None = None,
                             layout: int = N.PT_LAYOUT_INTERLEAVED, use_env: bool = False,
                             pixel_format: int = N.PT_PIXEL_RGBA8, stream=None) -> None:
    """render_v4_device with the output stage fused into the render (pt_v4_render_device_present): also
    writes the job's rows as packed 8-bit pixels (nrows x width int32/uint32 device tensor `pixels`,
    row k = the job's row k; PT_PIXEL_RGBA8 = OutputToFile, PT_PIXEL_XRGB8 = OutputToScreen) with the
    tonemap flags of renderer.v4_config -- equal to render_v4_device followed by tonemap_device on
    those rows.  Launches of 8 or more frames that run the continuous-tiles kernel with the default
    tonemap flags write the pixels in the render kernel; every other launch converts in a second pass
    on the same stream.  Asynchronous on `stream`."""
    nrows = height if nrows is None else nrows
    job = _job(buf, width, height, row_start, row_stride, nrows, frame_first, nframes, num_bounces, layout, use_env)
    _check_pixels(pixels, width * nrows, buf)
    N.check(N.load().pt_v4_render_device_present(ctypes.byref(job), pixels.data_ptr(), pixel_format, _stream(stream)),
            "pt_v4_render_device_present")


def _v4_batch(what: str, buf, cameras, width: int, height: int, nrows, job_kw: dict, pixels, pixel_format: int, *,
              frames=None, scenes=None, scene_of_view=None, envs=None, env_of_view=None):
    """The arguments of a batched v4 launch, marshalled once for the four render_v4_device_* calls: (the
    pt_device_job, a filled pt_v4_batch, the list that keeps its ctypes arrays alive).  `what` names the caller
    in every PtError; job_kw: _job's keywords but nrows."""
    nrows = height if nrows is None else nrows
    cams = [(tuple(float(x) for x in pos), float(fov)) for pos, fov in cameras]
    nviews = len(cams)
    if any(len(pos) != 3 for pos, _ in cams):
        raise N.PtError(N.PT_EINVAL, what, "a camera position has three components")
    if not 1 <= nviews <= N.PT_V4_MAX_VIEWS:
        raise N.PtError(N.PT_EINVAL, what, f"{nviews} cameras outside [1, {N.PT_V4_MAX_VIEWS}]")
    # (_job checks the tensor against nrows: the batch as one job of V x nrows rows, then the job's own rows)
    job = _job(buf, width, height, nrows=nviews * nrows, **job_kw)
    job.nrows = nrows
    if pixels is not None:
        _check_pixels(pixels, nviews * nrows * width, buf)
    keep = []

    def per_view(m, name, ctype, conv):
        if m is None:
            return None
        if len(m) != nviews:
            raise N.PtError(N.PT_EINVAL, what, f"{name} has {len(m)} entries for {nviews} views")
        keep.append((ctype * nviews)(*[conv(x) for x in m]))
        return keep[-1]
    b = N.PtV4Batch()
    b.cams, b.nviews = per_view(cams, "cameras", N.PtV4Camera, lambda c: N.PtV4Camera((ctypes.c_float * 3)(*c[0]), c[1])), nviews
    b.frames = per_view(frames, "frames", N.PtV4FrameRange, lambda r: N.PtV4FrameRange(int(r[0]), int(r[1])))
    if scenes is not None:
        descs = [v4_scene_desc(s) for s in scenes]
        if not descs:
            raise N.PtError(N.PT_EINVAL, what, "no scenes")
        keep.append((N.PtV4SceneDesc * len(descs))(*descs))
        b.scenes, b.nscenes = keep[-1], len(descs)
    b.scene_of_view = per_view(scene_of_view, "scene_of_view", ctypes.c_int32, int)
    b.envs = envs.handle if envs is not None else None
    b.env_of_view = per_view(env_of_view, "env_of_view", ctypes.c_int32, int)
    b.pixels = pixels.data_ptr() if pixels is not None else None
    b.format = pixel_format
    return job, b, keep


def render_v4_device_views(buf, cameras, width: int, height: int, *, frame_first: int, nframes: int, num_bounces: int = 8,
                           row_start: int = 0, row_stride: int = 1, nrows: int | None = None,
                           layout: int = N.PT_LAYOUT_INTERLEAVED, use_env: bool = False, pixels=None,
                           pixel_format: int = N.PT_PIXEL_RGBA8, stream=None) -> None:
    """A batch of views in one launch (pt_v4_render_device_views): `cameras` is a sequence of (position,
    fov_degrees) as renderer.v4_camera takes them, `buf` a contiguous f32 device tensor of at least
    V x nrows x width x 3 elements (e.g. shaped [V, nrows, W, 3]) whose slice v ends bit for bit as
    v4_camera(*cameras[v]) + render_v4_device on it would leave it.  pixels: an optional 32-bit tensor of
    V x nrows x width words, each slice equal to tonemap_device on its accumulator slice.  The camera of
    v4_camera and the v4 frame counter are neither read nor changed.  Asynchronous on `stream`."""
    job_kw = dict(row_start=row_start, row_stride=row_stride, frame_first=frame_first, nframes=nframes, num_bounces=num_bounces,
                  layout=layout, use_env=use_env)
    job, b, _keep = _v4_batch("render_v4_device_views", buf, cameras, width, height, nrows, job_kw, pixels, pixel_format)
    N.check(N.load().pt_v4_render_device_views(ctypes.byref(job), b.cams, b.nviews, b.pixels, b.format, _stream(stream)),
            "pt_v4_render_device_views")


def v4_scene_desc(scene) -> "N.PtV4SceneDesc":
    """A pt_v4_scene_desc from {"quads", "spheres", "materials"} (or a (quads, spheres, materials) sequence):
    quads 4 x 3 (V0..V3), spheres (x, y, z, r), materials dicts with the keys of renderer.v4_get_scene_desc
    (or AddMaterialToScene's long names; missing fields are zero, like `SceneMaterial{ 0 }`).  The counts are
    passed on as given -- the library rejects a scene that is too large -- but only what fits is copied."""
    import numpy as np
    from .renderer import _MAT_KEYS
    if isinstance(scene, N.PtV4SceneDesc):
        return scene
    if isinstance(scene, dict):
        quads, spheres, mats = scene.get("quads", ()), scene.get("spheres", ()), scene.get("materials", ())
    else:
        quads, spheres, mats = scene
    d = N.PtV4SceneDesc()
    d.nquads, d.nspheres, d.nmaterials = len(quads), len(spheres), len(mats)
    for i, q in enumerate(quads[:N.PT_V4_MAX_OBJECTS]):
        d.quads[i][:] = [float(x) for x in np.asarray(q, np.float32).reshape(12)]
    for i, p in enumerate(spheres[:N.PT_V4_MAX_OBJECTS]):
        d.spheres[i][:] = [float(x) for x in np.asarray(p, np.float32).reshape(4)]
    for i, m in enumerate(mats[:N.PT_V4_MAX_OBJECTS]):
        for short, long in _MAT_KEYS:
            v = m.get(short, m.get(long))
            if v is None:
                continue
            if short in ("albedo", "emissive", "spec_color", "refr_color"):
                getattr(d.materials[i], long)[:] = [float(x) for x in v]
            else:
                setattr(d.materials[i], long, float(v))
    return d


def render_v4_device_scenes(buf, scenes, cameras, width: int, height: int, scene_of_view=None, *, frame_first: int,
                            nframes: int, num_bounces: int = 8, row_start: int = 0, row_stride: int = 1,
                            nrows: int | None = None, layout: int = N.PT_LAYOUT_INTERLEAVED, use_env: bool = False,
                            pixels=None, pixel_format: int = N.PT_PIXEL_RGBA8, stream=None) -> None:
    """A batch of scenes in one launch (pt_v4_render_device_scenes): render_v4_device_views with a scene per
    view.  `scenes` is a sequence of scene descriptions (v4_scene_desc), `cameras` one (position,
    fov_degrees) per view; view v renders scenes[scene_of_view[v]] -- scene v when scene_of_view is None,
    which needs as many scenes as cameras.  Slice v of `buf` ends bit for bit as ClearScene, the
    description's Add*ToScene calls, v4_camera(*cameras[v]) and render_v4_device on it would leave it; the
    scene of Add*ToScene, the camera of v4_camera and the v4 frame counter are neither read nor changed.
    Asynchronous on `stream`."""
    descs = [v4_scene_desc(s) for s in scenes]   # (here `scenes` is not optional)
    if not descs:
        raise N.PtError(N.PT_EINVAL, "render_v4_device_scenes", "no scenes")
    job_kw = dict(row_start=row_start, row_stride=row_stride, frame_first=frame_first, nframes=nframes, num_bounces=num_bounces,
                  layout=layout, use_env=use_env)
    job, b, _keep = _v4_batch("render_v4_device_scenes", buf, cameras, width, height, nrows, job_kw, pixels, pixel_format,
                              scenes=descs, scene_of_view=scene_of_view)
    N.check(N.load().pt_v4_render_device_scenes(ctypes.byref(job), b.scenes, b.nscenes, b.cams, b.scene_of_view, b.nviews,
                                                b.pixels, b.format, _stream(stream)), "pt_v4_render_device_scenes")


class V4EnvSet:
    """An env set (pt_v4_make_env_set): textures resident in device memory until close() or garbage
    collection.  pt_shutdown releases every set; closing one after that is harmless."""

    def __init__(self, handle: int, count: int):
        self._handle, self.count = handle, count

    def __len__(self) -> int:
        return self.count

    @property
    def handle(self) -> int:
        if not self._handle:
            raise N.PtError(N.PT_EINVAL, "V4EnvSet", "the env set is closed")
        return self._handle

    def close(self) -> None:
        if self._handle:
            N.load().pt_v4_free_env_set(self._handle)
            self._handle = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:   # (interpreter teardown)
            pass


def make_v4_env_set(textures) -> V4EnvSet:
    """Upload a list of H x W x 3 float32 arrays (shapes may differ) as one env set, once; each is read as the
    v4_config's env_mode says at render time (equirect, or six cubemap faces stacked).  Synchronous."""
    from .renderer import _pt_texture
    pairs = [_pt_texture(t) for t in textures]
    if not pairs:
        raise N.PtError(N.PT_EINVAL, "make_v4_env_set", "no textures")
    arr = (N.PtTexture * len(pairs))(*[p for p, _ in pairs])
    out = ctypes.c_void_p()
    N.check(N.load().pt_v4_make_env_set(arr, len(pairs), ctypes.byref(out)), "pt_v4_make_env_set")
    del pairs
    return V4EnvSet(out.value, len(arr))


def render_v4_device_envs(buf, envs: V4EnvSet, cameras, width: int, height: int, env_of_view=None, scenes=None,
                          scene_of_view=None, *, frame_first: int, nframes: int, num_bounces: int = 8, row_start: int = 0,
                          row_stride: int = 1, nrows: int | None = None, layout: int = N.PT_LAYOUT_INTERLEAVED,
                          use_env: bool = True, pixels=None, pixel_format: int = N.PT_PIXEL_RGBA8, stream=None) -> None:
    """A batch of env maps in one launch (pt_v4_render_device_envs): render_v4_device_scenes with a texture per
    view.  View v reads texture env_of_view[v] of `envs` (make_v4_env_set) -- texture v when env_of_view is
    None, which needs as many textures as cameras -- and renders scenes[scene_of_view[v]], or the current
    scene when `scenes` is None.  Slice v of `buf` ends bit for bit as set_env_map(that texture), that scene
    built through ClearScene + Add*ToScene, v4_camera(*cameras[v]) and render_v4_device on it would leave it;
    the env map of set_env_map, the scene, the camera and the v4 frame counter are not changed.  Asynchronous
    on `stream`."""
    job_kw = dict(row_start=row_start, row_stride=row_stride, frame_first=frame_first, nframes=nframes, num_bounces=num_bounces,
                  layout=layout, use_env=use_env)
    job, b, _keep = _v4_batch("render_v4_device_envs", buf, cameras, width, height, nrows, job_kw, pixels, pixel_format,
                              scenes=scenes, scene_of_view=scene_of_view, envs=envs, env_of_view=env_of_view)
    N.check(N.load().pt_v4_render_device_envs(ctypes.byref(job), b.envs, b.env_of_view, b.scenes, b.nscenes, b.scene_of_view,
                                              b.cams, b.nviews, b.pixels, b.format, _stream(stream)), "pt_v4_render_device_envs")


def render_v4_device_batch(buf, cameras, width: int, height: int, *, frames=None, scenes=None, scene_of_view=None, envs=None,
                           env_of_view=None, pixels=None, frame_first: int = 1, nframes: int = 0, num_bounces: int = 8,
                           row_start: int = 0, row_stride: int = 1, nrows: int | None = None,
                           layout: int = N.PT_LAYOUT_INTERLEAVED, use_env: bool | None = None,
                           pixel_format: int = N.PT_PIXEL_RGBA8, stream=None, stats=None) -> None:
    """Everything per view in one launch (pt_v4_render_device_batch): render_v4_device_envs with a frame range
    per view.  `frames` is a sequence of (frame_first, nframes), one per camera -- a view of 0 frames keeps its
    slice of `buf` bit for bit and still gets its pixels -- or None: every view renders the keywords
    frame_first / nframes (which are not read otherwise).  `scenes` None: the current scene.  `envs` None: the
    map of set_env_map when use_env (None: "when a set is given"), else the ambient.  Slice v of `buf` ends bit
    for bit as that view's env map, scene, v4_camera(*cameras[v]) and render_v4_device over frames[v] would
    leave it; no process-wide state is changed.  Asynchronous on `stream`.

    `stats` None: that call.  A contiguous int32 tensor of nviews x 4 on `buf`'s device: the same render through
    pt_v4_render_device_batch_stats, which overwrites row v with view v's pt_v4_view_stats record -- how much the
    view's 8-bit image (the v4_config's tonemap pair; R, G, B) moved in this launch: columns 0 and 1 are the low
    and high word of sum_delta, column 2 is `changed`, column 3 is max_delta (v4_view_stats reads them).  A view
    of 0 frames has zeros.  Read it after the stream reaches the call."""
    job_kw = dict(row_start=row_start, row_stride=row_stride, frame_first=frame_first, nframes=nframes, num_bounces=num_bounces,
                  layout=layout, use_env=envs is not None if use_env is None else use_env)
    job, b, _keep = _v4_batch("render_v4_device_batch", buf, cameras, width, height, nrows, job_kw, pixels, pixel_format,
                              frames=frames, scenes=scenes, scene_of_view=scene_of_view, envs=envs, env_of_view=env_of_view)
    if stats is None:
        N.check(N.load().pt_v4_render_device_batch(ctypes.byref(job), ctypes.byref(b), _stream(stream)), "pt_v4_render_device_batch")
        return
    import torch
    if (not isinstance(stats, torch.Tensor) or stats.device != buf.device or stats.dtype != torch.int32 or
            tuple(stats.shape) != (b.nviews, 4) or not stats.is_contiguous()):
        raise N.PtError(N.PT_EINVAL, "render_v4_device_batch",
                        f"stats must be a contiguous int32 tensor of {b.nviews} x 4 on the buffer's device")
    N.check(N.load().pt_v4_render_device_batch_stats(ctypes.byref(job), ctypes.byref(b), stats.data_ptr(), _stream(stream)),
            "pt_v4_render_device_batch_stats")


def v4_view_stats(stats) -> list[dict]:
    """The records of a `stats` tensor of render_v4_device_batch as [{sum_delta, changed, max_delta}], one per view.
    It copies the tensor to the host, which waits for the work queued before on the current stream: nviews x 16
    bytes."""
    import numpy as np
    a = np.ascontiguousarray(stats.cpu().numpy()).view(np.dtype([("sum_delta", "<u8"), ("changed", "<u4"), ("max_delta", "<u4")]))
    return [{"sum_delta": int(r["sum_delta"]), "changed": int(r["changed"]), "max_delta": int(r["max_delta"])} for r in a.reshape(-1)]


def render_v4_adaptive(buf, cameras, width: int, height: int, *, max_frames: int, frames_per_round: int = 8, tol: int = 0,
                       patience: int = 1, **batch_kw) -> list[int]:
    """Render every view until its displayed image stops moving, in rounds of one batch launch each; returns the
    frames each view rendered.  Every view starts at frame 1 (the caller zeroes `buf` for a fresh image, or keeps
    what is there to blend into).  Each round an active view gets min(frames_per_round, max_frames - done) frames
    and a retired view 0 (its slice and pixels stay as they are); after the launch the nviews statistics records
    are read back -- the only synchronisation, 16 bytes per view.  A view's quiet count goes up when its max_delta
    <= tol and is reset to 0 otherwise; the view retires when the count reaches `patience`, or at max_frames.
    `batch_kw`: the keywords of render_v4_device_batch but frames, frame_first, nframes and stats.

    8-bit stability is a display criterion, not a variance bound: it says the picture on screen has stopped
    changing at this frame count's blend factor (1 / (frame + 1) shrinks every round), not that the estimate's
    error is below anything.  Use a larger `patience` where a view may rest for one round and move again."""
    import torch
    for k in ("frames", "frame_first", "nframes", "stats"):
        if k in batch_kw:
            raise N.PtError(N.PT_EINVAL, "render_v4_adaptive", f"the keyword {k} is the loop's own")
    if max_frames < 0 or frames_per_round < 1 or patience < 1 or tol < 0:
        raise N.PtError(N.PT_EINVAL, "render_v4_adaptive", "max_frames >= 0, frames_per_round >= 1, patience >= 1, tol >= 0")
    cameras = list(cameras)
    nviews = len(cameras)
    done, quiet = [0] * nviews, [0] * nviews
    active = [max_frames > 0] * nviews
    stats = torch.zeros((nviews, 4), dtype=torch.int32, device=buf.device) if nviews else None
    stream = batch_kw.get("stream")
    while any(active):
        frames = [(1 + done[v], min(frames_per_round, max_frames - done[v]) if active[v] else 0) for v in range(nviews)]
        render_v4_device_batch(buf, cameras, width, height, frames=frames, stats=stats, **batch_kw)
        if stream is not None:
            stream.synchronize()
        recs = v4_view_stats(stats)
        for v in range(nviews):
            if not active[v]:
                continue
            done[v] += frames[v][1]
            quiet[v] = quiet[v] + 1 if recs[v]["max_delta"] <= tol else 0
            active[v] = quiet[v] < patience and done[v] < max_frames
    return done


def count_v4_device(buf, width: int, height: int, *, frame_first: int, nframes: int, num_bounces: int = 8,
                    row_start: int = 0, row_stride: int = 1, nrows: int | None = None,
                    layout: int = N.PT_LAYOUT_INTERLEAVED, use_env: bool = False, stream=None) -> dict:
    """render_v4_device + work counters (segments, lane_slots, samples, escaped).  Synchronous."""
    nrows = height if nrows is None else nrows
    job = _job(buf, width, height, row_start, row_stride, nrows, frame_first, nframes, num_bounces, layout, use_env)
    out = N.PtWorkCounts()
    N.check(N.load().pt_v4_count_device(ctypes.byref(job), _stream(stream), ctypes.byref(out)), "pt_v4_count_device")
    return {"segments": out.segments, "lane_slots": out.lane_slots, "samples": out.samples, "escaped": out.escaped,
            "sphere_fallbacks": out.sphere_fallbacks, "sky_skipped": out.sky_skipped}
