"""The camera-hit cache (pt_capi.cpp Sched::cam, pt_kernel.hip render_body_ct) against
the oracle, bit for bit.

A geometry's first uncounted continuous-tiles launch of at least 8 frames stores what TestSceneTrace
returned for every pixel's camera ray; every later such launch of the geometry loads the records
instead of tracing; shorter launches trace as ever.  The accumulator must stay the reference's
(demofox_path_tracing_scalar.cpp:785-820) whichever launch computed a pixel's camera hit, so every
case here runs launch sequences that fill and then use the cache and compares with
oracle/pt_oracle.c -- and with the same sequence under PT_MI355_CAM_CACHE=0.  The geometries are the
smallest that get a schedule entry (>= 512 tiles, pt_launch_plan.h kSchedMinTiles) with a width and height
that are no multiples of 8, so edge tiles have invalid lanes.

Which path the launches took is asserted through pt_cam_cache_query: the cache's state after each
launch (none / filled / settled), and, for a counted launch, how many traced hits it compared with
their records (every pixel outside the sky tiles; a difference is guard 15).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from conftest import bits_equal, mismatch_report
from oracle import pyoracle

pytestmark = pytest.mark.gpu

W, H, B = 188, 180, 8   # 24 x 23 = 552 tiles; 188 = 23 * 8 + 4, 180 = 22 * 8 + 4
KNOB = "PT_MI355_CAM_CACHE"


@pytest.fixture
def fresh(monkeypatch):
    """A fresh library state initialised under the test's environment."""
    import cpuperformanceraytracer_amd as pt

    def init(bounces=B, samples_per_frame=1, **envs):
        pt.shutdown()
        for k, v in envs.items():
            monkeypatch.setenv(k, v)
        pt.init(num_bounces=bounces, samples_per_frame=samples_per_frame)
    yield init
    pt.shutdown()


@functools.lru_cache(maxsize=None)
def _oracle(w, h, frames, bounces, row_start=0, row_stride=1, nrows=None, env=False):
    from cpuperformanceraytracer_amd.config import synthetic_env
    ref = pyoracle.render(w, h, nframes=frames, num_bounces=bounces, row_start=row_start, row_stride=row_stride,
                          nrows=nrows, env=synthetic_env() if env else None)
    ref.setflags(write=False)
    return ref


def _launches(w, h, bounces, sizes, *, chain=False, env=False, row_start=0, row_stride=1, nrows=None, buf=None,
              frame=1):
    """One launch per entry of `sizes` (its frames) into `buf` (zeroed when None).  Returns (images,
    states): the image after each launch (chained: after the last only) and the cache's state for that
    launch's length right after it was enqueued."""
    import torch
    from cpuperformanceraytracer_amd.device import cam_cache_query, check_device_errors, render_device
    nrows = h if nrows is None else nrows
    if buf is None:
        buf = torch.zeros(nrows * w * 3, dtype=torch.float32, device="cuda:0")
    geo = dict(num_bounces=bounces, row_start=row_start, row_stride=row_stride, nrows=nrows, use_env=env)
    images, states = [], []
    for s in sizes:
        render_device(buf, w, h, frame_first=frame, nframes=s, chain=chain, **geo)
        states.append(cam_cache_query(buf, w, h, nframes=s, **geo)["state"])
        frame += s
        if not chain:
            torch.cuda.synchronize()
            images.append(buf.cpu().numpy().reshape(nrows, w, 3))
    torch.cuda.synchronize()
    check_device_errors()
    if chain:
        images.append(buf.cpu().numpy().reshape(nrows, w, 3))
    return images, states


def test_fill_then_use_equal_oracle_and_knob_off(fresh):
    """The fill launch and two launches that use the cache, frame_first advancing by 8: the whole image
    equals the oracle after each launch, and the same sequence with the cache switched off leaves
    byte-identical buffers."""
    fresh()
    on, states = _launches(W, H, B, [8, 8, 8])
    assert states == ["filled", "settled", "settled"], states
    for k, img in enumerate(on):
        ref = _oracle(W, H, 8 * (k + 1), B)
        assert bits_equal(img, ref), (k, mismatch_report(img, ref))
    fresh(**{KNOB: "0"})
    off, states = _launches(W, H, B, [8, 8, 8])
    assert states == ["none"] * 3, states
    for k, (a, b) in enumerate(zip(on, off)):
        assert a.tobytes() == b.tobytes(), (k, mismatch_report(a, b))


def test_chained_fill_restart_continue(fresh):
    """Chained launches at a fixed launch variant: the fill launch, the restart after it, then launches
    that continue the overlap while reading the cache.  The image after 7 x 8 frames equals the oracle,
    and at least three launches continued."""
    from cpuperformanceraytracer_amd.device import chain_counts
    fresh(PT_MI355_CT_WAVES="6")
    c0 = chain_counts()
    imgs, states = _launches(W, H, B, [8] * 7, chain=True)
    c1 = chain_counts()
    assert states == ["filled"] + ["settled"] * 6, states
    assert c1["continued"] - c0["continued"] >= 3, (c0, c1)
    assert c1["restarts"] - c0["restarts"] >= 2, (c0, c1)   # the fill launch and the one after it
    ref = _oracle(W, H, 56, B)
    assert bits_equal(imgs[-1], ref), mismatch_report(imgs[-1], ref)


def test_short_chained_launches_neither_fill_nor_restart(fresh):
    """One frame per launch, chained (a progressive host): below the cache's launch length, so no
    launch fills, none is forced to restart (all but the first two continue), no cache exists for the
    geometry's 8-frame launches either, and the image equals the oracle.  Then 8-frame chained launches
    of the same geometry fill and use the cache while 1-frame launches between them go on tracing."""
    import torch
    from cpuperformanceraytracer_amd.device import cam_cache_query, chain_counts
    fresh(PT_MI355_CT_WAVES="6")
    buf = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda:0")
    c0 = chain_counts()
    imgs, states = _launches(W, H, B, [1] * 8, chain=True, buf=buf)
    c1 = chain_counts()
    assert states == ["none"] * 8, states
    assert c1["continued"] - c0["continued"] >= 5, (c0, c1)   # (as tests/test_gpu_chain.py: n - 3)
    assert cam_cache_query(buf, W, H, nframes=8, num_bounces=B)["state"] == "none"
    ref = _oracle(W, H, 8, B)
    assert bits_equal(imgs[-1], ref), mismatch_report(imgs[-1], ref)
    sizes = [8, 1, 8, 1, 8, 8]
    imgs, states = _launches(W, H, B, sizes, chain=True, buf=buf, frame=9)
    assert states == ["filled", "none", "settled", "none", "settled", "settled"], states
    ref = _oracle(W, H, 8 + sum(sizes), B)
    assert bits_equal(imgs[-1], ref), mismatch_report(imgs[-1], ref)


@pytest.mark.parametrize("sizes,bounces,expect", [
    # several chunks per tile (nframes > kChunk = 8), the last one short
    ([20, 20, 20], 8, ["filled", "settled", "settled"]),
    # one frame per launch, the progressive loop of a drop-in caller: below the cache's launch length
    ([1, 1, 1, 1], 8, ["none"] * 4),
    # c_numBounces 0: no items, the constant fold alone
    ([8, 8, 8], 0, ["filled", "settled", "settled"]),
    # either side of the launch length in one geometry: 7 traces, 8 fills, 7 traces, 8 and 8 use
    ([7, 8, 7, 8, 8], 8, ["none", "filled", "none", "settled", "settled"]),
])
def test_launch_shapes(fresh, sizes, bounces, expect):
    """Launch lengths on either side of the chunk size and of the cache's launch length, and a launch
    without items: the image after every launch equals the oracle."""
    fresh(bounces)
    imgs, states = _launches(W, H, bounces, sizes)
    assert states == expect, states
    done = 0
    for k, img in enumerate(imgs):
        done += sizes[k]
        ref = _oracle(W, H, done, bounces)
        assert bits_equal(img, ref), (k, mismatch_report(img, ref))


def test_row_shard(fresh):
    """A rank's row shard (rows 1::2 of a 188 x 364 image, the shape tests/test_gpu_configs.py gives
    rank 1 of 2): fill and two uses equal the oracle's rows."""
    fresh()
    h2 = 364
    nrows = h2 // 2
    imgs, states = _launches(W, h2, B, [8, 8, 8], row_start=1, row_stride=2, nrows=nrows)
    assert states == ["filled", "settled", "settled"], states
    for k, img in enumerate(imgs):
        ref = _oracle(W, h2, 8 * (k + 1), B, 1, 2, nrows)
        assert bits_equal(img, ref), (k, mismatch_report(img, ref))


def test_column_offset_tiles(fresh):
    """RenderTile of two 200 x 200 tiles side by side (625 8x8 tiles each, the second at column 200),
    8 samples per frame: each tile is a geometry of its own with its own cache; three frame calls
    (fill, use, use) equal the oracle.  (A host-buffer path: its cache state is not queried.)"""
    import cpuperformanceraytracer_amd as pt
    from layouts import tiled_to_interleaved
    fresh(samples_per_frame=8)
    w, h = 400, 200
    buf = np.zeros(w * h * 3, np.float32)
    tiles = pt.make_tiles(w, h, 2, 1)
    info = pt.RenderBufferInfo(buf, w, h, 3)
    for _ in range(3):
        pt.BeginFrame()
        for t in tiles:
            pt.RenderTile(info, t)
    img = tiled_to_interleaved(buf, w, h, 200, 200)
    ref = _oracle(w, h, 24, B)
    assert bits_equal(img, ref), mismatch_report(img, ref)


def test_two_geometries_alternated_and_eviction(fresh):
    """Two geometries alternated on one device, one of them with the env map, each against its own
    oracle image; then more geometries than the device keeps schedule entries for (16), which evicts
    the first geometry's entry and its cache, and one more launch of it (a fresh fill)."""
    import torch
    from cpuperformanceraytracer_amd.config import synthetic_env
    from cpuperformanceraytracer_amd.device import cam_cache_query, render_device, set_env_map
    fresh()
    set_env_map(synthetic_env(), 0, B)
    w2, h2 = 196, 172   # 25 x 22 = 550 tiles
    a = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda:0")
    b = torch.zeros(h2 * w2 * 3, dtype=torch.float32, device="cuda:0")
    for k in range(3):
        _, sa = _launches(W, H, B, [8], buf=a, frame=1 + 8 * k)
        _, sb = _launches(w2, h2, B, [8], buf=b, frame=1 + 8 * k, env=True)
        assert sa == sb == (["filled"] if k == 0 else ["settled"]), (k, sa, sb)
    ia, ib = a.cpu().numpy().reshape(H, W, 3), b.cpu().numpy().reshape(h2, w2, 3)
    ra, rb = _oracle(W, H, 24, B), _oracle(w2, h2, 24, B, env=True)
    assert bits_equal(ia, ra), mismatch_report(ia, ra)
    assert bits_equal(ib, rb), mismatch_report(ib, rb)
    scratch = torch.zeros(200 * 220 * 3, dtype=torch.float32, device="cuda:0")
    for k in range(17):
        render_device(scratch, 190 + k, 200, frame_first=1, nframes=1, num_bounces=B)
    assert cam_cache_query(a, W, H, nframes=8, num_bounces=B)["state"] == "none"   # evicted
    imgs, sa = _launches(W, H, B, [8], buf=a, frame=25)
    assert sa == ["filled"], sa
    ra = _oracle(W, H, 32, B)
    assert bits_equal(imgs[-1], ra), mismatch_report(imgs[-1], ra)


def test_counted_launch_checks_the_cache(fresh):
    """A counted launch once the cache is valid traces the camera rays as ever, so its work counters equal
    those of the same launch with the cache switched off, and it compares every traced hit (every pixel
    outside the sky tiles) with the cached record: the error words stay clear."""
    import torch
    from cpuperformanceraytracer_amd.device import cam_cache_query, check_device_errors, count_device
    counts, compared = {}, {}
    for knob in ("1", "0"):
        fresh(**{KNOB: knob})
        _launches(W, H, B, [8, 8])
        scratch = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda:0")
        counts[knob] = count_device(scratch, W, H, frame_first=17, nframes=8, num_bounces=B)
        compared[knob] = cam_cache_query(scratch, W, H, nframes=8, num_bounces=B)["compared"]
        torch.cuda.synchronize()
        check_device_errors()
        ref = pyoracle.render(W, H, frame_first=17, nframes=8, num_bounces=B)
        img = scratch.cpu().numpy().reshape(H, W, 3)
        assert bits_equal(img, ref), (knob, mismatch_report(img, ref))
    # (lane_slots is left out: 64 x the pool iterations the waves happened to run depends on which wave
    # claimed which tiles, so it differs from launch to launch of one library; the others count work)
    work = ("segments", "samples", "escaped", "primary", "quad_fallbacks", "sky_skipped")
    assert {k: counts["1"][k] for k in work} == {k: counts["0"][k] for k in work}, counts
    assert counts["1"]["primary"] == W * H, counts
    assert compared["1"] == W * H - counts["1"]["sky_skipped"] > 0, (compared, counts)
    assert compared["0"] == 0, compared


def test_across_schedule_rebuilds(fresh):
    """A schedule rebuild every 3 launches (PT_MI355_SCHED_REBUILD): the rebuilt order and its split
    tiles read the same per-tile records.  Plain and chained series of 8 launches equal the oracle."""
    fresh(PT_MI355_SCHED_REBUILD="3", PT_MI355_CT_WAVES="6")
    ref = _oracle(W, H, 64, B)
    imgs, states = _launches(W, H, B, [8] * 8)
    assert states == ["filled"] + ["settled"] * 7, states
    assert bits_equal(imgs[-1], ref), mismatch_report(imgs[-1], ref)
    imgs, states = _launches(W, H, B, [8] * 8, chain=True)
    assert states == ["settled"] * 8, states
    assert bits_equal(imgs[-1], ref), mismatch_report(imgs[-1], ref)


def test_env_kernel_fill_and_use(fresh):
    """The env continuous-tiles kernel (config 4's): one fill launch and one that uses the cache, 16
    frames each, against the oracle with the same env map."""
    from cpuperformanceraytracer_amd.config import synthetic_env
    from cpuperformanceraytracer_amd.device import set_env_map
    fresh()
    set_env_map(synthetic_env(), 0, B)
    imgs, states = _launches(W, H, B, [16, 16], env=True)
    assert states == ["filled", "settled"], states
    for k, img in enumerate(imgs):
        ref = _oracle(W, H, 16 * (k + 1), B, env=True)
        assert bits_equal(img, ref), (k, mismatch_report(img, ref))
