"""Host logic of bench.py (no GPU): the global image of an N-rank weak-scaling run keeps the
1920x1080 view (aspect ratio) and gives every rank ~1920x1080 pixels of interleaved rows."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import bench  # noqa: E402
from cpuperformanceraytracer_amd.shard import rows_of  # noqa: E402


@pytest.mark.parametrize("world", [1, 2, 3, 4, 8, 16])
def test_weak_image_keeps_view_and_per_rank_pixels(world):
    W, H = 1920, 1080
    Wg, Hg = bench.weak_image(W, H, world)
    assert Wg % 8 == 0
    assert abs((Wg / Hg) / (W / H) - 1.0) < 2e-3          # same aspect -> same camera view
    assert abs(Wg * Hg / (world * W * H) - 1.0) < 1e-2     # N x the pixels
    counts = [rows_of(r, world, Hg)[2] * Wg for r in range(world)]
    assert sum(counts) == Wg * Hg
    assert max(counts) - min(counts) <= Wg                 # balanced to one row
    if world == 1:
        assert (Wg, Hg) == (W, H)
    if world == 4:
        assert (Wg, Hg) == (3840, 2160)


def _tiny_run(argv, counted):
    """bench.run on the host clock, one rank, the oracle standing in for the GPU render."""
    from cpuperformanceraytracer_amd.config import Workload
    from oracle import pyoracle
    wl = Workload("tiny", 64, 36, 3, 8, scaling="weak")

    def render_fn(buf, W, H, f, n, rs, st, nr):
        pyoracle.render(W, H, frame_first=f, nframes=n, num_bounces=8, row_start=rs, row_stride=st, nrows=nr,
                        nthreads=2, buf=buf.numpy())

    def count_fn(buf, W, H, f, n, rs, st, nr):
        counted.append(f)
        render_fn(buf, W, H, f, n, rs, st, nr)
        _, c = pyoracle.render_counted(W, H, frame_first=f, nframes=n, num_bounces=8, row_start=rs,
                                       row_stride=st, nrows=nr)
        return {"segments": c["segments"], "samples": c["samples"], "escaped": c["escaped"],
                "lane_slots": c["segments"], "primary": c["samples"]}

    return wl, bench.run(bench.parse(argv), wl, 0, 1, bench.HostOps(), render_fn, count_fn, roofline=False)


def test_plain_run_times_the_steps_and_nothing_else():
    """Without --full the run is the warm-up and the K timed steps: no counted launches, no untimed
    passes (the accumulator holds exactly the W + K steps' frames), and the line holds the headline
    figures; --full adds the work counts and the roofline to the same headline keys."""
    import numpy as np
    from oracle import pyoracle
    counted = []
    wl, res = _tiny_run(["--steps", "3", "--warmup", "1", "--device-warmup-ms", "0"], counted)
    assert counted == [] and res["full"] is False
    assert res["steps"] == 3 and res["ms_per_step"] > 0 and res["value"] > 0
    assert res["unit"] == "ray-samples/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert res["metric"].endswith("at 64×36; ms/frame")
    assert abs(res["value"] - 64 * 36 * 3 * 8 / (res["ms_per_step"] * 1e-3)) <= 1e-9 * res["value"]
    assert "roofline" not in res and "segments_per_sample" not in res and "kernel_ms_event_pairs" not in res
    ref = pyoracle.render(64, 36, frame_first=1, nframes=4 * wl.spp, num_bounces=8, nthreads=2)
    acc = res["_accumulator"].numpy().reshape(36, 64, 3)
    assert np.array_equal(acc.view(np.uint32), ref.view(np.uint32))
    _, full = _tiny_run(["--steps", "3", "--warmup", "1", "--device-warmup-ms", "0", "--full"], counted)
    assert counted == [1 + wl.spp, 1 + 2 * wl.spp, 1 + 3 * wl.spp] and full["full"] is True
    assert full["roofline"]["frac"] > 0 and full["segments_per_sample"] > 0
    assert {k for k in res if k != "_accumulator"} <= set(full)


@pytest.mark.parametrize("full", [False, True])
def test_dump_outputs_is_the_last_timed_step_and_repeatable(tmp_path, full):
    """--dump-outputs writes the accumulator as the last timed step left it (not what --full's later
    passes add), in float32, and it does not depend on how many steps the device warm-up's time budget
    took: frames [1, 1 + (W + K) x spp) of a fresh accumulator."""
    import numpy as np
    from oracle import pyoracle
    imgs = []
    for i, budget in enumerate(["0", "30"]):
        argv = ["--steps", "2", "--warmup", "1", "--device-warmup-ms", budget, "--dump-outputs", str(tmp_path / str(i))]
        wl, res = _tiny_run(argv + (["--full"] if full else []), [])
        assert (res["device_warmup"]["steps"] > 0) == (budget != "0")
        assert [p.name for p in (tmp_path / str(i)).iterdir()] == ["image.npy"]
        imgs.append(np.load(tmp_path / str(i) / "image.npy"))
        assert res["outputs"]["arrays"]["image"]["shape"] == [36, 64, 3]
    ref = pyoracle.render(64, 36, frame_first=1, nframes=3 * wl.spp, num_bounces=8, nthreads=2)
    for img in imgs:
        assert img.dtype == np.float32 and img.shape == (36, 64, 3)
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))


def test_dump_outputs_samples_rows_of_a_large_image(tmp_path, monkeypatch):
    """An image above the size limit is written as the same seeded, sorted sample of its rows every time."""
    import numpy as np
    import torch
    img = torch.arange(40 * 8 * 3, dtype=torch.float32).reshape(40, 8, 3)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 10 * 8 * 3 * 4 + 5)
    a = bench.dump_outputs(tmp_path / "a", img)
    b = bench.dump_outputs(tmp_path / "b", img)
    assert a["arrays"] == b["arrays"] and a["arrays"]["image"]["sampled"]["rows"] == 10
    got = np.load(tmp_path / "a" / "image.npy")
    assert got.shape == (10, 8, 3) and got.nbytes <= bench.DUMP_MAX_BYTES
    assert np.array_equal(got, np.load(tmp_path / "b" / "image.npy"))
    rows = (got[:, 0, 0] / 24).astype(int)
    assert len(set(rows)) == 10 and list(rows) == sorted(rows) and np.array_equal(got, img.numpy()[rows])
