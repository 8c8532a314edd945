#!/usr/bin/env python3
"""A batch of small views: one pt_v4_render_device_views launch (A) against a launch per view (B).

Workload: 64 views of 256 x 144, 8 frames, 8 bounces, the default scene, the synthetic equirect map of
the benchmark (config.synthetic_env); the cameras on a circle around the scene, all looking down -z.
  A  one pt_v4_render_device_views launch
  B  64 x (pt_v4_set_camera + pt_v4_render_device) on one stream
Both are timed with device events around the whole batch and with the host clock over the same region
(enqueue only, then to the synchronise): B's cost is partly host work.  3 warm-up batches of each, then
`--batches` (>= 20) of each, interleaved A/B; the median and the spread (min, max, quartiles) of each.
Before timing, A's accumulators are compared bit for bit with B's.
Second line (no threshold): one 1920 x 1080 view, 8 frames: the views path (the per-tile kernel) against
pt_v4_render_device (continuous tiles).
One JSON line on stdout; --out FILE also writes it there."""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cpuperformanceraytracer_amd as pt  # noqa: E402
from cpuperformanceraytracer_amd import _native as N  # noqa: E402
from cpuperformanceraytracer_amd.config import synthetic_env  # noqa: E402
from cpuperformanceraytracer_amd.device import _job, _stream, set_env_map  # noqa: E402

BOUNCES, FRAMES = 8, 8


def circle(n: int, radius: float = 12.0, z: float = 40.0):
    """n cameras on a circle of `radius` in the plane z = 40, around the scene's axis; 90 degrees."""
    return [((radius * math.cos(2 * math.pi * k / n), radius * math.sin(2 * math.pi * k / n), z), 90.0) for k in range(n)]


def stats(xs):
    a = np.sort(np.asarray(xs, dtype=np.float64))
    return {"median": float(np.median(a)), "min": float(a[0]), "max": float(a[-1]), "q1": float(np.percentile(a, 25)),
            "q3": float(np.percentile(a, 75)), "n": int(a.size)}


class Lines:
    """The two ways to render `cams` at w x h into one [V, h, w, 3] buffer each, the ctypes calls prepared."""

    def __init__(self, cams, w, h):
        L = N.load()
        self.L, self.n = L, len(cams)
        self.st = _stream(None)
        self.buf_a = torch.zeros((self.n, h, w, 3), dtype=torch.float32, device="cuda:0")
        self.buf_b = torch.zeros_like(self.buf_a)
        self.job_a = _job(self.buf_a, w, h, 0, 1, self.n * h, 1, FRAMES, BOUNCES, N.PT_LAYOUT_INTERLEAVED, True)
        self.job_a.nrows = h
        self.cams = (N.PtV4Camera * self.n)(*[N.PtV4Camera((ctypes.c_float * 3)(*p), f) for p, f in cams])
        self.jobs_b = [_job(self.buf_b[v], w, h, 0, 1, h, 1, FRAMES, BOUNCES, N.PT_LAYOUT_INTERLEAVED, True) for v in range(self.n)]

    def a(self):
        N.check(self.L.pt_v4_render_device_views(ctypes.byref(self.job_a), self.cams, self.n, None, 0, self.st), "views")

    def b(self):
        for v in range(self.n):
            N.check(self.L.pt_v4_set_camera(ctypes.byref(self.cams[v])), "set_camera")
            N.check(self.L.pt_v4_render_device(ctypes.byref(self.jobs_b[v]), self.st), "render")

    def timed(self, fn):
        """(device ms between events around the batch, host ms to enqueue it, host ms to its completion)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        t1 = time.perf_counter()
        e1.synchronize()
        t2 = time.perf_counter()
        return e0.elapsed_time(e1), (t1 - t0) * 1e3, (t2 - t0) * 1e3

    def run(self, warmup, batches):
        for _ in range(warmup):
            self.a()
            self.b()
        torch.cuda.synchronize()
        ra, rb = [], []
        for _ in range(batches):
            ra.append(self.timed(self.a))
            rb.append(self.timed(self.b))
        pt.v4_camera()
        out = {}
        for name, r in (("A", ra), ("B", rb)):
            dev, enq, tot = zip(*r)
            out[name] = {"device_ms": stats(dev), "host_enqueue_ms": stats(enq), "host_total_ms": stats(tot)}
        out["A_over_B_device"] = out["A"]["device_ms"]["median"] / out["B"]["device_ms"]["median"]
        out["A_over_B_host_total"] = out["A"]["host_total_ms"]["median"] / out["B"]["host_total_ms"]["median"]
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--batches", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    pt.init(num_bounces=BOUNCES, device=0)
    pt.v4_config()
    set_env_map(synthetic_env(), 0, BOUNCES)

    small = Lines(circle(args.views), 256, 144)
    small.a()
    small.b()
    torch.cuda.synchronize()
    same = bool(torch.equal(small.buf_a.view(torch.int32), small.buf_b.view(torch.int32)))
    res = {"workload": {"views": args.views, "width": 256, "height": 144, "frames": FRAMES, "bounces": BOUNCES,
                        "scene": "default", "env": "synthetic equirect", "batches": args.batches, "warmup": args.warmup},
           "bit_equal_A_B": same, "small": small.run(args.warmup, args.batches)}
    del small
    big = Lines([((0.0, 0.0, 40.0), 90.0)], 1920, 1080)
    res["single_1080p"] = big.run(args.warmup, args.batches)
    pt.shutdown()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
