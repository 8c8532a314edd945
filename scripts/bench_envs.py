#!/usr/bin/env python3
"""A batch of small views under as many env maps: one pt_v4_render_device_envs launch (A) against what a
caller does without it (B), and against one pt_v4_render_device_scenes launch with ONE shared texture (C,
the kernel the envs kernel was made from).

Workload: 64 views of 256 x 144, 8 frames, 8 bounces, InitializeScene's scene, the cameras of
scripts/bench_views.py, 64 synthetic equirect maps of 512 x 256 (config.synthetic_env, a seed per view).
  A  one pt_v4_render_device_envs launch: an env set of the 64 maps, made once outside the timed region
  B  64 x (pt_set_env_map + pt_v4_set_camera + pt_v4_render_device) on one stream
  C  one pt_v4_render_device_scenes launch of the 64 cameras, every view under map 0 (pt_set_env_map's)
Each is timed with device events around the whole batch and with the host clock over the same region, as
scripts/bench_scenes.py does; `--warmup` batches of each, then `--batches` (>= 20) of each, interleaved
A/B/C; the median and the spread of each.  Before timing, A's accumulators are compared bit for bit with
B's.  A - C is the price of a texture per view.
One JSON line on stdout; --out FILE also writes it there."""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cpuperformanceraytracer_amd as pt  # noqa: E402
from bench_views import circle, stats  # noqa: E402
from cpuperformanceraytracer_amd import _native as N  # noqa: E402
from cpuperformanceraytracer_amd.config import synthetic_env  # noqa: E402
from cpuperformanceraytracer_amd.device import _job, _stream, make_v4_env_set, v4_scene_desc  # noqa: E402

BOUNCES, FRAMES, W, H = 8, 8, 256, 144
ENV_H, ENV_W = 256, 512


class Lines:
    def __init__(self, cams, texs):
        L = N.load()
        self.L, self.n = L, len(cams)
        self.st = _stream(None)
        self.bufs = {k: torch.zeros((self.n, H, W, 3), dtype=torch.float32, device="cuda:0") for k in "ABC"}
        self.job = {}
        for k in "AC":
            self.job[k] = _job(self.bufs[k], W, H, 0, 1, self.n * H, 1, FRAMES, BOUNCES, N.PT_LAYOUT_INTERLEAVED, True)
            self.job[k].nrows = H
        self.cams = (N.PtV4Camera * self.n)(*[N.PtV4Camera((ctypes.c_float * 3)(*p), f) for p, f in cams])
        self.jobs_b = [_job(self.bufs["B"][v], W, H, 0, 1, H, 1, FRAMES, BOUNCES, N.PT_LAYOUT_INTERLEAVED, True) for v in range(self.n)]
        self.texs = [np.ascontiguousarray(t, np.float32) for t in texs]
        self.ptex = [N.PtTexture(t.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), t.shape[1], t.shape[0], 3) for t in self.texs]
        self.envs = make_v4_env_set(self.texs)
        self.scene = (N.PtV4SceneDesc * 1)(v4_scene_desc(pt.v4_get_scene_desc()))
        self.zeros = (ctypes.c_int32 * self.n)()

    def a(self):
        N.check(self.L.pt_v4_render_device_envs(ctypes.byref(self.job["A"]), self.envs.handle, None, None, 0, None, self.cams, self.n,
                                                None, 0, self.st), "envs")

    def b(self):
        L = self.L
        for v in range(self.n):
            N.check(L.pt_set_env_map(ctypes.byref(self.ptex[v])), "set_env_map")
            N.check(L.pt_v4_set_camera(ctypes.byref(self.cams[v])), "set_camera")
            N.check(L.pt_v4_render_device(ctypes.byref(self.jobs_b[v]), self.st), "render")

    def c(self):
        N.check(self.L.pt_v4_render_device_scenes(ctypes.byref(self.job["C"]), self.scene, 1, self.cams, self.zeros, self.n, None, 0,
                                                  self.st), "scenes")

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

    def round(self, rec=None):
        for name, fn in (("A", self.a), ("B", self.b), ("C", self.c)):
            if name == "C":   # (B left its last map behind; C renders under map 0)
                N.check(self.L.pt_set_env_map(ctypes.byref(self.ptex[0])), "set_env_map")
            r = self.timed(fn)
            if rec is not None:
                rec[name].append(r)
        pt.v4_camera()

    def run(self, warmup, batches):
        for _ in range(warmup):
            self.round()
        rec = {"A": [], "B": [], "C": []}
        for _ in range(batches):
            self.round(rec)
        out = {}
        for name, r in rec.items():
            dev, enq, tot = zip(*r)
            out[name] = {"device_ms": stats(dev), "host_enqueue_ms": stats(enq), "host_total_ms": stats(tot)}
        out["A_over_B_device"] = out["A"]["device_ms"]["median"] / out["B"]["device_ms"]["median"]
        out["A_over_B_host_total"] = out["A"]["host_total_ms"]["median"] / out["B"]["host_total_ms"]["median"]
        out["A_over_C_device"] = out["A"]["device_ms"]["median"] / out["C"]["device_ms"]["median"]
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
    pt.InitializeScene()

    lines = Lines(circle(args.views), [synthetic_env(ENV_H, ENV_W, 1000 + v) for v in range(args.views)])
    lines.a()
    lines.b()
    torch.cuda.synchronize()
    same = bool(torch.equal(lines.bufs["A"].view(torch.int32), lines.bufs["B"].view(torch.int32)))
    res = {"workload": {"views": args.views, "width": W, "height": H, "frames": FRAMES, "bounces": BOUNCES, "scene": "default",
                        "envs": f"{args.views} synthetic equirect {ENV_W}x{ENV_H}", "batches": args.batches,
                        "warmup": args.warmup, "lib": str(N.lib_path().name)},
           "bit_equal_A_B": same, "small": lines.run(args.warmup, args.batches)}
    lines.envs.close()
    pt.shutdown()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
