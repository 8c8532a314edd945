#!/usr/bin/env python3
"""A batch of small views with a frame range per view: one pt_v4_render_device_batch launch against the envs
call it was made from, and -- with uneven ranges -- against what a caller does without it.

Workload: 64 views of 256 x 144, 8 bounces, InitializeScene's scene, the cameras of scripts/bench_views.py,
64 synthetic equirect maps of 512 x 256 (config.synthetic_env, a seed per view), one env set made once
outside the timed region.
  A  one pt_v4_render_device_batch launch, every range (1, 8)
  C  one pt_v4_render_device_envs launch on the same inputs (frame_first 1, nframes 8): A / C is the price of
     the range per view
  M  one pt_v4_render_device_batch launch with mixed counts, nframes[v] = 1 + v % 16, and decorrelated first
     frames, frame_first[v] = 1 + (v * 7919) % 1000
  B  M's views set and launched one by one: 64 x (pt_set_env_map + pt_v4_set_camera + pt_v4_render_device)
Each is timed with device events around the whole batch and with the host clock over the same region, as
scripts/bench_envs.py does; `--warmup` batches of each, then `--batches` (>= 20) of each, interleaved
A/C/M/B; the median and the spread of each.  Before timing, A's accumulators are compared bit for bit with
C's, and M's with B's.
One JSON line on stdout; --out FILE also writes it there.

--stats: the statistics leg instead (pt_v4_render_device_batch_stats), on A's inputs, interleaved A/S/P/Q/T:
  A  the plain batch call, no pixels (the yardstick; with PT_MI355_LIB naming a library of an earlier revision
     that lacks the statistics call, A alone is timed -- run the two alternately to compare revisions)
  S  the statistics call, no pixels
  P  the plain batch call writing pixels          Q  the statistics call writing pixels
  T  what a caller does without it: pt_tonemap_device of all slices before, the plain call, pt_tonemap_device
     after, and a torch reduction per view of the two pixel sets (sum, changed, max over R, G, B)
Before timing, S's accumulators are compared bit for bit with A's and S's records with T's reduction."""
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
from cpuperformanceraytracer_amd.device import _job, _stream, make_v4_env_set  # noqa: E402

BOUNCES, FRAMES, W, H = 8, 8, 256, 144
ENV_H, ENV_W = 256, 512


def mixed(n):
    return [(1 + (v * 7919) % 1000, 1 + v % 16) for v in range(n)]


class Lines:
    def __init__(self, cams, texs):
        L = N.load()
        self.L, self.n = L, len(cams)
        self.st = _stream(None)
        self.bufs = {k: torch.zeros((self.n, H, W, 3), dtype=torch.float32, device="cuda:0") for k in "ACMB"}
        self.job = {}
        for k in "ACM":
            self.job[k] = _job(self.bufs[k], W, H, 0, 1, self.n * H, 1, FRAMES, BOUNCES, N.PT_LAYOUT_INTERLEAVED, True)
            self.job[k].nrows = H
        self.cams = (N.PtV4Camera * self.n)(*[N.PtV4Camera((ctypes.c_float * 3)(*p), f) for p, f in cams])
        self.mixed = mixed(self.n)
        self.jobs_b = [_job(self.bufs["B"][v], W, H, 0, 1, H, ff, nf, BOUNCES, N.PT_LAYOUT_INTERLEAVED, True)
                       for v, (ff, nf) in enumerate(self.mixed)]
        self.texs = [np.ascontiguousarray(t, np.float32) for t in texs]
        self.ptex = [N.PtTexture(t.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), t.shape[1], t.shape[0], 3) for t in self.texs]
        self.envs = make_v4_env_set(self.texs)
        self.ranges = {"A": (N.PtV4FrameRange * self.n)(*[N.PtV4FrameRange(1, FRAMES) for _ in range(self.n)]),
                       "M": (N.PtV4FrameRange * self.n)(*[N.PtV4FrameRange(ff, nf) for ff, nf in self.mixed])}
        self.batch = {}
        for k in "AM":
            b = N.PtV4Batch()
            b.cams, b.nviews, b.frames, b.envs = self.cams, self.n, self.ranges[k], self.envs.handle
            self.batch[k] = b

    def a(self):
        N.check(self.L.pt_v4_render_device_batch(ctypes.byref(self.job["A"]), ctypes.byref(self.batch["A"]), self.st), "batch")

    def m(self):
        N.check(self.L.pt_v4_render_device_batch(ctypes.byref(self.job["M"]), ctypes.byref(self.batch["M"]), self.st), "batch")

    # ---- the statistics leg (--stats): all on buffer A / batch A ----
    def stats_setup(self):
        self.have_stats = hasattr(self.L, "pt_v4_render_device_batch_stats")
        self.rec = torch.zeros((self.n, 4), dtype=torch.int32, device="cuda:0")
        self.pix = torch.zeros((2, self.n, H, W), dtype=torch.int32, device="cuda:0")
        self.batch["P"] = N.PtV4Batch()
        ctypes.memmove(ctypes.byref(self.batch["P"]), ctypes.byref(self.batch["A"]), ctypes.sizeof(N.PtV4Batch))
        self.batch["P"].pixels, self.batch["P"].format = self.pix[1].data_ptr(), N.PT_PIXEL_XRGB8

    def s(self):
        N.check(self.L.pt_v4_render_device_batch_stats(ctypes.byref(self.job["A"]), ctypes.byref(self.batch["A"]), self.rec.data_ptr(),
                                                       self.st), "batch_stats")

    def p(self):
        N.check(self.L.pt_v4_render_device_batch(ctypes.byref(self.job["A"]), ctypes.byref(self.batch["P"]), self.st), "batch")

    def q(self):
        N.check(self.L.pt_v4_render_device_batch_stats(ctypes.byref(self.job["A"]), ctypes.byref(self.batch["P"]), self.rec.data_ptr(),
                                                       self.st), "batch_stats")

    def t(self):
        tone = lambda k: N.check(self.L.pt_tonemap_device(self.bufs["A"].data_ptr(), W, self.n * H, N.PT_LAYOUT_INTERLEAVED, 0, 0,
                                                          self.pix[k].data_ptr(), N.PT_PIXEL_XRGB8, self.st), "tonemap")
        tone(0)
        self.a()
        tone(1)
        ch = torch.stack([(self.pix >> sh) & 255 for sh in (16, 8, 0)], -1)   # 2 x n x H x W x 3
        d = (ch[1] - ch[0]).abs().reshape(self.n, -1, 3)
        self.t_rec = torch.stack([d.sum((1, 2)), (d.amax(2) > 0).sum(1), d.amax((1, 2))], 1)   # n x 3 int64

    def run_stats(self, warmup, batches):
        legs = [("A", self.a)] + ([("S", self.s), ("P", self.p), ("Q", self.q), ("T", self.t)] if self.have_stats else [])
        rec = {k: [] for k, _ in legs}
        for i in range(warmup + batches):
            for name, fn in legs:
                self.bufs["A"].zero_()   # (every leg renders frames 1..8 from zeros: the same work and the same records)
                r = self.timed(fn)
                if i >= warmup:
                    rec[name].append(r)
        out = {}
        for name, r in rec.items():
            dev, enq, tot = zip(*r)
            out[name] = {"device_ms": stats(dev), "host_enqueue_ms": stats(enq), "host_total_ms": stats(tot)}
        med = {k: out[k]["device_ms"]["median"] for k in out}
        if self.have_stats:
            out["S_over_A_device"] = med["S"] / med["A"]
            out["Q_over_P_device"] = med["Q"] / med["P"]
            out["T_over_A_device"] = med["T"] / med["A"]
            out["T_over_S_device"] = med["T"] / med["S"]
        return out

    def c(self):
        N.check(self.L.pt_v4_render_device_envs(ctypes.byref(self.job["C"]), self.envs.handle, None, None, 0, None, self.cams, self.n,
                                                None, 0, self.st), "envs")

    def b(self):
        L = self.L
        for v in range(self.n):
            N.check(L.pt_set_env_map(ctypes.byref(self.ptex[v])), "set_env_map")
            N.check(L.pt_v4_set_camera(ctypes.byref(self.cams[v])), "set_camera")
            N.check(L.pt_v4_render_device(ctypes.byref(self.jobs_b[v]), self.st), "render")

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
        for name, fn in (("A", self.a), ("C", self.c), ("M", self.m), ("B", self.b)):
            r = self.timed(fn)
            if rec is not None:
                rec[name].append(r)
        pt.v4_camera()

    def run(self, warmup, batches):
        for _ in range(warmup):
            self.round()
        rec = {k: [] for k in "ACMB"}
        for _ in range(batches):
            self.round(rec)
        out = {}
        for name, r in rec.items():
            dev, enq, tot = zip(*r)
            out[name] = {"device_ms": stats(dev), "host_enqueue_ms": stats(enq), "host_total_ms": stats(tot)}
        med = {k: out[k]["device_ms"]["median"] for k in out}
        out["A_over_C_device"] = med["A"] / med["C"]
        out["M_over_B_device"] = med["M"] / med["B"]
        out["M_over_B_host_total"] = out["M"]["host_total_ms"]["median"] / out["B"]["host_total_ms"]["median"]
        out["M_over_A_device"] = med["M"] / med["A"]
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--batches", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--stats", action="store_true", help="the statistics leg (see the module text)")
    args = ap.parse_args()
    pt.init(num_bounces=BOUNCES, device=0)
    pt.v4_config()
    pt.InitializeScene()

    lines = Lines(circle(args.views), [synthetic_env(ENV_H, ENV_W, 1000 + v) for v in range(args.views)])
    if args.stats:
        return main_stats(args, lines)
    for fn in (lines.a, lines.c, lines.m, lines.b):
        fn()
    torch.cuda.synchronize()
    bits = {k: b.view(torch.int32) for k, b in lines.bufs.items()}
    same_ac, same_mb = bool(torch.equal(bits["A"], bits["C"])), bool(torch.equal(bits["M"], bits["B"]))
    res = {"workload": {"views": args.views, "width": W, "height": H, "frames_A_C": FRAMES, "frames_M_B": "1 + v % 16",
                        "frame_first_M_B": "1 + (v * 7919) % 1000", "frames_total_M": sum(n for _, n in lines.mixed),
                        "bounces": BOUNCES, "scene": "default", "envs": f"{args.views} synthetic equirect {ENV_W}x{ENV_H}",
                        "batches": args.batches, "warmup": args.warmup, "lib": str(N.lib_path().name)},
           "bit_equal_A_C": same_ac, "bit_equal_M_B": same_mb, "small": lines.run(args.warmup, args.batches)}
    lines.envs.close()
    pt.shutdown()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0 if same_ac and same_mb else 1


def main_stats(args, lines):
    lines.stats_setup()
    res = {"workload": {"views": args.views, "width": W, "height": H, "frames": FRAMES, "bounces": BOUNCES, "scene": "default",
                        "envs": f"{args.views} synthetic equirect {ENV_W}x{ENV_H}", "start": "zeros, every timed call",
                        "batches": args.batches, "warmup": args.warmup, "lib": str(N.lib_path().name)},
           "has_stats_call": lines.have_stats}
    ok = True
    if lines.have_stats:
        lines.a()
        torch.cuda.synchronize()
        plain = lines.bufs["A"].clone()
        lines.bufs["A"].zero_()
        lines.s()
        torch.cuda.synchronize()
        same = bool(torch.equal(plain.view(torch.int32), lines.bufs["A"].view(torch.int32)))
        got = lines.rec.cpu().numpy().view(np.dtype([("s", "<u8"), ("c", "<u4"), ("m", "<u4")])).reshape(-1)
        lines.bufs["A"].zero_()
        lines.t()
        torch.cuda.synchronize()
        want = lines.t_rec.cpu().numpy()
        agree = bool((got["s"] == want[:, 0]).all() and (got["c"] == want[:, 1]).all() and (got["m"] == want[:, 2]).all())
        res.update({"bit_equal_S_A": same, "records_equal_S_T": agree, "records_sum_delta_total": int(got["s"].sum())})
        ok = same and agree
    res["small"] = lines.run_stats(args.warmup, args.batches)
    lines.envs.close()
    pt.shutdown()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
