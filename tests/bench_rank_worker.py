"""Rank process for tests/test_bench_gloo.py::test_spawn_ranks_*: started by bench.spawn_ranks (the
`python bench.py --gpus N` entry without a launcher) with the environment it gives each rank, it runs
bench.run's N-rank path on CPU (gloo, the host clock, the oracle standing in for the GPU render) and
rank 0 prints one JSON line: the bench result plus the sha256 of its rendered rows.
Arguments: WIDTH HEIGHT SPP BOUNCES SCALING [FAIL_RANK]."""
from __future__ import annotations

import hashlib
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main() -> int:
    import torch.distributed as dist

    import bench
    from cpuperformanceraytracer_amd.config import Workload
    from oracle import pyoracle
    w, h, spp, b, scaling = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
    fail_rank = int(sys.argv[6]) if len(sys.argv) > 6 else -1
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    assert os.environ["MASTER_ADDR"] == "127.0.0.1" and int(os.environ["LOCAL_RANK"]) == rank
    if rank == fail_rank:
        return 3                                   # a rank that dies before the rendezvous
    dist.init_process_group("gloo")                # env:// rendezvous from spawn_ranks' variables
    try:
        wl = Workload("tiny", w, h, spp, b, scaling=scaling)
        args = bench.parse(["--gpus", str(world), "--steps", "2", "--warmup", "1", "--device-warmup-ms", "0",
                            "--full", "--verify-rows", "2"])

        def render_fn(buf, W, H, f, n, rs, st, nr):
            pyoracle.render(W, H, frame_first=f, nframes=n, num_bounces=b, row_start=rs, row_stride=st, nrows=nr,
                            nthreads=2, buf=buf.numpy())

        def count_fn(buf, W, H, f, n, rs, st, nr):
            render_fn(buf, W, H, f, n, rs, st, nr)
            _, c = pyoracle.render_counted(W, H, frame_first=f, nframes=n, num_bounces=b, row_start=rs,
                                           row_stride=st, nrows=nr)
            return {"segments": c["segments"], "samples": c["samples"], "escaped": c["escaped"],
                    "lane_slots": c["segments"], "primary": c["samples"]}

        res = bench.run(args, wl, rank, world, bench.HostOps(), render_fn, count_fn, roofline=False)
        if rank == 0:
            acc = res.pop("_accumulator").numpy()
            res["acc_sha256"] = hashlib.sha256(acc.tobytes()).hexdigest()
            print(json.dumps(res))
    finally:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
