"""The launch plan's behavioural fingerprint (csrc/pt_launch_plan.h, applied by pt_capi.cpp launch_chain):
which chained launches restart the chain and which continue it, at the smallest geometry that is
scheduled at all -- 256 x 128 pixels, 512 tiles of 8 x 8 (kSchedMinTiles).

12 chained launches of 8 frames with a schedule build every 4 launches (PT_MI355_SCHED_REBUILD=4) at a
fixed occupancy (PT_MI355_CT_WAVES=5), so no decision depends on event timing: the first launch records
the tile costs, the second builds the schedule from them, every fourth launch after rebuilds it -- each
of these restarts the chain, every other launch continues it.  The image equals the oracle, and
pt_chain_counts reports exactly the counts recorded for this series on the commit before the launch
rules moved into pt_launch_plan.h: they are that commit's behaviour, which the rules must reproduce.
"""
from __future__ import annotations

import pytest

from conftest import bits_equal, mismatch_report
from oracle import pyoracle
from test_gpu_chain import _series, fresh  # noqa: F401  (fresh: the fixture)

pytestmark = pytest.mark.gpu

W, H, B, S, LAUNCHES = 256, 128, 8, 8, 12
ENVS = dict(PT_MI355_SCHED_REBUILD="4", PT_MI355_CT_WAVES="5")
# recorded on the parent commit (the hand-synchronised rules in pt_capi.cpp) for the series above
PARENT_DIFFUSE = {"restarts": 4, "continued": 8}
PARENT_V4 = {"restarts": 4, "continued": 8}


def test_diffuse_chain_counts_and_image(fresh):
    fresh(B, **ENVS)
    img, frames, counts = _series(W, H, B, S, LAUNCHES)
    print("diffuse chain counts:", counts)
    assert counts == PARENT_DIFFUSE, counts
    ref = pyoracle.render(W, H, nframes=frames, num_bounces=B)
    assert bits_equal(img, ref), mismatch_report(img, ref)


def test_v4_chain_counts_and_image(fresh):
    """The v4 renderer on its continuous-tiles kernel (PT_MI355_V4_CT=1: the work threshold would route
    this size to the per-tile kernel, whose launches never continue a chain)."""
    import cpuperformanceraytracer_amd as pt
    from cpuperformanceraytracer_amd.config import synthetic_env
    fresh(B, PT_MI355_V4_CT="1", **ENVS)
    env = synthetic_env()
    pt.v4_config(num_bounces=B)
    pt.set_env_map(env)
    img, frames, counts = _series(W, H, B, S, LAUNCHES, env=True, v4=True)
    print("v4 chain counts:", counts)
    assert counts == PARENT_V4, counts
    ref = pyoracle.render4(W, H, nframes=frames, num_bounces=B, env=env)
    assert bits_equal(img, ref), mismatch_report(img, ref)
