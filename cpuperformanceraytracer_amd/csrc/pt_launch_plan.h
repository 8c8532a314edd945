// pt_launch_plan.h -- the rules that turn a job into a launch, each once, as functions
// of plain inputs: pt_capi.cpp and the host check (tests/native/check_launch_plan.cpp) share them.
// back_pct: a launch's default back-claim share; back_set: PT_MI355_BACK was given.
#pragma once
#include <stdint.h>

constexpr uint32_t kSchedMinTiles = 512;   // smaller jobs (e.g. one RenderTile) are not scheduled

// The schedule builder's tile split factor (PT_MI355_SPLIT; 0: whole tiles) of a diffuse launch.  Split
// tiles: launches of one 8-frame chunk (a tile's half of several chunks is a short chunk each, and the
// pool's two chunk contexts then wait on each other: 1080p 16 spp 0.452 vs 0.437 ms)
constexpr uint32_t pt_plan_split(int32_t nframes, uint32_t split) { return nframes <= 8 ? split : 0u; }
// The default back-claim share (PT_MI355_BACK, 20): the last-dispatched fifth of the grid (each CU's 5th
// block, the slowest under the SQ's oldest-first issue) claims the cheapest units, for launches of <= 16
// frames, whose end is a large part of them (A/B, scripts/gpu_ab.sh, 20 % vs none: 1080p 8 spp 0.2533
// vs 0.2561 ms, env 16 spp 0.4967 vs 0.5030, 4K 8 spp 0.8217 vs 0.8309; 4K 64 spp 5.913 vs 5.763: not there)
constexpr uint32_t pt_plan_back(int32_t nframes, uint32_t back_pct) { return nframes <= 16 ? back_pct : 0u; }

// What launch number `launches` (from 0) of a geometry does to its schedule.  It (re)builds it from the
// last launch's costs on the 2nd launch and then every `rebuild` launches (the costs of a fixed view
// barely change; the builder is a one-workgroup kernel of ~57 us at 1080p).  Its kernel records the
// tiles' costs only when the next launch builds from them (one 4-B store per tile is a 32-B HBM write:
// ~1 MB per 1080p launch otherwise).
struct PtSchedStep { bool builds, records; };
constexpr PtSchedStep pt_plan_sched_step(bool have_cost, bool built, unsigned long long launches, unsigned long long rebuild)
{
    const bool builds = have_cost && (!built || launches % rebuild == 0);
    return {builds, !(built || builds) || (launches + 1) % rebuild == 0};
}

// The launch variant of a continuous-tiles launch (diffuse and env kernels): PtJob::ct_wide (5 or 6 waves per SIMD) and
// PtJob::ct_back_pct.  PT_MI355_CT_WAVES=5|6 fixes the occupancy (and the env share); by default (0) the geometry's first
// scheduled launches time the ARMS and the fastest is kept (per stream: a geometry's Sched):
//   arm 0: 5 waves, arm 1: 6 waves -- each with the default back-claim share (20 %) -- and, for
//   launches that take back claims (<= 16 frames) unless PT_MI355_BACK is given, arm 2: 6 waves with
//   kBackWide % of the grid claiming from the back.  Measured (profiles/r05/r05i_back_sweep_ab.jsonl,
//   r05h_back_ab.jsonl): at 6 waves 45 % gave 1080p 8 spp 0.2392 vs 0.2440 ms and 4K 8 spp 0.8015 vs
//   0.8395 (55-90 %: 0.249 / 0.80), but 720p 0.1490 vs 0.1462 and, at 5 waves, 1080p 0.2526 vs 0.2488 --
//   so it is one more timed arm, not a new default.
// The env kernel has one occupancy (PT_ENV_WAVES); its arms, for launches that take back claims unless
//   PT_MI355_BACK is given, are the back-claim shares 20 (default), 33 and 45 %: measured
//   (profiles/r05/r05k_env_back_ab.jsonl) 1080p 8 frames 0.2786 / 0.2809 / 0.2738 ms, 16 frames
//   0.4821 / 0.4770 / 0.4885 -- the best share depends on the launch, as for the diffuse kernel.
// The arms are timed in a palindromic order (ABBA, ABCCBA), three rounds of which the first is not
// counted: the clocks of a fresh process ramp up over its first launches -- a plain
// alternation favoured the later arm, and one round of ABCCBA still picked 5 waves for 4K 8 spp in
// one of two runs (0.8242 vs 0.8023 ms, profiles/r05/r05j_timing3_ab.jsonl).  Until the pick: 6
// waves for launches of several chunks (ahead at 16 and 64 spp), 5 for one-chunk launches.  No pixel
// depends on the variant (tests/test_gpu_regime.py forces grid changes).
constexpr uint32_t kBackWide = 45;
constexpr uint32_t kEnvBack[3] = {0, 33, 45};   // env arms 1, 2 (arm 0: the default share)
constexpr uint32_t kTuneRounds = 3;   // rounds of the palindromic arm order timed; the first is discarded
// Whether an env launch has arms (else it runs the fixed variant); the arms a geometry's first timed launch fixes.
constexpr bool pt_plan_env_arms(bool env, uint32_t back_pct, bool back_set) { return env && back_pct != 0 && !back_set; }
constexpr uint32_t pt_plan_narms(bool env, uint32_t back_pct, bool back_set) { return (env || (back_pct != 0 && !back_set)) ? 3u : 2u; }
// Timed launches per round and in all; the arm of timed launch t (the sums skip the first round).
constexpr uint32_t pt_plan_round_launches(uint32_t narms) { return narms == 3 ? 6u : 4u; }
constexpr uint32_t pt_plan_tune_launches(uint32_t narms) { return narms ? kTuneRounds * pt_plan_round_launches(narms) : 0u; }
constexpr int pt_plan_arm_of(uint32_t narms, uint32_t t)
{
    constexpr int order3[6] = {0, 1, 2, 2, 1, 0};
    return narms == 3 ? order3[t % 6] : (int)((t ^ (t >> 1)) & 1u);
}
// The arm of a launch while the timed ones are outstanding, or of one that is not timeable.
constexpr int pt_plan_interim_arm(bool env, int32_t nframes) { return env || nframes <= 8 ? 0 : 1; }
// What an arm means to a launch -- what ct_occupancy applies and pt_launch_variant reports.  The env kernel
// has one occupancy: its arms are shares.  Arm 2 of the diffuse kernel and the env arms mean something
// only to launches that take them (above): any other launch of the geometry keeps its default share.
struct PtVariant { uint32_t wide, back_pct; };
constexpr PtVariant pt_plan_variant(bool env, int arm, uint32_t back_pct, bool back_set)
{
    if (env) return {0u, arm && pt_plan_env_arms(env, back_pct, back_set) ? kEnvBack[arm] : back_pct};
    return {arm != 0 ? 1u : 0u, arm == 2 && back_pct != 0 ? kBackWide : back_pct};
}

// A continuing chained launch that takes back claims (<= 16 frames) takes ALL its dynamic units from
// the back (cheapest first, after each wave's static first unit): its tail overlaps the next launch,
// so the launch-end balancing of the timed share no longer pays, and the reversed order measured faster
// (3 interleaved rounds, profiles/r06/r06u_*: c2 0.2180 vs 0.2207 ms at the timed 45 %, v4 0.3302 vs
// 0.3468 at its 20 %; the env kernel showed no difference, r06v: it keeps its timed share).  Launches of
// more frames keep claiming from the front (4K 64 spp 5.55 vs 5.62 ms with back claims, r06x).
constexpr uint32_t kChainBack = 100;   // (diffuse, env: from the variant's share; v4: from the configured one)
constexpr uint32_t pt_plan_chain_back(bool env, uint32_t variant_back_pct, bool back_set)
{
    return variant_back_pct != 0 && !env && !back_set ? kChainBack : variant_back_pct;
}
constexpr uint32_t pt_plan_chain_back_v4(int32_t nframes, uint32_t back_pct, bool back_set)
{
    return nframes <= 16 ? (back_set ? back_pct : kChainBack) : 0u;
}

// The camera-hit cache of a geometry (pt_camcache.h).  kCamEmpty; kCamFilled: the geometry's last launch
// filled it (the next launch is stream-ordered after it: a chained one restarts); kCamSettled: every
// later launch may read it
enum : uint8_t { kCamEmpty = 0, kCamFilled = 1, kCamSettled = 2 };
// Launches of fewer frames neither fill nor use a cache, and move no cache state.  A tile of such a
// launch carries few items, and the record load at the tile's start -- a dependent HBM / MALL access
// right after the claim's atomic -- then costs more than the coherent camera trace it replaces.
// Measured at 1920 x 1080, parent vs cache for every length (profiles/camcache): 1 frame per launch
// 0.1142 -> 0.1168 ms (+2.3 %), 8 frames 0.2198 -> 0.2169 (-1.3 %), 16 (env) and 64 (4K) -0.5 %.  The
// bound is the shortest length measured to gain, one whole chunk (kChunk, pt_kernel.hip).
constexpr int32_t kCamMinFrames = 8;   // (wanted: pt_cam_cache_wanted; cam_off: the allocation failed)
constexpr bool pt_cam_launch_qualifies(bool cam_off, int32_t nframes, bool wanted)
{
    return !cam_off && nframes >= kCamMinFrames && wanted;
}
// A chained launch may continue the overlap unless it would fill the cache or read records that a
// launch it may overlap is still writing.
constexpr bool pt_cam_chain_may_continue(bool qualifies, bool have_cache, uint8_t cam_state)
{
    return !qualifies || (have_cache && cam_state == kCamSettled);
}
// Whether a chained launch CONTINUES the live chain (launch_chain; else it restarts it): the chain is this
// geometry's, its schedule is built and not rebuilt now, the variant is settled, the camera cache allows it.
// Known defect, kept: a chained v4 launch of fewer than 8 frames runs the per-tile kernel, which ignores
// the tile epochs, yet may continue a live chain.  The fix is one more input here; it
// changes which launches restart and needs its own GPU test.
constexpr bool pt_plan_chain_continues(bool same_geometry, bool built, bool builds, bool variant_fixed, bool cam_may_continue)
{
    return same_geometry && built && !builds && variant_fixed && cam_may_continue;
}
