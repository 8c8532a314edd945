// tests/native/check_launch_plan.cpp -- host check of the launch rules (csrc/pt_launch_plan.h, applied
// by pt_capi.cpp): every expectation below is written out, none is computed by the header.
// usage: check_launch_plan     exit 0 iff every check holds
#include <stdint.h>
#include <stdio.h>

#include "pt_launch_plan.h"

static int fails = 0;
#define CHECK(c) \
    do { \
        if (!(c)) { \
            printf("FAILED line %d: %s\n", __LINE__, #c); \
            ++fails; \
        } \
    } while (0)

static bool variant_is(bool env, int arm, uint32_t back, bool back_set, uint32_t wide, uint32_t want_back)
{
    const PtVariant v = pt_plan_variant(env, arm, back, back_set);
    return v.wide == wide && v.back_pct == want_back;
}

int main()
{
    // ---- per-launch constants: split factor 1 (the default) and 3, share 20 (the default) and 45
    const int32_t frames[6] = {1, 8, 9, 16, 17, 64};
    const uint32_t split1[6] = {1, 1, 0, 0, 0, 0}, split3[6] = {3, 3, 0, 0, 0, 0};
    const uint32_t back20[6] = {20, 20, 20, 20, 0, 0}, back45[6] = {45, 45, 45, 45, 0, 0};
    for (int i = 0; i < 6; ++i) {
        CHECK(pt_plan_split(frames[i], 1) == split1[i]);
        CHECK(pt_plan_split(frames[i], 3) == split3[i]);
        CHECK(pt_plan_split(frames[i], 0) == 0);
        CHECK(pt_plan_back(frames[i], 20) == back20[i]);
        CHECK(pt_plan_back(frames[i], 45) == back45[i]);
        CHECK(pt_plan_back(frames[i], 0) == 0);
    }
    CHECK(kSchedMinTiles == 512 && kBackWide == 45 && kEnvBack[1] == 33 && kEnvBack[2] == 45 && kChainBack == 100);
    CHECK(kTuneRounds == 3 && kCamMinFrames == 8);

    // ---- the schedule step over launches 0 .. 600, as use_sched and launch_chain apply it
    const unsigned long long rebuilds[5] = {1, 2, 4, 64, 256};
    const int want_builds[5] = {600, 301, 151, 10, 3};   // launch 1, then every multiple of `rebuild` from 2 on
    for (int r = 0; r < 5; ++r) {
        bool have_cost = false, built = false, prev_recorded = false;
        bool recorded[601];
        bool builds_at[602] = {};
        int builds = 0;
        for (unsigned long long n = 0; n <= 600; ++n) {
            const PtSchedStep s = pt_plan_sched_step(have_cost, built, n, rebuilds[r]);
            if (n == 0) CHECK(s.records && !s.builds);   // the first launch records
            if (n == 1) CHECK(s.builds);                 // the second builds
            if (s.builds) CHECK(prev_recorded);          // never from costs that were not recorded
            builds_at[n] = s.builds;
            builds += s.builds;
            built = built || s.builds;
            have_cost = have_cost || s.records;
            recorded[n] = prev_recorded = s.records;
        }
        // no other launch records: only the first, and one whose successor builds (launch 601 would
        // build exactly when 601 is a multiple of `rebuild`: for 1 only)
        builds_at[601] = rebuilds[r] == 1;
        for (int n = 1; n <= 600; ++n) CHECK(recorded[n] == builds_at[n + 1]);
        CHECK(builds == want_builds[r]);
    }

    // ---- the arms
    const int abba[12] = {0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0};
    const int abccba[18] = {0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0};
    CHECK(pt_plan_round_launches(2) == 4 && pt_plan_tune_launches(2) == 12);
    CHECK(pt_plan_round_launches(3) == 6 && pt_plan_tune_launches(3) == 18);
    CHECK(pt_plan_tune_launches(0) == 0);   // (not started: nothing is timed yet)
    for (uint32_t t = 0; t < 12; ++t) CHECK(pt_plan_arm_of(2, t) == abba[t]);
    for (uint32_t t = 0; t < 18; ++t) CHECK(pt_plan_arm_of(3, t) == abccba[t]);
    // the sums start after the first round (launch 4 or 6) and then hold every arm equally often: 4
    for (uint32_t narms = 2; narms <= 3; ++narms) {
        int n[3] = {0, 0, 0};
        CHECK(pt_plan_round_launches(narms) == (narms == 2 ? 4u : 6u));
        for (uint32_t t = pt_plan_round_launches(narms); t < pt_plan_tune_launches(narms); ++t) ++n[pt_plan_arm_of(narms, t)];
        CHECK(n[0] == 4 && n[1] == 4 && n[2] == (narms == 3 ? 4 : 0));
    }
    // how many arms: 3 for launches that take back claims unless PT_MI355_BACK is given, and for env launches
    CHECK(pt_plan_narms(false, 20, false) == 3 && pt_plan_narms(false, 0, false) == 2 && pt_plan_narms(false, 30, true) == 2);
    CHECK(pt_plan_narms(true, 20, false) == 3);
    CHECK(pt_plan_env_arms(true, 20, false) && !pt_plan_env_arms(true, 0, false) && !pt_plan_env_arms(true, 30, true));
    CHECK(!pt_plan_env_arms(false, 20, false));
    // until the pick: 5 waves for one-chunk launches, 6 for longer ones; env: the default share
    CHECK(pt_plan_interim_arm(false, 1) == 0 && pt_plan_interim_arm(false, 8) == 0 && pt_plan_interim_arm(false, 9) == 1);
    CHECK(pt_plan_interim_arm(false, 64) == 1 && pt_plan_interim_arm(true, 8) == 0 && pt_plan_interim_arm(true, 16) == 0);
    // arm -> (wide, back), the one table ct_occupancy applies and pt_launch_variant reports (waves = wide ? 6 : 5).
    // diffuse with the default share, without back claims (a 64-frame launch), with PT_MI355_BACK=30 (two arms)
    CHECK(variant_is(false, 0, 20, false, 0, 20) && variant_is(false, 1, 20, false, 1, 20) && variant_is(false, 2, 20, false, 1, 45));
    CHECK(variant_is(false, 0, 0, false, 0, 0) && variant_is(false, 1, 0, false, 1, 0) && variant_is(false, 2, 0, false, 1, 0));
    CHECK(variant_is(false, 0, 30, true, 0, 30) && variant_is(false, 1, 30, true, 1, 30));
    // env: one occupancy, the shares 20 / 33 / 45; a launch without arms (no back claims, or PT_MI355_BACK=30)
    // keeps its share whatever the geometry's pick
    CHECK(variant_is(true, 0, 20, false, 0, 20) && variant_is(true, 1, 20, false, 0, 33) && variant_is(true, 2, 20, false, 0, 45));
    CHECK(variant_is(true, 0, 0, false, 0, 0) && variant_is(true, 1, 0, false, 0, 0) && variant_is(true, 2, 0, false, 0, 0));
    CHECK(variant_is(true, 0, 30, true, 0, 30) && variant_is(true, 1, 30, true, 0, 30) && variant_is(true, 2, 30, true, 0, 30));
    // the same, from the frame counts pt_launch_variant sees: 8 diffuse, 16 env, 64 (no back claims)
    const int rep_waves[3] = {5, 6, 6}, rep_back[3] = {20, 20, 45}, rep_env_back[3] = {20, 33, 45};
    for (int pick = 0; pick < 3; ++pick) {
        const PtVariant d = pt_plan_variant(false, pick, pt_plan_back(8, 20), false);
        CHECK((d.wide ? 6 : 5) == rep_waves[pick] && (int)d.back_pct == rep_back[pick]);
        CHECK((int)pt_plan_variant(true, pick, pt_plan_back(16, 20), false).back_pct == rep_env_back[pick]);
        CHECK((int)pt_plan_variant(false, pick, pt_plan_back(64, 20), false).back_pct == 0);
        CHECK((int)pt_plan_variant(true, pick, pt_plan_back(64, 20), false).back_pct == 0);
    }

    // ---- the chained share
    CHECK(pt_plan_chain_back(false, 20, false) == 100 && pt_plan_chain_back(false, 45, false) == 100);
    CHECK(pt_plan_chain_back(false, 0, false) == 0 && pt_plan_chain_back(false, 30, true) == 30);
    CHECK(pt_plan_chain_back(true, 33, false) == 33 && pt_plan_chain_back(true, 0, false) == 0);
    CHECK(pt_plan_chain_back_v4(8, 20, false) == 100 && pt_plan_chain_back_v4(16, 20, false) == 100);
    CHECK(pt_plan_chain_back_v4(17, 20, false) == 0 && pt_plan_chain_back_v4(8, 30, true) == 30);
    CHECK(pt_plan_chain_back_v4(8, 0, true) == 0 && pt_plan_chain_back_v4(64, 30, true) == 0);

    // ---- the continue rule: of its 32 rows only (same geometry, built, not building, fixed, cache allows)
    for (int m = 0; m < 32; ++m) {
        const bool same = m & 1, built = m & 2, builds = m & 4, fixed = m & 8, cam = m & 16;
        CHECK(pt_plan_chain_continues(same, built, builds, fixed, cam) == (m == (1 | 2 | 8 | 16)));
    }
    // the camera-hit cache: 7 frames never touch it; 8 frames continue only on a settled cache
    const uint8_t states[3] = {kCamEmpty, kCamFilled, kCamSettled};
    const bool want8[3] = {false, false, true};
    CHECK(kCamEmpty == 0 && kCamFilled == 1 && kCamSettled == 2);
    CHECK(!pt_cam_launch_qualifies(false, 7, true) && pt_cam_launch_qualifies(false, 8, true));
    CHECK(!pt_cam_launch_qualifies(true, 8, true) && !pt_cam_launch_qualifies(false, 8, false));
    for (int i = 0; i < 3; ++i) {
        CHECK(pt_cam_chain_may_continue(pt_cam_launch_qualifies(false, 7, true), true, states[i]));
        CHECK(pt_cam_chain_may_continue(pt_cam_launch_qualifies(false, 7, true), false, states[i]));
        CHECK(pt_cam_chain_may_continue(pt_cam_launch_qualifies(false, 8, true), true, states[i]) == want8[i]);
        CHECK(!pt_cam_chain_may_continue(pt_cam_launch_qualifies(false, 8, true), false, states[i]));   // (not allocated yet)
        CHECK(pt_cam_chain_may_continue(pt_cam_launch_qualifies(true, 8, true), false, states[i]));     // (no cache, ever)
        CHECK(pt_cam_chain_may_continue(pt_cam_launch_qualifies(false, 8, false), false, states[i]));   // (v4, switched off)
    }

    if (fails) printf("%d check(s) failed\n", fails);
    else printf("launch plan: all checks hold\n");
    return fails ? 1 : 0;
}
