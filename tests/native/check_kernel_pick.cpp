// tests/native/check_kernel_pick.cpp -- host check of the instance pick (csrc/pt_kernel_pick.h, applied
// by pt_kernel.hip and pt_v4.hip): every expectation below is written out, none is computed by the header.
// usage: check_kernel_pick     exit 0 iff every check holds
#include <stdint.h>
#include <stdio.h>

#include "pt_kernel_pick.h"

static int fails = 0;
#define CHECK(c) \
    do { \
        if (!(c)) { \
            printf("FAILED line %d: %s\n", __LINE__, #c); \
            ++fails; \
        } \
    } while (0)

// layouts: 0 interleaved, 1 planar8, 2 tiled
static PtFacts diffuse(int layout, bool env, int32_t nframes, bool count = false, bool ct_wide = false, bool pix_out = false)
{
    return PtFacts{layout, env, nframes, count, ct_wide, pix_out};
}
static bool pool_is(bool env, int32_t nframes, bool multi, bool ring)
{
    const PtKey k = pt_pick_pool_key(diffuse(0, env, nframes));
    return k.multi == multi && k.ring == ring && !k.ct && !k.wide && !k.present && k.env == env && k.layout == 0 && !k.count;
}

// a device job that presents: interleaved rows, 8 frames, the default scene, camera and sampling flags,
// fast exp and the default tonemap pair
static PtV4Facts v4_rows()
{
    return PtV4Facts{0, 0, 8, false, true, true, true, true, true, true, true, true};
}
// the drop-in's presenting call: the tiled layout, one frame, full-image pixel rows
static PtV4Facts v4_dropin()
{
    PtV4Facts f = v4_rows();
    f.layout = 2;
    f.nframes = 1;
    f.pix_rows = false;
    return f;
}
static bool v4_key_is(const PtV4Key& k, int env, int layout, bool count, bool def, int fexp, bool dfl, bool present, bool ct)
{
    return k.env == env && k.layout == layout && k.count == count && k.def == def && k.fexp == fexp && k.dfl == dfl &&
           k.present == present && k.ct == ct;
}

int main()
{
    CHECK(kRingMinFrames == 48 && kPickChunk == 8 && kPickWaves == 4 && kPickTiled == 2);
    CHECK(kPtKeyCount == 46 && kPtV4KeyCount == 114);

    // ---- the grid
    CHECK(pt_pick_grid(1536, 5, 4) == 2);
    CHECK(pt_pick_grid(1536, 32400, 4) == 1536);
    CHECK(pt_pick_grid(1536, 4, 4) == 1 && pt_pick_grid(1536, 6144, 4) == 1536 && pt_pick_grid(1536, 6140, 4) == 1535);

    // ---- diffuse pools by frame count: single chunk, multi, ring (the ambient kernel from 48 frames)
    CHECK(pool_is(false, 1, false, false) && pool_is(true, 1, false, false));
    CHECK(pool_is(false, 8, false, false) && pool_is(true, 8, false, false));
    CHECK(pool_is(false, 9, true, false) && pool_is(true, 9, true, false));
    CHECK(pool_is(false, 47, true, false) && pool_is(true, 47, true, false));
    CHECK(pool_is(false, 48, true, true) && pool_is(true, 48, true, false));
    CHECK(pool_is(false, 256, true, true) && pool_is(true, 256, true, false));
    // the tiled layout is not countable; an unknown layout
    CHECK(!pt_pick_valid(diffuse(2, false, 8, true)) && !pt_pick_valid(diffuse(2, true, 8, true)));
    CHECK(pt_pick_valid(diffuse(2, false, 8)) && pt_pick_valid(diffuse(0, false, 8, true)) && pt_pick_valid(diffuse(1, true, 8, true)));
    CHECK(!pt_pick_valid(diffuse(3, false, 8)) && !pt_pick_valid(diffuse(-1, false, 8)));
    // continuous tiles presents only uncounted, in a row layout
    CHECK(pt_pick_ct_key(diffuse(0, false, 8, false, false, true)).present);
    CHECK(pt_pick_ct_key(diffuse(1, true, 8, false, false, true)).present);
    CHECK(!pt_pick_ct_key(diffuse(0, false, 8, true, false, true)).present);    // present + count
    CHECK(!pt_pick_ct_key(diffuse(2, false, 8, false, false, true)).present);   // present + tiled
    CHECK(!pt_pick_ct_key(diffuse(0, false, 8, false, false, false)).present);
    CHECK(!pt_pick_pool_key(diffuse(0, false, 8, false, false, true)).present);   // the per-tile pools never present
    // wide follows ct_wide (the ambient kernel; the env kernel has one occupancy)
    CHECK(pt_pick_ct_key(diffuse(0, false, 8, false, true)).wide && !pt_pick_ct_key(diffuse(0, false, 8, false, false)).wide);
    CHECK(pt_pick_ct_key(diffuse(1, false, 64, true, true)).wide && !pt_pick_ct_key(diffuse(1, true, 8, false, true)).wide);
    {
        const PtKey k = pt_pick_ct_key(diffuse(1, false, 64, true, true, true));
        CHECK(k.layout == 1 && !k.env && k.count && !k.multi && !k.ring && k.ct && k.wide && !k.present);
    }
    // continuous tiles takes a launch whose grid the slots cover: 1536 resident blocks are 6144 waves
    CHECK(pt_pick_ct_takes(true, 6144, 1536, 32400));
    CHECK(!pt_pick_ct_takes(false, 6144, 1536, 32400));   // no slots
    CHECK(!pt_pick_ct_takes(true, 6143, 1536, 32400));    // the grid exceeds ct_waves
    CHECK(pt_pick_ct_takes(true, 8, 1536, 5) && !pt_pick_ct_takes(true, 7, 1536, 5));   // (5 tiles: 2 blocks, 8 waves)
    // the follow-up tonemap pass: pix_out set and the launch did not present
    CHECK(pt_pick_tonemap_follows(true, false));
    CHECK(!pt_pick_tonemap_follows(true, true) && !pt_pick_tonemap_follows(false, false) && !pt_pick_tonemap_follows(false, true));

    // ---- v4: the default camera, by bits
    {
        const float dflt[3] = {0.0f, 0.0f, 40.0f}, far_z[3] = {0.0f, 0.0f, 40.000004f}, neg0[3] = {-0.0f, 0.0f, 40.0f};
        CHECK(pt_v4_camera_is_default(dflt, 1.0f));
        CHECK(!pt_v4_camera_is_default(far_z, 1.0f));
        CHECK(!pt_v4_camera_is_default(neg0, 1.0f));
        CHECK(!pt_v4_camera_is_default(dflt, 1.0000001f));
    }
    // DEF needs the default geometry and the default camera
    {
        PtV4Facts f = v4_rows();
        CHECK(pt_pick_v4_normalise(f).def);
        f.camera_is_default = false;
        CHECK(!pt_pick_v4_normalise(f).def);
        f = v4_rows();
        f.default_geometry = false;
        CHECK(!pt_pick_v4_normalise(f).def);
    }
    // DFL needs both sampling flags (and fast exp); FEXP is 2 in the counted instances, else fast_exp
    {
        PtV4Facts f = v4_rows();
        f.pix_out = false;
        CHECK(v4_key_is(pt_pick_v4_tile_key(f, pt_pick_v4_normalise(f)), 0, 0, false, true, 1, true, false, false));
        f.random_jitter = false;
        CHECK(v4_key_is(pt_pick_v4_tile_key(f, pt_pick_v4_normalise(f)), 0, 0, false, true, 1, false, false, false));
        f.random_jitter = true;
        f.rejection = false;
        CHECK(v4_key_is(pt_pick_v4_tile_key(f, pt_pick_v4_normalise(f)), 0, 0, false, true, 1, false, false, false));
        f.rejection = true;
        f.fast_exp = false;
        CHECK(v4_key_is(pt_pick_v4_tile_key(f, pt_pick_v4_normalise(f)), 0, 0, false, true, 0, false, false, false));
        f.count = true;
        CHECK(v4_key_is(pt_pick_v4_tile_key(f, pt_pick_v4_normalise(f)), 0, 0, true, true, 2, false, false, false));
        f.fast_exp = true;
        CHECK(v4_key_is(pt_pick_v4_tile_key(f, pt_pick_v4_normalise(f)), 0, 0, true, true, 2, false, false, false));
        f.default_geometry = false;
        f.env = 2;
        f.layout = 1;
        CHECK(v4_key_is(pt_pick_v4_tile_key(f, pt_pick_v4_normalise(f)), 2, 1, true, false, 2, false, false, false));
        CHECK(v4_key_is(pt_pick_v4_ct_key(f, pt_pick_v4_normalise(f)).key, 2, 1, true, false, 2, false, false, true));
        f.count = false;
        CHECK(v4_key_is(pt_pick_v4_tile_key(f, pt_pick_v4_normalise(f)), 2, 1, false, false, 1, false, false, false));
    }
    // the present rule, a row-layout device job: each conjunct flipped alone removes presentation
    {
        PtV4Facts f = v4_rows();
        CHECK(pt_pick_v4_normalise(f).present);
        CHECK(v4_key_is(pt_pick_v4_ct_key(f, pt_pick_v4_normalise(f)).key, 0, 0, false, true, 1, true, true, true));
        // continuous tiles may not take it: the per-tile twin does not present
        CHECK(v4_key_is(pt_pick_v4_tile_key(f, pt_pick_v4_normalise(f)), 0, 0, false, true, 1, true, false, false));
        f = v4_rows(), f.pix_out = false;
        CHECK(!pt_pick_v4_normalise(f).present);
        f = v4_rows(), f.fast_exp = false;
        CHECK(!pt_pick_v4_normalise(f).present);
        f = v4_rows(), f.pix_fast_tone = false;
        CHECK(!pt_pick_v4_normalise(f).present);
        f = v4_rows(), f.count = true;
        CHECK(!pt_pick_v4_normalise(f).present);
        f = v4_rows(), f.layout = 2;   // job-row pixels are the row layouts'
        CHECK(!pt_pick_v4_normalise(f).present);
        f = v4_rows(), f.nframes = 7;
        CHECK(!pt_pick_v4_normalise(f).present);
        // the rule's dflt term: the default scene presents with the default sampling flags only
        f = v4_rows(), f.random_jitter = false;
        CHECK(!pt_pick_v4_normalise(f).present);
        f = v4_rows(), f.rejection = false;
        CHECK(!pt_pick_v4_normalise(f).present);
        // the generic presenting instance, whatever the sampling flags (a moved camera, another geometry)
        for (int m = 0; m < 8; ++m) {
            f = v4_rows();
            f.random_jitter = m & 1;
            f.rejection = m & 2;
            if (m & 4) f.camera_is_default = false;
            else f.default_geometry = false;
            CHECK(pt_pick_v4_normalise(f).present);
            CHECK(v4_key_is(pt_pick_v4_ct_key(f, pt_pick_v4_normalise(f)).key, 0, 0, false, false, 1, false, true, true));
        }
    }
    // the present rule, the drop-in's call
    {
        PtV4Facts f = v4_dropin();
        CHECK(pt_pick_v4_normalise(f).present && !pt_pick_v4_ct_key(f, pt_pick_v4_normalise(f)).any);
        CHECK(v4_key_is(pt_pick_v4_tile_key(f, pt_pick_v4_normalise(f)), 0, 2, false, true, 1, true, true, false));
        f = v4_dropin(), f.pix_out = false;
        CHECK(!pt_pick_v4_normalise(f).present);
        CHECK(v4_key_is(pt_pick_v4_tile_key(f, pt_pick_v4_normalise(f)), 0, 2, false, true, 1, true, false, false));
        f = v4_dropin(), f.fast_exp = false;
        CHECK(!pt_pick_v4_normalise(f).present);
        f = v4_dropin(), f.pix_fast_tone = false;
        CHECK(!pt_pick_v4_normalise(f).present);
        f = v4_dropin(), f.count = true;
        CHECK(!pt_pick_v4_normalise(f).present);
        f = v4_dropin(), f.layout = 0;   // full-image pixel rows are the tiled layout's
        CHECK(!pt_pick_v4_normalise(f).present);
        f = v4_dropin(), f.nframes = 8;
        CHECK(!pt_pick_v4_normalise(f).present);
        f = v4_dropin(), f.random_jitter = false;
        CHECK(!pt_pick_v4_normalise(f).present);
        f = v4_dropin(), f.rejection = false;
        CHECK(!pt_pick_v4_normalise(f).present);
        f = v4_dropin(), f.camera_is_default = false;   // (no generic presenting instance in the tiled layout)
        CHECK(!pt_pick_v4_normalise(f).present);
    }
    // the tiled layout: no continuous tiles, nothing counted, fewer than 8 frames
    {
        PtV4Facts f = v4_dropin();
        CHECK(pt_pick_v4_valid(f));
        f.nframes = 7;
        CHECK(pt_pick_v4_valid(f));
        f.nframes = 8;
        CHECK(!pt_pick_v4_valid(f));
        f = v4_dropin(), f.count = true;
        CHECK(!pt_pick_v4_valid(f));
        f = v4_rows(), f.count = true, f.nframes = 64;
        CHECK(pt_pick_v4_valid(f));
        f = v4_rows(), f.env = 3;
        CHECK(!pt_pick_v4_valid(f));
        f = v4_rows(), f.layout = 3;
        CHECK(!pt_pick_v4_valid(f));
    }
    // the continuous-tiles take rule at 1536 resident blocks: 6144 waves, nframes x tiles >= 196608
    CHECK(pt_pick_v4_ct_takes(true, 6144, 1536, 240 * 135, 8, false));
    CHECK(!pt_pick_v4_ct_takes(true, 6144, 1536, 160 * 90, 8, false));
    CHECK(!pt_pick_v4_ct_takes(true, 6144, 1536, 160 * 90, 13, false));   // 187200
    CHECK(pt_pick_v4_ct_takes(true, 6144, 1536, 160 * 90, 14, false));    // 201600
    CHECK(!pt_pick_v4_ct_takes(true, 6144, 1536, 240 * 135, 7, false) && !pt_pick_v4_ct_takes(true, 6144, 1536, 240 * 135, 7, true));
    CHECK(pt_pick_v4_ct_takes(true, 6144, 1536, 160 * 90, 8, true));
    CHECK(!pt_pick_v4_ct_takes(true, 6143, 1536, 240 * 135, 8, false) && !pt_pick_v4_ct_takes(true, 6143, 1536, 160 * 90, 8, true));
    CHECK(!pt_pick_v4_ct_takes(false, 6144, 1536, 240 * 135, 8, false) && !pt_pick_v4_ct_takes(false, 6144, 1536, 160 * 90, 8, true));

    // ---- the key lists: some instances that exist, some that do not
    CHECK(kPtKeys.find(PtKey{0, false, true, true, true, false, false, false}) >= 0);     // counted ring
    CHECK(kPtKeys.find(PtKey{2, false, false, false, false, true, true, false}) >= 0);    // tiled 6-wave CT
    CHECK(kPtKeys.find(PtKey{2, false, true, false, false, false, false, false}) < 0);    // tiled, counted
    CHECK(kPtKeys.find(PtKey{2, true, false, false, false, true, false, true}) < 0);      // tiled, presenting
    CHECK(kPtKeys.find(PtKey{0, true, false, true, true, false, false, false}) < 0);      // env ring
    CHECK(kPtKeys.find(PtKey{0, true, false, false, false, true, true, false}) < 0);      // env 6-wave CT
    CHECK(kPtV4Keys.find(PtV4Key{1, 2, false, true, 1, true, true, false}) >= 0);         // the drop-in's presenting one
    CHECK(kPtV4Keys.find(PtV4Key{1, 0, false, false, 1, false, true, true}) >= 0);        // generic presenting CT
    CHECK(kPtV4Keys.find(PtV4Key{1, 0, false, false, 1, false, true, false}) < 0);        // row layouts present in CT only
    CHECK(kPtV4Keys.find(PtV4Key{1, 2, false, true, 1, true, false, true}) < 0);          // tiled CT
    CHECK(kPtV4Keys.find(PtV4Key{1, 2, true, true, 2, false, false, false}) < 0);         // tiled, counted
    CHECK(kPtV4Keys.find(PtV4Key{0, 0, false, false, 1, true, false, false}) < 0);        // DFL without DEF
    // no key twice
    for (size_t i = 0; i < kPtKeyCount; ++i) CHECK(kPtKeys.find(kPtKeys.k[i]) == (int)i);
    for (size_t i = 0; i < kPtV4KeyCount; ++i) CHECK(kPtV4Keys.find(kPtV4Keys.k[i]) == (int)i);

    // ---- the batched v4 launches: kinds 0 views, 1 scenes, 2 envs, 3 batch; 12 + 12 + 8 + 12 instances
    CHECK(kPtV4BatchedKeyCount == 44 && kPtV4BatchedKeys.size == 44);
    CHECK((int)PtV4BatchKind::kViews == 0 && (int)PtV4BatchKind::kScenes == 1 && (int)PtV4BatchKind::kEnvs == 2 &&
          (int)PtV4BatchKind::kBatch == 3);
    for (size_t i = 0; i < kPtV4BatchedKeyCount; ++i) CHECK(kPtV4BatchedKeys.find(kPtV4BatchedKeys.k[i]) == (int)i);   // no key twice
    {
        int valid = 0, per_kind[4] = {0, 0, 0, 0};
        for (int kind = 0; kind < 4; ++kind)
            for (int env = -1; env <= 3; ++env)
                for (int layout = -1; layout <= 3; ++layout) {
                    const PtV4BatchKind k = (PtV4BatchKind)kind;
                    // written out: a row layout (0, 1), env in [0, 3), and an envs launch has an env term
                    const bool expect = (layout == 0 || layout == 1) && (env == 0 || env == 1 || env == 2) && !(kind == 2 && env == 0);
                    CHECK(pt_pick_v4_batched_valid(k, env, layout) == expect);
                    for (int fe = 0; fe < 2; ++fe) {
                        const PtV4BatchedKey key = pt_pick_v4_batched_key(k, env, layout, fe != 0);
                        CHECK(key.kind == k && key.env == env && key.layout == layout && key.fexp == fe);   // fast_exp -> fexp 1 / 0
                        int found = 0;
                        for (size_t i = 0; i < kPtV4BatchedKeyCount; ++i) found += kPtV4BatchedKeys.k[i] == key;
                        CHECK(found == (expect ? 1 : 0));   // a valid key at exactly one index, an invalid one nowhere
                        valid += expect;
                        per_kind[kind] += expect;
                    }
                }
        CHECK(valid == 44 && per_kind[0] == 12 && per_kind[1] == 12 && per_kind[2] == 8 && per_kind[3] == 12);
    }
    CHECK(!pt_pick_v4_batched_valid(PtV4BatchKind::kEnvs, 0, 0) && !pt_pick_v4_batched_valid(PtV4BatchKind::kEnvs, 0, 1));   // envs, env none
    CHECK(pt_pick_v4_batched_valid(PtV4BatchKind::kEnvs, 1, 0) && pt_pick_v4_batched_valid(PtV4BatchKind::kBatch, 0, 1));
    for (int kind = 0; kind < 4; ++kind) {
        CHECK(!pt_pick_v4_batched_valid((PtV4BatchKind)kind, 1, 2));   // the tiled layout
        CHECK(!pt_pick_v4_batched_valid((PtV4BatchKind)kind, 3, 0) && !pt_pick_v4_batched_valid((PtV4BatchKind)kind, -1, 0));
    }
    CHECK(pt_pick_v4_batched_key(PtV4BatchKind::kScenes, 2, 1, true).fexp == 1 && pt_pick_v4_batched_key(PtV4BatchKind::kScenes, 2, 1, false).fexp == 0);
    // ordered by kind, then env, layout, fast exp first -- as the four lists before them
    CHECK((kPtV4BatchedKeys.k[0] == PtV4BatchedKey{PtV4BatchKind::kViews, 0, 0, 1}) && (kPtV4BatchedKeys.k[1] == PtV4BatchedKey{PtV4BatchKind::kViews, 0, 0, 0}));
    CHECK((kPtV4BatchedKeys.k[12] == PtV4BatchedKey{PtV4BatchKind::kScenes, 0, 0, 1}) && (kPtV4BatchedKeys.k[24] == PtV4BatchedKey{PtV4BatchKind::kEnvs, 1, 0, 1}));
    CHECK((kPtV4BatchedKeys.k[32] == PtV4BatchedKey{PtV4BatchKind::kBatch, 0, 0, 1}) && (kPtV4BatchedKeys.k[43] == PtV4BatchedKey{PtV4BatchKind::kBatch, 2, 1, 0}));

    // ---- completeness: every key a valid job can be given exists; the listed keys no job reaches are printed
    static bool hit[kPtKeyCount], hit4[kPtV4KeyCount];
    int jobs = 0, unreached = 0;
    const int32_t frames[8] = {1, 7, 8, 9, 16, 47, 48, 64};
    for (int layout = 0; layout < 3; ++layout)
        for (int m = 0; m < 16; ++m)
            for (int fi = 0; fi < 8; ++fi) {
                const PtFacts f = diffuse(layout, m & 1, frames[fi], m & 2, m & 4, m & 8);
                if (!pt_pick_valid(f)) continue;
                ++jobs;
                const int ct = kPtKeys.find(pt_pick_ct_key(f)), pool = kPtKeys.find(pt_pick_pool_key(f));
                CHECK(ct >= 0 && pool >= 0);
                if (ct >= 0) hit[ct] = true;
                if (pool >= 0) hit[pool] = true;
            }
    for (int env = 0; env < 3; ++env)
        for (int layout = 0; layout < 3; ++layout)
            for (int m = 0; m < 512; ++m)
                for (int fi = 0; fi < 8; ++fi) {
                    const PtV4Facts f{env, layout, frames[fi], (m & 1) != 0, (m & 2) != 0, (m & 4) != 0, (m & 8) != 0,
                                      (m & 16) != 0, (m & 32) != 0, (m & 64) != 0, (m & 128) != 0, (m & 256) != 0};
                    if (!pt_pick_v4_valid(f)) continue;
                    ++jobs;
                    const PtV4Norm n = pt_pick_v4_normalise(f);
                    const PtV4CtKey ck = pt_pick_v4_ct_key(f, n);
                    const int tile = kPtV4Keys.find(pt_pick_v4_tile_key(f, n)), ct = ck.any ? kPtV4Keys.find(ck.key) : -1;
                    CHECK(tile >= 0 && (ct >= 0 || !ck.any));
                    CHECK(ck.any == (layout != 2));
                    if (tile >= 0) hit4[tile] = true;
                    if (ct >= 0) hit4[ct] = true;
                }
    for (size_t i = 0; i < kPtKeyCount; ++i)
        if (!hit[i]) {
            const PtKey& k = kPtKeys.k[i];
            printf("never picked: diffuse {layout %d env %d count %d multi %d ring %d ct %d wide %d present %d}\n", k.layout, k.env,
                   k.count, k.multi, k.ring, k.ct, k.wide, k.present);
            ++unreached;
        }
    for (size_t i = 0; i < kPtV4KeyCount; ++i)
        if (!hit4[i]) {
            const PtV4Key& k = kPtV4Keys.k[i];
            printf("never picked: v4 {env %d layout %d count %d def %d fexp %d dfl %d present %d ct %d}\n", k.env, k.layout, k.count,
                   k.def, k.fexp, k.dfl, k.present, k.ct);
            ++unreached;
        }
    printf("%d jobs enumerated, %d listed keys never picked\n", jobs, unreached);
    CHECK(unreached == 0);   // (today every instance is reachable)

    if (fails) printf("%d check(s) failed\n", fails);
    else printf("kernel pick: all checks hold\n");
    return fails ? 1 : 0;
}
