// pt_kernel_pick.h -- which kernel instance a job runs, once, as data and functions of
// plain inputs: pt_kernel.hip and pt_v4.hip build their instance tables from the key lists below and
// look the picked key up; pt_capi.cpp shares the camera test; the host check
// (tests/native/check_kernel_pick.cpp) enumerates the facts.  No HIP include: a host compiler reads it.
// A key holds a kernel's template arguments as values.  A new instance is one more key in a list here:
// the tables (pt_instance / v4_instance) instantiate exactly the listed keys.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

constexpr int kPickLayouts = 3, kPickTiled = 2;   // PT_LAYOUT_*: 0 interleaved, 1 planar8 (the row layouts), 2 tiled
constexpr int kPickChunk = 8;                     // frames per LDS chunk (kChunk of both renderers)
constexpr int kPickWaves = 4;                     // waves per block of every render kernel

template <typename K, size_t N>
struct PtKeyList {
    K k[N];
    static constexpr size_t size = N;
    constexpr int find(const K& key) const   // index, -1: no such instance
    {
        for (size_t i = 0; i < N; ++i)
            if (k[i] == key) return (int)i;
        return -1;
    }
};

// The persistent grid: the resident blocks, at most one tile per wave.
constexpr uint32_t pt_pick_grid(uint32_t resident_blocks, uint32_t tiles, uint32_t waves_per_block)
{
    const uint64_t need = ((uint64_t)tiles + waves_per_block - 1) / waves_per_block;
    return need < resident_blocks ? (uint32_t)need : resident_blocks;
}

// ---- the diffuse renderers (pt_kernel.hip) ----
// multi, ring: pt_render_kernel / pt_render_env_kernel (the per-tile pools); ct, wide, present: the
// continuous-tiles kernels (wide: 6 waves per SIMD, the ambient kernel only).
struct PtKey {
    int layout;
    bool env, count, multi, ring, ct, wide, present;
    constexpr bool operator==(const PtKey& o) const
    {
        return layout == o.layout && env == o.env && count == o.count && multi == o.multi && ring == o.ring && ct == o.ct &&
               wide == o.wide && present == o.present;
    }
};
struct PtFacts {
    int layout;
    bool env;
    int32_t nframes;
    bool count, ct_wide, pix_out;
};
// Launches of at least kRingMinFrames frames run the ambient kernel's continuous ring pool (one pool
// tail per tile instead of one per 8-frame chunk); fewer frames keep the chunked pool, whose own-lane
// frame and lighter iteration win while there are only a few chunks.  Ring vs chunked at 1080p
// (profiles/r03y_ab_*.jsonl): 16 spp 0.484 vs 0.462 ms, 32 spp 0.898 vs 0.890, 48 spp 1.307 vs
// 1.316; 4K 64 spp 6.33 vs 6.74 ms; 8K 256 spp 97.9 vs 106.4 ms.
#ifndef PT_RING_MIN
#define PT_RING_MIN 48
#endif
constexpr int kRingMinFrames = PT_RING_MIN;

// counted launches are device jobs (pt_capi.cpp pt_count_device: the row layouts only), so the tiled
// layout has no counting instances
constexpr bool pt_pick_valid(const PtFacts& f)
{
    return f.layout >= 0 && f.layout < kPickLayouts && !(f.layout == kPickTiled && f.count);
}
// The per-tile pools.  multi: the launch accumulates more frames than one LDS chunk holds.
constexpr PtKey pt_pick_pool_key(const PtFacts& f)
{
    const bool multi = f.nframes > kPickChunk;
    return {f.layout, f.env, f.count, multi, multi && !f.env && f.nframes >= kRingMinFrames, false, false, false};
}
// The continuous-tiles pool; its presenting instances (row layouts, uncounted) write job.pix_out themselves.
constexpr PtKey pt_pick_ct_key(const PtFacts& f)
{
    return {f.layout, f.env, f.count, false, false, true, !f.env && f.ct_wide, f.pix_out && !f.count && f.layout != kPickTiled};
}
// It takes every launch whose grid the caller's slots cover (ct_waves_cap waves; pt_capi.cpp use_ct_slots).
constexpr bool pt_pick_ct_takes(bool have_slots, uint64_t ct_waves_cap, uint32_t resident_blocks, uint32_t tiles)
{
    return have_slots && (uint64_t)pt_pick_grid(resident_blocks, tiles, kPickWaves) * kPickWaves <= ct_waves_cap;
}
// A presenting job whose launch did not present is followed by the stand-alone output pass.
constexpr bool pt_pick_tonemap_follows(bool pix_out, bool presented) { return pix_out && !presented; }

// Every instance: per layout, the ambient then the env kernels; the tiled layout has the uncounted,
// not presenting ones.
struct PtShape {
    bool count, multi, ring, ct, wide, present;
};
constexpr PtShape kPtAmbientShapes[12] = {
    {false, false, false, false, false, false}, {false, true, false, false, false, false}, {false, true, true, false, false, false},
    {true, false, false, false, false, false},  {true, true, false, false, false, false},  {true, true, true, false, false, false},
    {false, false, false, true, false, false},  {false, false, false, true, true, false},  {false, false, false, true, false, true},
    {false, false, false, true, true, true},    {true, false, false, true, false, false},  {true, false, false, true, true, false},
};
constexpr PtShape kPtEnvShapes[7] = {
    {false, false, false, false, false, false}, {false, true, false, false, false, false}, {true, false, false, false, false, false},
    {true, true, false, false, false, false},   {false, false, false, true, false, false}, {false, false, false, true, false, true},
    {true, false, false, true, false, false},
};
constexpr size_t kPtKeyCount = 46;
constexpr PtKeyList<PtKey, kPtKeyCount> pt_key_list()
{
    PtKeyList<PtKey, kPtKeyCount> l{};
    size_t n = 0;
    for (int layout = 0; layout < kPickLayouts; ++layout)
        for (int env = 0; env < 2; ++env)
            for (size_t s = 0; s < (env ? 7u : 12u); ++s) {
                const PtShape h = env ? kPtEnvShapes[s] : kPtAmbientShapes[s];
                if (layout == kPickTiled && (h.count || h.present)) continue;
                l.k[n++] = {layout, env != 0, h.count, h.multi, h.ring, h.ct, h.wide, h.present};
            }
    return l;
}
constexpr PtKeyList<PtKey, kPtKeyCount> kPtKeys = pt_key_list();
static_assert(kPtKeys.k[kPtKeyCount - 1].ct && kPtKeys.k[kPtKeyCount - 1].env, "46 instances: the last is the tiled env CT one");

// ---- the v4 renderer (pt_v4.hip) ----
// pt_v4_kernel (the per-tile pool) or, ct, pt_v4_ct_kernel <env, layout, count, def, fexp, dfl, present>
struct PtV4Key {
    int env, layout;
    bool count, def;
    int fexp;
    bool dfl, present, ct;
    constexpr bool operator==(const PtV4Key& o) const
    {
        return env == o.env && layout == o.layout && count == o.count && def == o.def && fexp == o.fexp && dfl == o.dfl &&
               present == o.present && ct == o.ct;
    }
};
// What pt_launch_v4 knows of a job.  default_geometry: the scene is InitializeScene's
// (pt_v4_is_default_geometry); pix_out, pix_rows, pix_fast_tone: the present request (pt_v4.h)
struct PtV4Facts {
    int env, layout;
    int32_t nframes;
    bool count, default_geometry, camera_is_default, fast_exp, random_jitter, rejection;
    bool pix_out, pix_rows, pix_fast_tone;
};
// The DEF instances carry the default camera as literals: InitializeScene seen by a camera bit-equal
// to (0, 0, 40), distance 1.0f.  Any other camera runs the generic instances.
inline bool pt_v4_camera_is_default(const float pos[3], float dist)
{
    const float cam_default[4] = {0.0f, 0.0f, 40.0f, 1.0f}, cam[4] = {pos[0], pos[1], pos[2], dist};
    return memcmp(cam, cam_default, sizeof(cam)) == 0;
}
// def: the job runs the literal-scene instances.  present: the launch may write pix_out.  The fused
// output stage runs in the presenting instances only, uncounted, with fast exp and the default fast
// ACES / gamma:
//  - the drop-in's calls (DemofoxRenderOptV4: the tiled layout, one frame -- the per-tile pool
//    kernel, full-image pixel rows), the default scene and sampling flags;
//  - device jobs (pt_v4_render_device_present: a row layout, job-row pixels, pix_rows) that the
//    continuous-tiles kernel takes (pt_pick_v4_ct_takes), the default scene with the default
//    sampling flags or a generic scene.
struct PtV4Norm {
    bool def, present;
};
constexpr PtV4Norm pt_pick_v4_normalise(const PtV4Facts& f)
{
    const bool def = f.default_geometry && f.camera_is_default;
    const bool tiled = f.layout == kPickTiled;
    const bool tone = f.fast_exp && f.pix_fast_tone && !f.count;
    const bool dflt = def && f.random_jitter && f.rejection;
    return {def, f.pix_out && tone && (f.pix_rows ? !tiled && f.nframes >= kPickChunk && (dflt || !def)
                                                  : tiled && f.nframes < kPickChunk && dflt)};
}
// The tiled layout is the drop-in's (pt_capi.cpp pt_render_opt_v4 and its work-queue entries): one
// frame per call (NUM_SAMPLES_PER_FRAME = 1), never counted (counted launches are device jobs, the
// row layouts only) -- so only the per-tile pool's uncounted instances exist for it.
constexpr bool pt_pick_v4_valid(const PtV4Facts& f)
{
    return f.env >= 0 && f.env < 3 && f.layout >= 0 && f.layout < kPickLayouts &&
           !(f.layout == kPickTiled && (f.count || f.nframes >= kPickChunk));
}
// The per-tile pool's instance.  fexp: 2 in the counted instances, else fast_exp; dfl: the default
// scene's instance with the default sampling flags compiled in.  It presents in the tiled layout only:
// a presenting row-layout job that continuous tiles does not take renders plain and the caller converts.
constexpr PtV4Key pt_pick_v4_tile_key(const PtV4Facts& f, PtV4Norm n)
{
    return {f.env, f.layout, f.count, n.def, f.count ? 2 : (f.fast_exp ? 1 : 0),
            !f.count && n.def && f.fast_exp && f.random_jitter && f.rejection, n.present && f.layout == kPickTiled, false};
}
// The continuous-tiles twin (any: there is one -- not in the tiled layout).  The presenting ones: the
// default scene's default-flags instance and the generic scene's, whatever its sampling flags.
struct PtV4CtKey {
    bool any;
    PtV4Key key;
};
constexpr PtV4CtKey pt_pick_v4_ct_key(const PtV4Facts& f, PtV4Norm n)
{
    PtV4Key k = pt_pick_v4_tile_key(f, n);
    k.present = n.present;
    k.ct = true;
    return {f.layout != kPickTiled, k};
}
// The continuous-tiles kernel takes the launch when the caller provides its slots for the whole grid
// (ct_waves_cap waves) and the launch holds >= 4 full chunks (8 frames x tile) per wave (force: any
// launch of a full chunk), else the per-tile pool kernel.  Measured (round 4, 5-wave CT vs per-tile):
// 1080p 32 spp 1.257 vs 1.320 ms (51 chunks per wave), 4K 8 spp 1.308 vs 1.328 (25), 1080p 8 spp
// 0.3602 vs 0.3589 (6), 1 spp 0.133 vs 0.115 (one item per pixel and chunk: the chunk events, claim
// and fold, dominate); round 5, the 6-wave CT kernel: 1080p 8 spp (5.3 chunks per wave) 0.3591 vs 0.3602.
constexpr bool pt_pick_v4_ct_takes(bool have_slots, uint64_t ct_waves_cap, uint32_t resident_blocks, uint32_t tiles,
                                   int32_t nframes, bool force)
{
    const uint64_t ct_waves = (uint64_t)pt_pick_grid(resident_blocks, tiles, kPickWaves) * kPickWaves;
    return have_slots && ct_waves <= ct_waves_cap && nframes >= kPickChunk &&
           (force || (uint64_t)nframes * (uint64_t)tiles >= 4ull * kPickChunk * ct_waves);
}

// Every instance: per env mode and layout -- a row layout has the per-tile shapes and their
// continuous-tiles twins, the tiled layout its own per-tile ones.
struct PtV4Shape {
    bool count, def;
    int fexp;
    bool dfl, present, ct;
};
constexpr PtV4Shape kPtV4RowShapes[16] = {
    {true, true, 2, false, false, false},  {false, true, 1, true, false, false},   {false, true, 1, false, false, false},
    {false, true, 0, false, false, false}, {true, false, 2, false, false, false},  {false, false, 1, false, false, false},
    {false, false, 0, false, false, false},
    {true, true, 2, false, false, true},   {false, true, 1, true, false, true},    {false, true, 1, false, false, true},
    {false, true, 0, false, false, true},  {true, false, 2, false, false, true},   {false, false, 1, false, false, true},
    {false, false, 0, false, false, true}, {false, true, 1, true, true, true},     {false, false, 1, false, true, true},
};
constexpr PtV4Shape kPtV4TiledShapes[6] = {
    {false, true, 1, true, true, false},   {false, true, 1, true, false, false},   {false, true, 1, false, false, false},
    {false, true, 0, false, false, false}, {false, false, 1, false, false, false}, {false, false, 0, false, false, false},
};
constexpr size_t kPtV4KeyCount = 3 * (2 * 16 + 6);
constexpr PtKeyList<PtV4Key, kPtV4KeyCount> pt_v4_key_list()
{
    PtKeyList<PtV4Key, kPtV4KeyCount> l{};
    size_t n = 0;
    for (int env = 0; env < 3; ++env)
        for (int layout = 0; layout < kPickLayouts; ++layout)
            for (size_t s = 0; s < (layout == kPickTiled ? 6u : 16u); ++s) {
                const PtV4Shape h = layout == kPickTiled ? kPtV4TiledShapes[s] : kPtV4RowShapes[s];
                l.k[n++] = {env, layout, h.count, h.def, h.fexp, h.dfl, h.present, h.ct};
            }
    return l;
}
constexpr PtKeyList<PtV4Key, kPtV4KeyCount> kPtV4Keys = pt_v4_key_list();

// ---- the batched v4 launches (pt_v4.hip pt_v4_views_kernel / _scenes_ / _envs_ / _batch_ <env, layout, fexp>) ----
// What travels per view: kViews a camera, kScenes also a scene, kEnvs also an env map, kBatch also a frame
// range.  Each kind runs the per-tile pool's generic form only: uncounted, a row layout, the sampling flags
// and the pixel output at run time.  An envs launch has no meaning without an env term, so its ENV is
// equirect or cubemap; the batch launch (the superset) has an instance for every env term, none included.
// A list of its own: kPtV4Keys stays what one-camera jobs reach.
enum class PtV4BatchKind { kViews, kScenes, kEnvs, kBatch };
constexpr int kPtV4BatchKinds = 4;
struct PtV4BatchedKey {
    PtV4BatchKind kind;
    int env, layout, fexp;
    constexpr bool operator==(const PtV4BatchedKey& o) const
    {
        return kind == o.kind && env == o.env && layout == o.layout && fexp == o.fexp;
    }
};
constexpr bool pt_pick_v4_batched_valid(PtV4BatchKind kind, int env, int layout)
{
    return env >= (kind == PtV4BatchKind::kEnvs ? 1 : 0) && env < 3 && layout >= 0 && layout < kPickTiled;
}
constexpr PtV4BatchedKey pt_pick_v4_batched_key(PtV4BatchKind kind, int env, int layout, bool fast_exp)
{
    return {kind, env, layout, fast_exp ? 1 : 0};
}
constexpr size_t kPtV4BatchedKeyCount = 12 + 12 + 8 + 12;
constexpr PtKeyList<PtV4BatchedKey, kPtV4BatchedKeyCount> pt_v4_batched_key_list()
{
    PtKeyList<PtV4BatchedKey, kPtV4BatchedKeyCount> l{};
    size_t n = 0;
    for (int kind = 0; kind < kPtV4BatchKinds; ++kind)
        for (int env = 0; env < 3; ++env)
            for (int layout = 0; layout < kPickTiled; ++layout)
                for (int fexp = 1; fexp >= 0; --fexp)
                    if (pt_pick_v4_batched_valid((PtV4BatchKind)kind, env, layout)) l.k[n++] = {(PtV4BatchKind)kind, env, layout, fexp};
    return l;
}
constexpr PtKeyList<PtV4BatchedKey, kPtV4BatchedKeyCount> kPtV4BatchedKeys = pt_v4_batched_key_list();
static_assert(kPtV4BatchedKeys.k[kPtV4BatchedKeyCount - 1] == PtV4BatchedKey{PtV4BatchKind::kBatch, 2, 1, 0},
              "44 instances: the last is the batch kind's cubemap, planar8, exact-exp one");

// ---- the batch launch with per-view statistics (pt_v4.hip pt_v4_batch_stats_kernel <env, layout, fexp>) ----
// The batch kind's twelve instances once more, each also reducing its tiles' 8-bit differences into the view's
// record (pt_v4.h PtV4Stats).  A list of its own: kPtV4BatchedKeys and PtV4BatchKind stay what the four plain
// calls reach, and their instances the code they were.
constexpr size_t kPtV4BatchStatsKeyCount = 12;
constexpr PtKeyList<PtV4BatchedKey, kPtV4BatchStatsKeyCount> pt_v4_batch_stats_key_list()
{
    PtKeyList<PtV4BatchedKey, kPtV4BatchStatsKeyCount> l{};
    size_t n = 0;
    for (int env = 0; env < 3; ++env)
        for (int layout = 0; layout < kPickTiled; ++layout)
            for (int fexp = 1; fexp >= 0; --fexp) l.k[n++] = {PtV4BatchKind::kBatch, env, layout, fexp};
    return l;
}
constexpr PtKeyList<PtV4BatchedKey, kPtV4BatchStatsKeyCount> kPtV4BatchStatsKeys = pt_v4_batch_stats_key_list();
static_assert(kPtV4BatchStatsKeys.k[0] == PtV4BatchedKey{PtV4BatchKind::kBatch, 0, 0, 1} &&
                  kPtV4BatchStatsKeys.k[kPtV4BatchStatsKeyCount - 1] == PtV4BatchedKey{PtV4BatchKind::kBatch, 2, 1, 0},
              "12 instances, in the batch kind's order");
