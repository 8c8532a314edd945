// tests/native/check_v4_batch.cpp -- host check of the batched v4 launch's rules (csrc/pt_v4_batch.h, applied by
// pt_capi.cpp): the block layout of every reachable shape against section sizes worked out here from sizeof, the
// fill into a block of exactly `need` bytes (the sanitized build of this program sees any overrun) against values
// written out here, and every rejection tests/test_abi_v4_{views,scenes,envs,batch,batch_stats}.py exercise, with
// their words, including calls that break two rules.
// usage: check_v4_batch     exit 0 iff every check holds
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pt_v4_batch.h"

static int fails = 0;
#define CHECK(c) \
    do { \
        if (!(c)) { \
            printf("FAILED line %d: %s\n", __LINE__, #c); \
            ++fails; \
        } \
    } while (0)

static int g_code = 0;
static char g_msg[512] = "";
static int record(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
    return g_code = code;
}

using Kind = PtV4BatchKind;
static pt_v4_env_set* const kFakeSet = reinterpret_cast<pt_v4_env_set*>(0x2000);   // never dereferenced
static const pt_v4_camera kCam = {{0.0f, 0.0f, 40.0f}, 90.0f};
static size_t r16(size_t n) { return (n + 15) / 16 * 16; }

// ---- layout -----------------------------------------------------------------------------------------------
// A reachable shape and what it must have; env: 0 none, 1 the staged map (no set, an env term), 2 a set.
struct ShapeCase {
    const char* name;
    Kind kind;
    int env;
    bool frames_given, scenes_given;
    bool recs, smap, emap, erec, frames, current;   // expected
};
static const ShapeCase kShapes[] = {
    {"views", Kind::kViews, 0, false, false, false, false, false, false, false, false},
    {"views, env term", Kind::kViews, 1, false, false, false, false, false, false, false, false},
    {"scenes", Kind::kScenes, 0, false, true, true, true, false, false, false, false},
    {"scenes, env term", Kind::kScenes, 1, false, true, true, true, false, false, false, false},
    {"envs + scenes", Kind::kEnvs, 2, false, true, true, true, true, false, false, false},
    {"envs, current scene", Kind::kEnvs, 2, false, false, true, true, true, false, false, true},
    {"batch set frames scenes", Kind::kBatch, 2, true, true, true, true, true, false, true, false},
    {"batch set frames current", Kind::kBatch, 2, true, false, true, true, true, false, true, true},
    {"batch set noframes scenes", Kind::kBatch, 2, false, true, true, true, true, false, true, false},
    {"batch set noframes current", Kind::kBatch, 2, false, false, true, true, true, false, true, true},
    {"batch staged frames scenes", Kind::kBatch, 1, true, true, true, true, true, true, true, false},
    {"batch staged frames current", Kind::kBatch, 1, true, false, true, true, true, true, true, true},
    {"batch staged noframes scenes", Kind::kBatch, 1, false, true, true, true, true, true, true, false},
    {"batch staged noframes current", Kind::kBatch, 1, false, false, true, true, true, true, true, true},
    {"batch noenv frames scenes", Kind::kBatch, 0, true, true, true, true, false, false, true, false},
    {"batch noenv frames current", Kind::kBatch, 0, true, false, true, true, false, false, true, true},
    {"batch noenv noframes scenes", Kind::kBatch, 0, false, true, true, true, false, false, true, false},
    {"batch noenv noframes current", Kind::kBatch, 0, false, false, true, true, false, false, true, true},
};

static pt_v4_batch shape_args(const ShapeCase& c, int32_t nviews, int32_t nscenes)
{
    static const pt_v4_frame_range some_frames[1] = {{1, 1}};
    static const pt_v4_scene_desc some_scenes[1] = {};
    pt_v4_batch a{};
    a.cams = &kCam;
    a.nviews = nviews;
    a.frames = c.frames_given ? some_frames : nullptr;   // (the shape looks at the pointers only)
    a.scenes = c.scenes_given ? some_scenes : nullptr;
    a.nscenes = c.scenes_given ? nscenes : 0;
    a.envs = c.env == 2 ? kFakeSet : nullptr;
    return a;
}

static void check_layouts()
{
    const int32_t sizes[5][2] = {{1, 1}, {3, 2}, {8, 8}, {1024, 1}, {1024, 1024}};
    for (const ShapeCase& c : kShapes)
        for (const auto& sz : sizes) {
            const int32_t nv = sz[0];
            const pt_v4_batch a = shape_args(c, nv, sz[1]);
            const PtV4BatchShape s = pt_v4_batch_shape(c.kind, a, c.env != 0, PT_V4_ENV_EQUIRECT);
            const bool shape_ok = s.scene_recs == c.recs && s.scene_map == c.smap && s.env_map == c.emap && s.staged_env == c.erec &&
                                  s.frames == c.frames && s.current_scene == c.current && s.env_set() == (c.env == 2);
            // the records: none for views, the one current scene, or the caller's
            const int32_t ns = c.kind == Kind::kViews ? 0 : c.scenes_given ? sz[1] : 1;
            const bool ns_ok = pt_v4_batch_nscenes(s, a) == ns;
            const size_t len[6] = {c.recs ? r16((size_t)ns * sizeof(PtV4SceneRec)) : 0, r16((size_t)nv * sizeof(PtV4View)),
                                   c.smap ? r16((size_t)nv * 4) : 0,                    c.emap ? r16((size_t)nv * 4) : 0,
                                   c.erec ? r16(sizeof(PtV4EnvRec)) : 0,                c.frames ? r16((size_t)nv * 8) : 0};
            const PtV4BatchLayout l = pt_v4_batch_layout(s, ns, nv);
            const size_t off[7] = {l.scenes, l.views, l.scene_map, l.env_map, l.env_rec, l.frames, l.need};
            bool ok = shape_ok && ns_ok && off[0] == 0;
            size_t end = 0;
            for (int i = 0; i < 6; ++i) {   // in the documented order, back to back: disjoint; absent: empty
                ok = ok && off[i] == end && off[i] % 16 == 0 && off[i + 1] - off[i] == len[i];
                end += len[i];
            }
            ok = ok && l.need == end;
            if (c.kind == Kind::kViews) ok = ok && l.views == 0 && l.need == r16((size_t)nv * sizeof(PtV4View));
            // the typed pointers are the offsets
            unsigned char* const base = reinterpret_cast<unsigned char*>(0x10000);
            ok = ok && (unsigned char*)pt_v4_batch_scenes(base, l) == base + l.scenes && (unsigned char*)pt_v4_batch_views(base, l) == base + l.views &&
                 (unsigned char*)pt_v4_batch_scene_map(base, l) == base + l.scene_map && (unsigned char*)pt_v4_batch_env_map(base, l) == base + l.env_map &&
                 (unsigned char*)pt_v4_batch_env_rec(base, l) == base + l.env_rec && (unsigned char*)pt_v4_batch_frames(base, l) == base + l.frames;
            if (!ok) {
                printf("FAILED layout: %s, %d views, %d scenes\n", c.name, nv, sz[1]);
                ++fails;
            }
        }
    // an env term is use_env AND an env mode: neither alone stages a table
    pt_v4_batch a{};
    a.cams = &kCam;
    a.nviews = 1;
    CHECK(!pt_v4_batch_shape(Kind::kBatch, a, 1, PT_V4_ENV_NONE).staged_env && !pt_v4_batch_shape(Kind::kBatch, a, 1, PT_V4_ENV_NONE).env_map);
    CHECK(!pt_v4_batch_shape(Kind::kBatch, a, 0, PT_V4_ENV_CUBEMAP).staged_env);
    CHECK(pt_v4_batch_shape(Kind::kBatch, a, 1, PT_V4_ENV_CUBEMAP).staged_env);
    CHECK(sizeof(PtV4EnvRec) == 16 && sizeof(PtV4FrameRange) == 8 && sizeof(PtV4View) == 16 + sizeof(PtV4SkyWin));
}

// ---- fill -------------------------------------------------------------------------------------------------
static PtV4SceneDesc g_default;
// scene i of a test: the default scene with i % 3 spheres fewer (so that the records differ)
static PtV4SceneDesc scene_no(int i)
{
    PtV4SceneDesc d = g_default;
    d.nspheres -= i % 3;
    return d;
}
static pt_v4_camera cam_no(int v) { return pt_v4_camera{{(float)v, -2.0f, 40.0f - (float)v}, 60.0f + (float)v}; }

enum MapMode { kGiven, kOmitted, kCurrent };
static void check_fill(Kind kind, int32_t nv, int32_t ns, MapMode smode, int env, MapMode emode, bool frames_given, bool sky_off)
{
    const bool views = kind == Kind::kViews;
    std::vector<pt_v4_camera> cams;
    std::vector<float> dist;
    std::vector<PtV4SceneDesc> descs;
    std::vector<int32_t> smap, emap;
    std::vector<pt_v4_frame_range> frames;
    for (int v = 0; v < nv; ++v) {
        cams.push_back(cam_no(v));
        dist.push_back(1.0f + 0.25f * (float)v);
        smap.push_back(ns ? (nv - 1 - v) % ns : 0);
        emap.push_back((v * 5 + 1) % nv);
        frames.push_back(pt_v4_frame_range{(uint32_t)(v + 1), 2 * v});
    }
    for (int i = 0; i < ns; ++i) descs.push_back(scene_no(i));
    PtV4SceneDesc current = scene_no(1);
    pt_v4_batch a{};
    a.cams = cams.data();
    a.nviews = nv;
    a.frames = frames_given ? frames.data() : nullptr;
    if (!views && smode != kCurrent) {
        a.scenes = reinterpret_cast<const pt_v4_scene_desc*>(descs.data());
        a.nscenes = ns;
        a.scene_of_view = smode == kGiven ? smap.data() : nullptr;
    }
    a.envs = env == 2 ? kFakeSet : nullptr;
    a.env_of_view = env == 2 && emode == kGiven ? emap.data() : nullptr;
    pt_device_job dj{reinterpret_cast<float*>(0x1000), 24, 16, 0, 1, 16, PT_LAYOUT_INTERLEAVED, 5, 8, 8, env != 0};
    const PtV4BatchState st{PT_V4_ENV_EQUIRECT, env == 2, env == 2 ? nv : 0, &current, sky_off};
    const PtV4BatchShape s = pt_v4_batch_shape(kind, a, dj.use_env, st.env_mode);
    const int32_t nrec = pt_v4_batch_nscenes(s, a);
    const PtV4BatchLayout l = pt_v4_batch_layout(s, nrec, nv);
    unsigned char* const blk = (unsigned char*)malloc(l.need);   // exactly: not rounded up
    memset(blk, 0xAB, l.need);
    const PtV4EnvRec staged{reinterpret_cast<const float*>(0x5000), 7, 9};
    CHECK(pt_v4_batch_fill(blk, l, s, dj, a, st, dist.data(), staged, record) == PT_OK);

    bool ok = nrec == (views ? 0 : smode == kCurrent ? 1 : ns);
    const unsigned char* p = blk;   // the sections, walked by the sizes worked out here
    for (int i = 0; i < nrec; ++i) {
        PtV4SceneRec want;
        const PtV4SceneDesc d = smode == kCurrent ? current : descs[(size_t)i];
        ok = ok && pt_v4_build_scene(&d, &want.sc) == 0;
        memset(want.mx, 0, sizeof(want.mx));
        ok = ok && !memcmp(p + (size_t)i * sizeof(PtV4SceneRec), &want, sizeof(want));
    }
    p += views ? 0 : r16((size_t)nrec * sizeof(PtV4SceneRec));
    for (int v = 0; v < nv; ++v) {
        PtV4View want;
        memcpy(want.cam_pos, cams[(size_t)v].position, sizeof(want.cam_pos));
        want.cam_dist = 1.0f + 0.25f * (float)v;
        const int sc = smode == kGiven ? (nv - 1 - v) % ns : smode == kCurrent ? 0 : v;
        const PtV4SceneDesc d = views || smode == kCurrent ? current : descs[(size_t)sc];
        pt_v4_skywin_build(d.nquads, d.quad, d.nspheres, d.sphere, cams[(size_t)v].position, &want.sky);
        PtV4View got;
        memcpy(&got, p + (size_t)v * sizeof(PtV4View), sizeof(got));
        if (sky_off) ok = ok && got.sky.nrects == -1 && !memcmp(got.cam_pos, want.cam_pos, 12) && got.cam_dist == want.cam_dist;
        else ok = ok && !memcmp(&got, &want, sizeof(want)) && got.sky.nrects >= 0;   // (these cameras see a window)
    }
    p += r16((size_t)nv * sizeof(PtV4View));
    if (!views) {
        for (int v = 0; v < nv; ++v) {
            int32_t got;
            memcpy(&got, p + 4 * (size_t)v, 4);
            ok = ok && got == (smode == kGiven ? (nv - 1 - v) % ns : smode == kCurrent ? 0 : v);
        }
        p += r16((size_t)nv * 4);
    }
    if (env == 2 || (env == 1 && kind == Kind::kBatch)) {
        for (int v = 0; v < nv; ++v) {
            int32_t got;
            memcpy(&got, p + 4 * (size_t)v, 4);
            ok = ok && got == (env == 1 ? 0 : emode == kGiven ? (v * 5 + 1) % nv : v);
        }
        p += r16((size_t)nv * 4);
    }
    if (env == 1 && kind == Kind::kBatch) {
        ok = ok && !memcmp(p, &staged, sizeof(staged));
        p += 16;
    }
    if (kind == Kind::kBatch) {
        for (int v = 0; v < nv; ++v) {
            PtV4FrameRange got;
            memcpy(&got, p + 8 * (size_t)v, 8);
            ok = ok && got.frame_first == (frames_given ? (uint32_t)(v + 1) : 5u) && got.nframes == (frames_given ? 2 * v : 8);
        }
        p += r16((size_t)nv * 8);
    }
    ok = ok && (size_t)(p - blk) == l.need;
    if (!ok) {
        printf("FAILED fill: kind %d, %d views, %d scenes, smode %d, env %d, emode %d, frames %d, sky_off %d\n", (int)kind, nv, ns, smode,
               env, emode, frames_given, sky_off);
        ++fails;
    }
    free(blk);
}

static void check_fills()
{
    const int32_t sizes[3][2] = {{1, 1}, {3, 2}, {8, 8}};
    for (const auto& sz : sizes) {
        const int32_t nv = sz[0], ns = sz[1];
        for (int sky_off = 0; sky_off < 2; ++sky_off) {
            check_fill(Kind::kViews, nv, 0, kOmitted, 0, kOmitted, false, sky_off);
            check_fill(Kind::kViews, nv, 0, kOmitted, 1, kOmitted, false, sky_off);
        }
        for (MapMode sm : {kGiven, kOmitted, kCurrent}) {
            if (sm == kOmitted && ns != nv) continue;   // (view v -> scene v needs a scene per view)
            if (sm != kCurrent) check_fill(Kind::kScenes, nv, ns, sm, 0, kOmitted, false, false);
            for (MapMode em : {kGiven, kOmitted}) check_fill(Kind::kEnvs, nv, ns, sm, 2, em, false, false);
            for (int fg = 0; fg < 2; ++fg) {
                check_fill(Kind::kBatch, nv, ns, sm, 0, kOmitted, fg, false);
                check_fill(Kind::kBatch, nv, ns, sm, 1, kOmitted, fg, fg);
                for (MapMode em : {kGiven, kOmitted}) check_fill(Kind::kBatch, nv, ns, sm, 2, em, fg, false);
            }
        }
    }
}

// ---- checks -----------------------------------------------------------------------------------------------
// One call's arguments; a row of the table changes what it needs.
struct Call {
    pt_device_job job{reinterpret_cast<float*>(0x1000), 256, 144, 0, 1, 144, PT_LAYOUT_INTERLEAVED, 1, 8, 8, 0};
    bool null_job = false;
    std::vector<pt_v4_camera> cams = std::vector<pt_v4_camera>(3, kCam);
    std::vector<pt_v4_scene_desc> scenes;
    std::vector<int32_t> smap, emap;
    std::vector<pt_v4_frame_range> frames;
    pt_v4_batch a{};
    PtV4BatchState st{PT_V4_ENV_EQUIRECT, false, 0, &g_default, false};
    int32_t nviews = -99, nscenes = -99;   // -99: the arrays' lengths
    bool null_cams = false, null_scenes = false;
    void view_count(size_t n) { cams.assign(n, kCam); }
    void huge() { job.width = 16384, job.height = job.nrows = 8192; }
    void live_set(int32_t count) { a.envs = kFakeSet, st.env_live = true, st.env_count = count, job.use_env = 1; }
};
static const pt_v4_camera kBadCam = {{0.0f, 0.0f, 40.0f}, 180.0f};
static uint32_t* const kPix = reinterpret_cast<uint32_t*>(0x3000);
constexpr uint32_t kMax = 1u << 24;

struct Row {
    Kind kind;
    void (*change)(Call&);
    int code;               // expected
    const char* words[2];   // "=text": the whole message; else a part of it; nullptr: not looked at
    bool nothing;           // PT_OK rows: nothing to render
};
static const Row kRows[] = {
    // -- what every kind rejects, as the views call words it (test_abi_v4_views.py)
    {Kind::kViews, [](Call& c) { c.null_job = true; }, PT_EINVAL, {"device job"}, false},
    {Kind::kBatch, [](Call& c) { c.null_job = true; }, PT_EINVAL, {"device job"}, false},
    {Kind::kViews, [](Call& c) { c.job.buf = nullptr, c.null_cams = true, c.nviews = 0; }, PT_EINVAL, {"=null device job/buffer"}, false},
    {Kind::kViews, [](Call& c) { c.null_cams = true, c.nviews = 0; }, PT_EINVAL, {"=null camera array"}, false},
    {Kind::kViews, [](Call& c) { c.null_cams = true, c.nviews = 2; }, PT_EINVAL, {"camera"}, false},
    {Kind::kViews, [](Call& c) { c.nviews = 0, c.a.pixels = kPix, c.a.format = 7; }, PT_EINVAL, {"=nviews 0 outside [1, 1024]"}, false},
    {Kind::kViews, [](Call& c) { c.nviews = -1; }, PT_EINVAL, {"nviews"}, false},
    {Kind::kViews, [](Call& c) { c.nviews = 1025; }, PT_EINVAL, {"nviews"}, false},
    {Kind::kViews, [](Call& c) { c.huge(), c.view_count(1024), c.a.pixels = kPix, c.a.format = 7; }, PT_EINVAL, {"=unknown pixel format 7"}, false},
    {Kind::kViews, [](Call& c) { c.huge(), c.cams.assign(1024, kBadCam); }, PT_EINVAL,
     {"=1024 views x 2097152 tiles exceed the tile queue's 1073741823 entries"}, false},
    {Kind::kViews, [](Call& c) { c.job.nframes = 0, c.cams = {kCam, kBadCam}; }, PT_EINVAL, {"=view 1: fov_degrees 180 outside (0, 180)"}, false},
    {Kind::kViews, [](Call& c) { c.job.frame_first = 0; }, PT_EINVAL, {"=frame range [0, +8) invalid"}, false},
    {Kind::kViews, [](Call& c) { c.job.layout = PT_LAYOUT_TILED_PLANAR8; }, PT_EINVAL, {nullptr}, false},
    {Kind::kViews, [](Call& c) { c.job.width = c.job.height = c.job.nrows = 8192, c.job.nframes = 0, c.view_count(1024); }, PT_EINVAL, {"tile"}, false},
    {Kind::kViews, [](Call& c) { c.job.width = 8192, c.job.height = c.job.nrows = 8184, c.job.nframes = 0, c.view_count(1024); }, PT_OK, {nullptr}, true},
    {Kind::kViews, [](Call& c) { c.a.pixels = kPix, c.a.format = 7; }, PT_EINVAL, {"format"}, false},
    {Kind::kViews, [](Call& c) { c.job.nframes = 0, c.a.format = 7; }, PT_OK, {nullptr}, true},   // no pixels: the format is not looked at
    {Kind::kViews, [](Call& c) { c.cams = {kCam, cam_no(1), kBadCam, kCam}; }, PT_EINVAL, {"view 2", "fov"}, false},
    {Kind::kViews, [](Call& c) { c.cams = {kCam, pt_v4_camera{{0.0f, NAN, 1.0f}, 90.0f}}; }, PT_EINVAL, {"view 1"}, false},
    {Kind::kViews, [](Call& c) { c.job.nframes = 0, c.job.use_env = 1; }, PT_OK, {nullptr}, true},
    {Kind::kViews, [](Call& c) { c.job.nrows = 0, c.job.use_env = 1; }, PT_OK, {nullptr}, true},
    {Kind::kViews, [](Call&) {}, PT_OK, {nullptr}, false},
    // -- the scenes call (test_abi_v4_scenes.py)
    {Kind::kScenes, [](Call& c) { c.job.buf = nullptr; }, PT_EINVAL, {nullptr}, false},
    {Kind::kScenes, [](Call& c) { c.null_cams = true, c.nviews = 1; }, PT_EINVAL, {"camera"}, false},
    {Kind::kScenes, [](Call& c) { c.nviews = 0; }, PT_EINVAL, {"nviews"}, false},
    {Kind::kScenes, [](Call& c) { c.a.pixels = kPix, c.a.format = 7; }, PT_EINVAL, {"format"}, false},
    {Kind::kScenes, [](Call& c) { c.huge(), c.view_count(1024), c.scenes.resize(1024); }, PT_EINVAL, {"tile"}, false},
    {Kind::kScenes, [](Call& c) { c.cams[2] = kBadCam; }, PT_EINVAL, {"view 2", "fov"}, false},
    {Kind::kScenes, [](Call& c) { c.null_scenes = true, c.nscenes = 1, c.view_count(1); }, PT_EINVAL, {"scene"}, false},
    {Kind::kScenes, [](Call& c) { c.view_count(1), c.smap = {0}, c.nscenes = 0; }, PT_EINVAL, {"nscenes"}, false},
    {Kind::kScenes, [](Call& c) { c.view_count(1), c.smap = {0}, c.nscenes = -1; }, PT_EINVAL, {"nscenes"}, false},
    {Kind::kScenes, [](Call& c) { c.view_count(1), c.smap = {0}, c.nscenes = 1025; }, PT_EINVAL, {"nscenes"}, false},
    {Kind::kScenes, [](Call& c) { c.scenes.resize(2); }, PT_EINVAL, {"nscenes 2", "nviews 3"}, false},
    {Kind::kScenes, [](Call& c) { c.job.nframes = 0; }, PT_OK, {nullptr}, true},
    {Kind::kScenes, [](Call& c) { c.scenes.resize(2), c.view_count(5), c.smap = {1, 0, 1, 2, 0}; }, PT_EINVAL, {"view 3"}, false},
    {Kind::kScenes, [](Call& c) { c.scenes.resize(2), c.view_count(5), c.smap = {-1, 0, 1, 1, 0}; }, PT_EINVAL, {"view 0"}, false},
    {Kind::kScenes, [](Call& c) { c.scenes.resize(2), c.view_count(5), c.smap = {1, 0, 1, 1, 1 << 30}; }, PT_EINVAL, {"view 4"}, false},
    {Kind::kScenes, [](Call& c) { c.scenes.resize(4), c.view_count(4), c.scenes[2].nquads = -1; }, PT_EINVAL, {"scene 2"}, false},
    {Kind::kScenes, [](Call& c) { c.scenes.resize(4), c.view_count(4), c.scenes[2].nmaterials = -1; }, PT_EINVAL, {"scene 2"}, false},
    {Kind::kScenes, [](Call& c) { c.scenes.resize(4), c.view_count(4), c.scenes[2].nquads = 7, c.scenes[2].nspheres = 6; }, PT_EINVAL, {"scene 2"}, false},
    {Kind::kScenes, [](Call& c) { c.scenes.resize(4), c.view_count(4), c.scenes[2].nspheres = 13; }, PT_EINVAL, {"scene 2"}, false},
    {Kind::kScenes, [](Call& c) { c.scenes.resize(4), c.view_count(4), c.scenes[2].nmaterials = 13; }, PT_EINVAL, {"scene 2"}, false},
    {Kind::kScenes, [](Call& c) { c.scenes.resize(4), c.view_count(4), c.scenes[2].nquads = c.scenes[2].nspheres = INT32_MAX; }, PT_EINVAL, {"scene 2"}, false},
    // (every description is checked, mapped to or not)
    {Kind::kScenes, [](Call& c) { c.scenes.resize(4), c.view_count(1), c.smap = {0}, c.scenes[2].nquads = 13; }, PT_EINVAL, {"scene 2"}, false},
    {Kind::kScenes, [](Call& c) { c.view_count(1), c.scenes.resize(1), c.cams[0].position[2] = 4000.0f; }, PT_EINVAL, {nullptr}, false},
    {Kind::kScenes, [](Call& c) { c.job.nrows = 0, c.view_count(5), c.smap = {2, 2, 0, 1, 1}; }, PT_OK, {nullptr}, true},
    // two at once: the mapping before the descriptions, the camera before both
    {Kind::kScenes, [](Call& c) { c.scenes[1].nquads = 13, c.smap = {0, 3, 0}; }, PT_EINVAL, {"scene_of_view 3"}, false},
    {Kind::kScenes, [](Call& c) { c.scenes[1].nquads = 13, c.cams[0] = kBadCam; }, PT_EINVAL, {"view 0", "fov"}, false},
    // -- the envs call (test_abi_v4_envs.py: use_env 1)
    {Kind::kEnvs, [](Call& c) { c.job.use_env = 1, c.scenes.clear(), c.view_count(1); }, PT_EINVAL, {"env set"}, false},
    {Kind::kEnvs, [](Call& c) { c.job.use_env = 1, c.scenes.clear(), c.view_count(1), c.job.nframes = 0; }, PT_EINVAL, {"env set"}, false},
    {Kind::kEnvs, [](Call& c) { c.job.use_env = 1, c.scenes.clear(), c.job.buf = nullptr; }, PT_EINVAL, {nullptr}, false},
    {Kind::kEnvs, [](Call& c) { c.job.use_env = 1, c.scenes.clear(), c.nviews = 0; }, PT_EINVAL, {"nviews"}, false},
    {Kind::kEnvs, [](Call& c) { c.job.use_env = 1, c.scenes.clear(), c.nscenes = 1; }, PT_EINVAL, {"nscenes"}, false},
    {Kind::kEnvs, [](Call& c) { c.job.use_env = 1, c.scenes.clear(), c.smap = {0, 0, 0}; }, PT_EINVAL, {"scene_of_view"}, false},
    {Kind::kEnvs, [](Call& c) { c.live_set(3), c.a.envs = kFakeSet, c.st.env_live = false; }, PT_EINVAL, {"not a live env set"}, false},
    {Kind::kEnvs, [](Call& c) { c.live_set(2); }, PT_EINVAL, {"the set has 2 textures for 3 views"}, false},
    {Kind::kEnvs, [](Call& c) { c.live_set(2), c.emap = {0, 2, 1}; }, PT_EINVAL, {"view 1", "env_of_view 2"}, false},
    // an envs call without an env term: rejected after the mapping checks, in its own words
    {Kind::kEnvs, [](Call& c) { c.live_set(3), c.job.use_env = 0; }, PT_EINVAL, {"an envs launch needs", "use_env 0"}, false},
    {Kind::kEnvs, [](Call& c) { c.live_set(3), c.st.env_mode = PT_V4_ENV_NONE; }, PT_EINVAL, {"an envs launch needs", "env mode 0"}, false},
    {Kind::kEnvs, [](Call& c) { c.live_set(3), c.job.use_env = 0, c.emap = {0, 3, 1}; }, PT_EINVAL, {"env_of_view 3"}, false},
    {Kind::kEnvs, [](Call& c) { c.live_set(3), c.emap = {2, 2, 0}; }, PT_OK, {nullptr}, false},
    {Kind::kEnvs, [](Call& c) { c.live_set(3), c.scenes.clear(), c.job.nframes = 0; }, PT_OK, {nullptr}, true},
    // -- the batch call (test_abi_v4_batch.py, test_abi_v4_batch_stats.py: the current scene unless said)
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.job.buf = nullptr; }, PT_EINVAL, {nullptr}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.nviews = 0; }, PT_EINVAL, {"nviews"}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.nviews = 0, c.null_cams = true; }, PT_EINVAL, {"camera"}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.null_cams = true; }, PT_EINVAL, {"camera"}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.a.pixels = kPix, c.a.format = 77; }, PT_EINVAL, {"format"}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.job.frame_first = 0; }, PT_EINVAL, {"frame range"}, false},   // frames NULL: the job's own
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.job.use_env = 1, c.a.envs = kFakeSet; }, PT_EINVAL, {"env set"}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.frames = {{0, 1}, {5, 0}, {3, 9}}; }, PT_EINVAL, {"view 0", "[0, +1)"}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.frames = {{1, 8}, {5, 0}, {1, -1}}; }, PT_EINVAL, {"view 2", "+-1)"}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.frames = {{kMax, 1}, {5, 0}, {3, 9}}; }, PT_EINVAL, {"view 0", "[16777216, +1)"}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.frames = {{1, 8}, {5, 0}, {kMax - 7, 8}}; }, PT_EINVAL, {"view 2", "+8)"}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.frames = {{0xFFFFFFFFu, 2}, {5, 0}, {3, 9}}; }, PT_EINVAL, {"view 0", "+2)"}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.frames = {{1, 8}, {0, 1}, {0, 1}}; }, PT_EINVAL, {"view 1"}, false},   // the first bad view
    // with ranges the job's own range is not read
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.job.frame_first = 0, c.job.nframes = -3, c.frames = {{1, 0}, {1, 0}, {1, 0}}; }, PT_OK, {nullptr}, true},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.frames = {{kMax, 0}, {kMax - 1, 0}, {1, 0}}; }, PT_OK, {nullptr}, true},
    // a set without an env term: before the set is looked at, in the batch call's words
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.a.envs = kFakeSet; }, PT_EINVAL, {"an env set needs", "use_env 0"}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.a.envs = kFakeSet, c.emap = {0, 0, 0}, c.frames = {{1, 8}, {1, 8}, {1, 8}}; }, PT_EINVAL, {"env term"}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.a.envs = kFakeSet, c.job.use_env = 1, c.st.env_mode = PT_V4_ENV_NONE; }, PT_EINVAL,
     {"an env set needs", "env mode 0"}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.frames = {{1, 0}, {1, 0}, {1, 0}}; }, PT_OK, {nullptr}, true},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.nscenes = 1; }, PT_EINVAL, {"nscenes"}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.smap = {0, 0, 0}; }, PT_EINVAL, {"scene_of_view"}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.emap = {0, 0, 0}; }, PT_EINVAL, {"env_of_view"}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.job.use_env = 1, c.emap = {0, 0, 0}; }, PT_EINVAL, {"env_of_view"}, false},
    // two at once: the stray mapping before a bad range; a bad description before the set
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.emap = {0, 0, 0}, c.frames = {{0, 1}, {1, 1}, {1, 1}}; }, PT_EINVAL, {"env_of_view must be NULL"}, false},
    {Kind::kBatch, [](Call& c) { c.scenes[0].nquads = 13, c.a.envs = kFakeSet; }, PT_EINVAL, {"scene 0"}, false},
    // nothing to render
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.job.nframes = 0; }, PT_OK, {nullptr}, true},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.job.nrows = 0; }, PT_OK, {nullptr}, true},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.frames = {{1, 0}, {100, 0}, {7, 0}}; }, PT_OK, {nullptr}, true},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.job.nrows = 0, c.frames = {{1, 8}, {100, 1}, {7, 17}}; }, PT_OK, {nullptr}, true},
    {Kind::kScenes, [](Call& c) { c.job.nrows = 0; }, PT_OK, {nullptr}, true},
    {Kind::kEnvs, [](Call& c) { c.live_set(3), c.job.nrows = 0; }, PT_OK, {nullptr}, true},
    // something to render
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.frames = {{1, 0}, {100, 1}, {7, 0}}; }, PT_OK, {nullptr}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(); }, PT_OK, {nullptr}, false},
    {Kind::kBatch, [](Call& c) { c.live_set(3), c.frames = {{1, 0}, {100, 1}, {7, 0}}; }, PT_OK, {nullptr}, false},
    {Kind::kBatch, [](Call& c) { c.scenes.clear(), c.job.use_env = 1; }, PT_OK, {nullptr}, false},
};

static void check_checks()
{
    int n = 0;
    for (const Row& r : kRows) {
        ++n;
        Call c;
        if (r.kind != Kind::kViews) c.scenes.resize(3);   // (zeroed: a scene without objects is valid)
        r.change(c);
        c.a.cams = c.null_cams ? nullptr : c.cams.data();
        c.a.nviews = c.nviews != -99 ? c.nviews : (int32_t)c.cams.size();
        c.a.scenes = c.null_scenes || c.scenes.empty() ? nullptr : c.scenes.data();
        c.a.nscenes = c.nscenes != -99 ? c.nscenes : (int32_t)c.scenes.size();
        c.a.scene_of_view = c.smap.empty() ? nullptr : c.smap.data();
        c.a.env_of_view = c.emap.empty() ? nullptr : c.emap.data();
        c.a.frames = c.frames.empty() ? nullptr : c.frames.data();
        const PtV4BatchShape s = pt_v4_batch_shape(r.kind, c.a, c.job.use_env, c.st.env_mode);
        std::vector<float> dist;
        bool nothing = false;
        g_code = 0;
        strcpy(g_msg, "(none)");
        const int rc = pt_v4_batch_check(c.null_job ? nullptr : &c.job, s, c.a, c.st, &dist, &nothing, record);
        bool ok = rc == r.code && (rc == PT_OK || g_code == rc) && (rc != PT_OK || nothing == r.nothing);
        for (const char* w : r.words)
            if (w) ok = ok && (w[0] == '=' ? !strcmp(g_msg, w + 1) : strstr(g_msg, w) != nullptr);
        if (rc == PT_OK) {
            ok = ok && dist.size() == c.cams.size();
            for (size_t v = 0; ok && v < dist.size(); ++v)   // camera.Distance, as pt_v4_set_camera computes it
                ok = dist[v] == 1.0f / tanf(c.cams[v].fov_degrees * 0.5f * 3.14159265359f / 180.0f);
        }
        if (!ok) {
            printf("FAILED check row %d: rc %d (want %d), nothing %d (want %d), message \"%s\"\n", n, rc, r.code, nothing, r.nothing, g_msg);
            ++fails;
        }
    }
    // the camera check alone, as pt_v4_set_camera calls it: no view named
    float d = 0.0f;
    CHECK(pt_v4_check_camera(&kBadCam, &d, -1, record) == PT_EINVAL && !strcmp(g_msg, "fov_degrees 180 outside (0, 180)"));
    CHECK(pt_v4_check_camera(&kCam, &d, -1, record) == PT_OK && d > 0.99f && d < 1.01f);
}

int main()
{
    pt_v4_default_scene_desc(&g_default);
    CHECK(g_default.nquads == 4 && g_default.nspheres == 7 && g_default.nmat == 11);
    check_layouts();
    check_fills();
    check_checks();
    if (fails) printf("%d check(s) FAILED\n", fails);
    else printf("v4 batch rules: all checks hold\n");
    return fails ? 1 : 0;
}
