// pt_v4_batch.h -- the rules of a batched v4 launch (pt_v4_render_device_views / _scenes / _envs / _batch;
// pt_v4.h PtV4Views ... PtV4Frames), each once, as functions of plain inputs: what a launch reads (its
// shape), where that lies in the staging block (its layout), every argument check made before the first
// HIP call, and the block's contents.  Host only -- no HIP call, no global: what is process-wide arrives as
// a PtV4BatchState.  pt_capi.cpp and the host check (tests/native/check_v4_batch.cpp) share it.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "pt_kernel.h"   // PT_TILE_MASK
#include "pt_v4.h"
#include "../../include/pt_mi355.h"

constexpr uint32_t kMaxFrame = 1u << 24;   // iFrame is an f32 counter: exact below 2^24
constexpr int32_t kMaxDim = 1 << 24;        // pixel coordinates are f32 in mainImage: exact up to 2^24

// How a check reports: the library's `fail` (it keeps the message for pt_last_error and returns the code).
typedef int (*PtFail)(int code, const char* fmt, ...);

// ---- the shape: what a launch of `kind` with these arguments reads ---------------------------------
//   kViews   a camera per view; every view renders the process-wide scene, a kernel argument
//   kScenes  the scene per view as well: records, and the view -> scene mapping
//   kEnvs    the texture per view as well: record env_of_view[v] of the env set's device table; `scenes`
//            may be NULL (every view renders the process-wide scene, which then travels as the one record)
//   kBatch   the frame range per view as well -- `frames`, or the job's range for every view.  A texture
//            per view when a set is given; without a set but with an env term the process-wide map travels
//            as a one-record table (with a mapping of zeros), so that the kernel reads a table either way.
struct PtV4BatchShape {
    bool scene_recs;      // scene records travel in the block
    bool scene_map;       // and the view -> scene mapping
    bool env_map;         // the view -> texture mapping
    bool staged_env;      // the one-record env table (pt_set_env_map's texture), mapping all zeros
    bool frames;          // a frame range per view
    bool current_scene;   // the process-wide scene stands in for `scenes` (one record, every view maps to it)
    bool env_set() const { return env_map && !staged_env; }   // the textures come from the caller's env set
};
inline PtV4BatchShape pt_v4_batch_shape(PtV4BatchKind kind, const pt_v4_batch& a, int32_t use_env, int32_t env_mode)
{
    const bool views = kind == PtV4BatchKind::kViews, batch = kind == PtV4BatchKind::kBatch;
    const bool with_set = kind == PtV4BatchKind::kEnvs || (batch && a.envs);
    const bool staged = batch && !a.envs && use_env && env_mode != PT_V4_ENV_NONE;
    return {!views, !views, with_set || staged, staged, batch, (with_set || batch) && !a.scenes};
}
// The records of a launch: a views launch has none, the process-wide scene is one.
inline int32_t pt_v4_batch_nscenes(const PtV4BatchShape& s, const pt_v4_batch& a)
{
    return !s.scene_recs ? 0 : s.current_scene ? 1 : a.nscenes;
}

// ---- the layout: the sections of the staging block, in this order, each on a 16-byte boundary -------
// scene records | view table | view -> scene | view -> texture | staged env record | frame ranges.  A
// section the shape does not have is empty (a views block is the view table alone, at 0).
struct PtV4BatchLayout {
    size_t scenes, views, scene_map, env_map, env_rec, frames;   // byte offsets
    size_t need;                                                 // bytes of the block
};
inline PtV4BatchLayout pt_v4_batch_layout(const PtV4BatchShape& s, int32_t nscenes, int32_t nviews)
{
    const auto up16 = [](size_t n) { return (n + 15u) & ~(size_t)15u; };
    const size_t nv = (size_t)nviews;
    PtV4BatchLayout l{};
    l.scenes = 0;
    l.views = l.scenes + (s.scene_recs ? up16((size_t)nscenes * sizeof(PtV4SceneRec)) : 0u);
    l.scene_map = l.views + up16(nv * sizeof(PtV4View));
    l.env_map = l.scene_map + (s.scene_map ? up16(nv * sizeof(int32_t)) : 0u);
    l.env_rec = l.env_map + (s.env_map ? up16(nv * sizeof(int32_t)) : 0u);
    l.frames = l.env_rec + (s.staged_env ? up16(sizeof(PtV4EnvRec)) : 0u);
    l.need = l.frames + (s.frames ? up16(nv * sizeof(PtV4FrameRange)) : 0u);
    return l;
}
// A section of the block at `base` -- the host copy to fill it, the device copy for the kernel's arguments.
inline PtV4SceneRec* pt_v4_batch_scenes(unsigned char* base, const PtV4BatchLayout& l) { return reinterpret_cast<PtV4SceneRec*>(base + l.scenes); }
inline PtV4View* pt_v4_batch_views(unsigned char* base, const PtV4BatchLayout& l) { return reinterpret_cast<PtV4View*>(base + l.views); }
inline int32_t* pt_v4_batch_scene_map(unsigned char* base, const PtV4BatchLayout& l) { return reinterpret_cast<int32_t*>(base + l.scene_map); }
inline int32_t* pt_v4_batch_env_map(unsigned char* base, const PtV4BatchLayout& l) { return reinterpret_cast<int32_t*>(base + l.env_map); }
inline PtV4EnvRec* pt_v4_batch_env_rec(unsigned char* base, const PtV4BatchLayout& l) { return reinterpret_cast<PtV4EnvRec*>(base + l.env_rec); }
inline PtV4FrameRange* pt_v4_batch_frames(unsigned char* base, const PtV4BatchLayout& l) { return reinterpret_cast<PtV4FrameRange*>(base + l.frames); }

// ---- the checks -------------------------------------------------------------------------------------
// The process-wide facts a batched launch depends on.
struct PtV4BatchState {
    int32_t env_mode;               // pt_v4_config.env_mode
    bool env_live;                  // the batch's `envs` is a live env set (it is dereferenced by nobody else)
    int32_t env_count;              // its textures (0 unless live)
    const PtV4SceneDesc* current;   // the process-wide scene's description
    bool skywin_off;                // PT_MI355_V4_SKYWIN=0: no sky windows
};

// The geometry / frame checks of every device job (the scalar-path jobs' and v4's).
inline int pt_check_device_job(const pt_device_job* dj, PtFail fail)
{
    if (!dj || !dj->buf) return fail(PT_EINVAL, "null device job/buffer");
    if (dj->width <= 0 || dj->height <= 0 || dj->nrows < 0 || dj->row_stride <= 0 || dj->row_start < 0)
        return fail(PT_EINVAL, "invalid device job geometry");
    if (dj->width > kMaxDim || dj->height > kMaxDim)
        return fail(PT_EINVAL, "image side > 2^24 (f32 pixel coordinates inexact)");
    if (dj->nrows > 0 && dj->row_start + (int64_t)(dj->nrows - 1) * dj->row_stride >= dj->height)
        return fail(PT_EINVAL, "row shard exceeds the image height");
    if (dj->layout != PT_LAYOUT_INTERLEAVED && dj->layout != PT_LAYOUT_PLANAR8)
        return fail(PT_EINVAL, "device jobs support the interleaved and planar8 layouts");
    if (dj->layout == PT_LAYOUT_PLANAR8 && dj->width % 8) return fail(PT_EINVAL, "planar8 needs width % 8 == 0");
    if (dj->frame_first < 1 || dj->nframes < 0 || (uint64_t)dj->frame_first + (uint64_t)dj->nframes > kMaxFrame)
        return fail(PT_EINVAL, "frame range [%u, +%d) invalid", dj->frame_first, dj->nframes);
    if (dj->num_bounces < 0 || dj->num_bounces > 1024) return fail(PT_EINVAL, "num_bounces out of range");
    return PT_OK;
}

// camera.Distance of InitializeCamera (v4 :1500): 1.0f / tanf(c_FOVDegrees * 0.5f * c_pi / 180.0f) in
// f32, c_pi = 3.14159265359f (mathutils.h:5); glibc tanf for MSVC's float overload
inline float pt_v4_camera_distance(float fov_degrees)
{
    const float c_pi = 3.14159265359f;
    return 1.0f / tanf(fov_degrees * 0.5f * c_pi / 180.0f);
}

// The camera check of pt_v4_set_camera and of every view of a batched launch (view >= 0: the message
// names it); *dist: camera.Distance.
inline int pt_v4_check_camera(const pt_v4_camera* c, float* dist, int view, PtFail fail)
{
    char who[32] = "";
    if (view >= 0) snprintf(who, sizeof(who), "view %d: ", view);
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(c->position[k]) || std::fabs(c->position[k]) > 1024.0f)
            return fail(PT_EINVAL, "%scamera position[%d] = %g is not finite or beyond +-1024", who, k, (double)c->position[k]);
    if (!std::isfinite(c->fov_degrees) || !(c->fov_degrees > 0.0f && c->fov_degrees < 180.0f))
        return fail(PT_EINVAL, "%sfov_degrees %g outside (0, 180)", who, (double)c->fov_degrees);
    *dist = pt_v4_camera_distance(c->fov_degrees);
    if (!(std::isnormal(*dist) && *dist > 0.0f))
        return fail(PT_EINVAL, "%sfov_degrees %g gives the camera distance %g, not a finite positive normal f32", who,
                    (double)c->fov_degrees, (double)*dist);
    return PT_OK;
}

// The description a launch's scene s is built from.
inline const PtV4SceneDesc* pt_v4_batch_descs(const PtV4BatchShape& s, const pt_v4_batch& a, const PtV4BatchState& st)
{
    return s.current_scene ? st.current : reinterpret_cast<const PtV4SceneDesc*>(a.scenes);   // (pt_v4_scene_desc is PtV4SceneDesc)
}

// Every argument check of a batched launch, in the order the callers know (tests/test_abi_v4_*.py pin it).
// PT_OK: *dist holds each view's camera distance, and *nothing says that no view has a pixel to render (no
// frames anywhere, or no rows) -- the caller then launches nothing.
inline int pt_v4_batch_check(const pt_device_job* dj, const PtV4BatchShape& s, const pt_v4_batch& a, const PtV4BatchState& st,
                             std::vector<float>* dist, bool* nothing, PtFail fail)
{
    int rc;
    const int32_t nviews = a.nviews;
    const pt_v4_frame_range* const frames = s.frames ? a.frames : nullptr;
    *nothing = false;
    if (!dj) return fail(PT_EINVAL, "null device job");
    {
        pt_device_job geo = *dj;
        if (frames) {   // (the job's own range is not read: each view's is checked below)
            geo.frame_first = 1;
            geo.nframes = 0;
        }
        if ((rc = pt_check_device_job(&geo, fail))) return rc;
    }
    if (!a.cams) return fail(PT_EINVAL, "null camera array");
    if (nviews < 1 || nviews > PT_V4_MAX_VIEWS) return fail(PT_EINVAL, "nviews %d outside [1, %d]", nviews, PT_V4_MAX_VIEWS);
    if (a.pixels && a.format != PT_PIXEL_RGBA8 && a.format != PT_PIXEL_XRGB8) return fail(PT_EINVAL, "unknown pixel format %d", a.format);
    const uint64_t view_tiles = (uint64_t)((dj->width + 7) / 8) * (uint64_t)((dj->nrows + 7) / 8);
    if (view_tiles * (uint64_t)nviews > PT_TILE_MASK)
        return fail(PT_EINVAL, "%d views x %llu tiles exceed the tile queue's %u entries", nviews, (unsigned long long)view_tiles,
                    PT_TILE_MASK);
    dist->assign((size_t)nviews, 0.0f);
    for (int32_t v = 0; v < nviews; ++v)
        if ((rc = pt_v4_check_camera(&a.cams[v], &(*dist)[(size_t)v], v, fail))) return rc;
    if (s.current_scene && (a.nscenes != 0 || a.scene_of_view))
        return fail(PT_EINVAL, "no scenes (the current scene): nscenes must be 0 and scene_of_view NULL");
    const int32_t nscenes = pt_v4_batch_nscenes(s, a);
    const PtV4SceneDesc* const desc = pt_v4_batch_descs(s, a, st);
    if (s.scene_recs) {
        if (!desc) return fail(PT_EINVAL, "null scene array");
        if (nscenes < 1 || nscenes > PT_V4_MAX_VIEWS) return fail(PT_EINVAL, "nscenes %d outside [1, %d]", nscenes, PT_V4_MAX_VIEWS);
        if (!a.scene_of_view && !s.current_scene && nscenes != nviews)
            return fail(PT_EINVAL, "no scene_of_view: view v uses scene v, but nscenes %d != nviews %d", nscenes, nviews);
        if (a.scene_of_view)
            for (int32_t v = 0; v < nviews; ++v)
                if (a.scene_of_view[v] < 0 || a.scene_of_view[v] >= nscenes)
                    return fail(PT_EINVAL, "view %d: scene_of_view %d outside [0, %d)", v, a.scene_of_view[v], nscenes);
    }
    for (int32_t i = 0; i < nscenes; ++i) {
        const PtV4SceneDesc& d = desc[i];
        if (d.nquads < 0 || d.nspheres < 0 || d.nmat < 0 || d.nquads > PT_V4_MAX_OBJECTS || d.nspheres > PT_V4_MAX_OBJECTS ||
            d.nquads + d.nspheres > PT_V4_MAX_OBJECTS || d.nmat > PT_V4_MAX_OBJECTS)
            return fail(PT_EINVAL, "scene %d: %d quads + %d spheres, %d materials (each count >= 0; objects and materials <= %d)", i,
                        d.nquads, d.nspheres, d.nmat, PT_V4_MAX_OBJECTS);
    }
    const bool env_term = dj->use_env && st.env_mode != PT_V4_ENV_NONE;
    if (s.frames && a.envs && !env_term)   // (a batch call: before the set is looked at)
        return fail(PT_EINVAL, "an env set needs an env term: use_env %d, v4 env mode %d", dj->use_env, st.env_mode);
    if (s.env_set()) {
        if (!a.envs) return fail(PT_EINVAL, "null env set");
        if (!st.env_live) return fail(PT_EINVAL, "not a live env set (freed, or from before pt_shutdown)");
        if (!a.env_of_view && st.env_count != nviews)
            return fail(PT_EINVAL, "no env_of_view: view v uses texture v, but the set has %d textures for %d views", st.env_count, nviews);
        if (a.env_of_view)
            for (int32_t v = 0; v < nviews; ++v)
                if (a.env_of_view[v] < 0 || a.env_of_view[v] >= st.env_count)
                    return fail(PT_EINVAL, "view %d: env_of_view %d outside [0, %d)", v, a.env_of_view[v], st.env_count);
        if (!env_term) return fail(PT_EINVAL, "an envs launch needs an env term: use_env %d, v4 env mode %d", dj->use_env, st.env_mode);
    }
    if (s.frames) {
        if (!a.envs && a.env_of_view) return fail(PT_EINVAL, "no env set (the process-wide env map, or none): env_of_view must be NULL");
        bool any = false;
        for (int32_t v = 0; v < nviews; ++v) {
            const pt_v4_frame_range r = frames ? frames[v] : pt_v4_frame_range{dj->frame_first, dj->nframes};
            if (r.frame_first < 1 || r.nframes < 0 || (uint64_t)r.frame_first + (uint64_t)r.nframes > kMaxFrame)
                return fail(PT_EINVAL, "view %d: frame range [%u, +%d) invalid", v, r.frame_first, r.nframes);
            any = any || r.nframes > 0;
        }
        *nothing = !any || dj->nrows == 0;
    } else {
        *nothing = dj->nframes == 0 || dj->nrows == 0;
    }
    return PT_OK;
}

// The sky window of scene `d` seen from `position` (pt_v4_skywin.h); off: none (A/B timing, tests).
inline void pt_v4_sky_window_for(bool off, const PtV4SceneDesc& d, const float position[3], PtV4SkyWin* out)
{
    if (off) *out = PtV4SkyWin{-1, {}};
    else pt_v4_skywin_build(d.nquads, d.quad, d.nspheres, d.sphere, position, out);
}

// ---- the fill ----------------------------------------------------------------------------------------
// One block of pt_v4_batch_layout(...).need bytes at `base`, for arguments pt_v4_batch_check passed (`dist`
// is its result).  Scene records are pt_v4_build_scene of their descriptions -- the code behind pt_v4_add_* --
// with mx zeroed (the preparation kernel fills them on the device); view v's sky window is
// pt_v4_skywin_build of (its scene, its camera).  `staged`: the record of a staged env table.
inline int pt_v4_batch_fill(unsigned char* base, const PtV4BatchLayout& l, const PtV4BatchShape& s, const pt_device_job& dj,
                            const pt_v4_batch& a, const PtV4BatchState& st, const float* dist, const PtV4EnvRec& staged, PtFail fail)
{
    const int32_t nscenes = pt_v4_batch_nscenes(s, a);
    const PtV4SceneDesc* const desc = pt_v4_batch_descs(s, a, st);
    PtV4SceneRec* const rec = pt_v4_batch_scenes(base, l);
    for (int32_t i = 0; i < nscenes; ++i) {
        if (pt_v4_build_scene(&desc[i], &rec[i].sc)) return fail(PT_EINVAL, "scene %d exceeds MAX_OBJECTS", i);   // (checked before)
        memset(rec[i].mx, 0, sizeof(rec[i].mx));
    }
    PtV4View* const view = pt_v4_batch_views(base, l);
    for (int32_t v = 0; v < a.nviews; ++v) {
        const int32_t sc = a.scene_of_view ? a.scene_of_view[v] : s.current_scene ? 0 : v;
        if (s.scene_map) pt_v4_batch_scene_map(base, l)[v] = sc;
        if (s.env_map) pt_v4_batch_env_map(base, l)[v] = s.staged_env ? 0 : a.env_of_view ? a.env_of_view[v] : v;
        if (s.frames)
            pt_v4_batch_frames(base, l)[v] = a.frames ? PtV4FrameRange{a.frames[v].frame_first, a.frames[v].nframes}
                                                      : PtV4FrameRange{dj.frame_first, dj.nframes};
        PtV4View& r = view[v];
        memcpy(r.cam_pos, a.cams[v].position, sizeof(r.cam_pos));
        r.cam_dist = dist[v];
        // (a views launch renders the process-wide scene)
        pt_v4_sky_window_for(st.skywin_off, s.scene_recs ? desc[sc] : *st.current, a.cams[v].position, &r.sky);
    }
    if (s.staged_env) *pt_v4_batch_env_rec(base, l) = staged;
    return PT_OK;
}
