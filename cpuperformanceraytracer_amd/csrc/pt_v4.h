// pt_v4.h -- the v4 renderer (demofox_path_tracing_optimization_v4.cpp, the reference's shipping
// path, Application.cpp:474): scene tables, launch interface, host scene builder.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernel_pick.h"
#include "pt_v4_skywin.h"

#define PT_V4_MAX_OBJECTS 12   // MAX_OBJECTS / MAX_MATERIALS, v4 :351-352
static_assert(PT_V4_SKYWIN_MAX == PT_V4_MAX_OBJECTS, "one sky-window rectangle per object");

// env modes (global_preprocessor_flags.h:58-59)
#define PT_V4_ENV_NONE_ 0       // USE_ENV_MAP 0: ambient (0.11, 0.1, 0.15), v4 :782
#define PT_V4_ENV_EQUIRECT_ 1   // USE_ENV_MAP 1, USE_ENV_CUBEMAP 0 (default)
#define PT_V4_ENV_CUBEMAP_ 2    // USE_ENV_CUBEMAP 1 (six faces stacked, LoadCubemapTexture)

// QuadSceneObject after PrecomputeQuadData (v4 :256-320): only what TestQuadTrace (:556-637) reads.
struct PtV4Quad {
    float v0[3];
    float n[3];    // normalize(cross(V01, V02))
    float a0[3];   // NxV01 / DetBot   (bottom triangle 0,1,2)
    float a1[3];   // NxV20 / DetBot
    float b0[3];   // NxV30 / DetTop   (top triangle 0,2,3)
    float b1[3];   // NxV02 / DetTop
};

// One row of SceneMaterialSOA (v4 :354-373) as GatherMaterials (:389-427) reads it: 17 f32.
struct PtV4Mat {
    float albedo[3], emissive[3];
    float spec_chance, spec_rough, spec_color[3];
    float ior, refr_chance, refr_rough, refr_color[3];
};
static_assert(sizeof(PtV4Mat) == 17 * sizeof(float), "material row");

struct PtV4Scene {
    int32_t nquads, nspheres;
    PtV4Quad quad[PT_V4_MAX_OBJECTS];
    float sph[PT_V4_MAX_OBJECTS][4];     // PositionAndRadius
    PtV4Mat mat[PT_V4_MAX_OBJECTS];      // by object index (quads first); unused rows zero
};

struct PtV4Job {
    float* buf;                 // device accumulator
    int32_t width, height;      // iResolution
    int32_t col0, ncols;        // pixel columns [col0, col0 + ncols)
    int32_t row_start, row_stride, nrows;
    int32_t layout;             // PtLayout (pt_kernel.h)
    int32_t tile_w, tile_h;     // PT_LAYOUT_TILED_PLANAR8
    uint32_t frame_first;       // iFrame of the first frame (>= 1)
    int32_t nframes;
    int32_t num_bounces;        // c_numBounces (8)
    int32_t env_mode;           // PT_V4_ENV_*_
    int32_t random_jitter;      // USE_RANDOM_JITTER_TEXTURE_SAMPLING
    int32_t rejection;          // USE_UNIT_VECTOR_REJECTION_SAMPLING
    int32_t accumulate;         // ACCUMULATE_FRAMES: fused lerp into the accumulator (else store)
    int32_t fast_exp;           // USE_FAST_APPROXIMATE_EXP: approx_exp_ps (else glibc-exact expf)
    const float* env;           // device texture (H x W x 3), nullptr with PT_V4_ENV_NONE_
    int32_t env_w, env_h;
    unsigned long long* counters;   // COUNT launches: [0] segments, [1] samples, [2] escaped, [3] lane slots
    int32_t default_scene;          // the scene is InitializeScene's: literal-geometry instantiation
    // persistent-grid tile queue and schedule (pt_tile_queue.h; as PtJob, pt_kernel.h)
    unsigned int* queue;            // PT_QUEUE_WORDS words, zero at the launch's start
    unsigned int* queue_next;       // the next launch's words, zeroed by this launch (nullptr: none)
    const uint32_t* order;          // tile schedule (longest first) or nullptr
    const uint32_t* units;
    const uint32_t* nunits;
    uint32_t* cost;                 // per-tile cost written by this launch, or nullptr
    uint32_t* err;                  // PT_ERR_WORDS error words (pt_kernel.h), nullptr = not recorded
    // continuous-tiles pool (pt_v4.hip pt_v4_ct_kernel): pt_ct_wave_floats() f32 per wave for ct_waves
    // waves (the diffuse kernels' slot area, pt_kernel.h); nullptr: the per-tile pool kernel
    float* ct_slots;
    uint32_t ct_waves;
    int32_t ct_force;               // 1: the continuous-tiles kernel for every launch of >= 8 frames (tests)
    uint32_t ct_back_pct;           // the CT kernel: the last-dispatched ct_back_pct % of the grid claims
                                    // its units from the back of its queue group (pt_tile_queue.h)
    // fused output stage (OutputToScreen / OutputToFile after RenderTile, v4 :1562-1564): each
    // pixel's 8-bit value at pix_out[Y * width + X] (full-image rows, the screen's layout), written
    // with its final accumulator value; nullptr: none.  pix_fast_tone: the tonemap flags are the
    // default fast ACES / gamma (the only ones the presenting kernels carry)
    uint32_t* pix_out;
    int32_t pix_xrgb;               // PT_PIXEL_XRGB8 (OutputToScreen) else RGBA8 (OutputToFile)
    int32_t pix_fast_tone;
    // chained launches (pt_v4_render_device_chain): as PtJob's (pt_kernel.h) -- the continuous-tiles
    // kernel only
    uint32_t* tile_epoch;
    uint32_t chain_seq;
    uint32_t chain_wait;
    unsigned long long* started;
    uint32_t chain_delay;
    // pix_out's address mode: 1 = job rows, pix_out[k * ncols + (X - col0)] for the job's row k (a
    // device job's nrows x ncols pixel buffer, pt_v4_render_device_present: the continuous-tiles
    // kernel's presenting instances); 0 = the full image, as above.  (Last: in the struct's tail
    // padding, so no other member's kernel-argument offset moved when it was added.)
    int32_t pix_rows;
    // the camera (camera.Position, camera.Distance: v4 :1500-1501, read by mainImage :1112, :1128) and
    // the sky window of (scene, camera) (pt_v4_skywin.h; nrects -1: none).  Appended: no member above
    // moved.  Read by the generic instances only -- default_scene is set only with the default camera,
    // bit-equal to (0, 0, 40) and 1.0f, which the DEF instances carry as literals (with sky_ray_v4).
    float cam_pos[3];
    float cam_dist;
    PtV4SkyWin sky;
};
static_assert(sizeof(PtV4Job) + sizeof(PtV4Scene) <= 4096, "kernel arguments (job, scene) exceed the 4 KiB limit");

// Scene description in AddQuad/Sphere/MaterialToScene order (v4 :1368-1401).
struct PtV4SceneDesc {
    int32_t nquads, nspheres, nmat;
    float quad[PT_V4_MAX_OBJECTS][4][3];
    float sphere[PT_V4_MAX_OBJECTS][4];
    PtV4Mat mat[PT_V4_MAX_OBJECTS];   // as passed to AddMaterialToScene (before its albedo.x copy)
};

void pt_v4_default_scene_desc(PtV4SceneDesc* d);                   // InitializeScene, v4 :1403-1496
int pt_v4_build_scene(const PtV4SceneDesc* d, PtV4Scene* out);     // PrecomputeQuadData + AddMaterialToScene
bool pt_v4_is_default_geometry(const PtV4Scene& s);                // geometry == pt_v4_default_scene.h
// *presented (optional): the launch also wrote job.pix_out (the fused output stage; only for the
// presenting configuration, pt_v4.hip pt_launch_v4 -- otherwise the caller converts separately)
// *ct_blocks (optional): the grid of the continuous-tiles kernel it launched (0: the per-tile pool, or
// nothing launched) -- a chained launch's gate waits for that many started blocks.
// (as pt_set_chain_polls, for the v4 kernels)
hipError_t pt_v4_set_chain_polls(uint32_t polls);
hipError_t pt_launch_v4(const PtV4Job& job, const PtV4Scene& scene, hipStream_t stream, bool count,
                        bool* presented = nullptr, uint32_t* ct_blocks = nullptr);

// ---- a batch of views in one launch (pt_v4_render_device_views; pt_v4.hip pt_v4_views_kernel) ----
// The per-tile pool's tile queue spans nviews views of one job geometry: entry e is tile e % T of view
// e / T (T = the job's tiles).  What differs per view -- the camera and the sky window of (scene,
// camera) -- is a record of a device table (job and scene already fill most of the 4 KiB of kernel
// arguments; 1024 records are 212 KiB); the view also selects the accumulator slice, job.buf + view *
// nrows * width * 3, and the pixel slice, pix + view * nrows * width.  The job's own cam_pos, cam_dist
// and sky are not read.
struct PtV4View {
    float cam_pos[3];   // camera.Position
    float cam_dist;     // camera.Distance (the host's 1 / tanf, as pt_v4_set_camera's)
    PtV4SkyWin sky;     // pt_v4_skywin_build for (scene, cam_pos); nrects -1: no window
};
static_assert(sizeof(PtV4View) == 16 + sizeof(PtV4SkyWin) && sizeof(PtV4View) % 4 == 0, "a view record is whole dwords");
struct PtV4Views {
    const PtV4View* table;   // device memory, nviews records, read-only while the launch runs
    int32_t nviews;
    uint32_t* pix;           // nviews x nrows x width packed pixels (the default fast ACES / gamma,
                             // job.pix_xrgb), or nullptr: none
    uint32_t grid_cap;       // test knob: at most this many blocks (0: the resident grid)
};

// ---- a batch of scenes in one launch (pt_v4_render_device_scenes; pt_v4.hip pt_v4_scenes_kernel) ----
// A views launch whose views each name a scene: the scene is a record of a device table instead of a
// kernel argument.  Record s holds pt_v4_build_scene's tables of scene s and, per material, the five
// constants of pt_v4.hip's mat_consts -- filled on the device (pt_v4_scenes_prep_kernel, on the launch's
// stream before the render kernel), because they come from the device's rcp sequence and fresnel_m has
// to see the bits it sees in the plain kernels.  View v's scene is scene_of_view[v] (a parallel array of
// the view table: PtV4View and the views kernels stay as they are).  The geometry is read through the
// constant address space (the record's address is wave-uniform), a hit's material row and constants by
// the lane from the record in global memory: no block-wide material table exists in this kernel, so the
// four waves of a block can be on four scenes at once.
#define PT_V4_MATX_FLOATS 5   // pt_v4.hip MatX: r0sq, omr0, rior, nnout, rscc
struct PtV4SceneRec {
    PtV4Scene sc;
    float mx[PT_V4_MAX_OBJECTS][PT_V4_MATX_FLOATS];   // written by pt_v4_scenes_prep_kernel
};
static_assert(sizeof(PtV4SceneRec) % 4 == 0 && sizeof(PtV4SceneRec) == sizeof(PtV4Scene) + PT_V4_MAX_OBJECTS * PT_V4_MATX_FLOATS * 4,
              "a scene record is whole dwords, no padding");
struct PtV4Scenes {
    PtV4SceneRec* table;             // device memory, nscenes records (mx filled by the preparation kernel)
    int32_t nscenes;
    const int32_t* scene_of_view;    // device memory, one entry per view, each in [0, nscenes)
};

// ---- a batch of env maps in one launch (pt_v4_render_device_envs; pt_v4.hip pt_v4_envs_kernel) ----
// A scenes launch whose views each name a texture of an env set (pt_capi.cpp pt_v4_env_set): the texture
// is a record of a device table instead of job.env / env_w / env_h, which are not read.  View v's texture
// is env_of_view[v] (a parallel array of the view table, like scene_of_view).  The record is read through
// the constant address space at a wave-uniform address -- pointer, width and height together -- when the
// wave takes a tile; how it is sampled (equirect / stacked cubemap) stays job.env_mode.
struct PtV4EnvRec {
    const float* data;   // device texels, H x W x 3 f32
    int32_t w, h;
};
static_assert(sizeof(PtV4EnvRec) == 16, "an env record is 16 B");
struct PtV4Envs {
    const PtV4EnvRec* table;       // device memory, nenvs records, immutable while the set lives
    int32_t nenvs;
    const int32_t* env_of_view;    // device memory, one entry per view, each in [0, nenvs)
};

// ---- a batch with a frame range per view (pt_v4_render_device_batch; pt_v4.hip pt_v4_batch_kernel) ----
// The superset of the three launches above: a view is (camera, scene, environment, frame range).  View v
// renders frames [frame_first, frame_first + nframes) of its own -- a parallel array of 8-byte records,
// like scene_of_view and env_of_view (PtV4View stays as it is).  A wave reads its view's record when it
// takes a tile: one 8-byte read through the constant address space at a wave-uniform address, so first
// frame and count change together and live in scalar registers.  job.frame_first and job.nframes are not
// read.  A view of 0 frames keeps its accumulator (loaded, not stored) and still packs its pixels.
// With an env term (job.env_mode not NONE) the texture is always a record of `envs`, as in an envs launch
// (the host stages a one-record table for pt_set_env_map's texture); without one `envs` is not read.
struct PtV4FrameRange {
    uint32_t frame_first;   // iFrame of the view's first frame (>= 1)
    int32_t nframes;        // >= 0; frame_first + nframes <= 2^24
};
static_assert(sizeof(PtV4FrameRange) == 8, "a frame range record is 8 B");
struct PtV4Frames {
    const PtV4FrameRange* range_of_view;   // device memory, one record per view
};

// ---- per-view statistics of a batch (pt_v4_render_device_batch_stats; pt_v4.hip pt_v4_batch_stats_kernel) ----
// How much each view's DISPLAYED image moved in the launch: `before` is the 8-bit value (pt_tonemap.h, the default
// fast ACES / gamma) of a pixel's accumulator as the launch finds it, `after` of the value it stores; R, G, B only.
// At a tile's end each lane with a pixel packs both, the wave reduces (pt_v4_stats.h) and one lane issues three
// integer atomics on the view's record -- one tile is one wave and one view.  The old value is re-read from the
// slice just before the store (the slice is untouched until then: one writer per pixel), so nothing more is live
// through the pool loop.  A view of 0 frames issues nothing: the host cleared the records on the stream.
struct PtV4ViewStats {
    unsigned long long sum_delta;   // sum over pixels and R, G, B of |after - before|
    uint32_t changed;               // pixels whose R, G, B differ
    uint32_t max_delta;             // largest |after - before| of one channel
};
static_assert(sizeof(PtV4ViewStats) == 16, "a statistics record is 16 B");
struct PtV4Stats {
    PtV4ViewStats* of_view;   // device memory, one record per view, zero at the launch's start
};

// ---- the one launch of the four kinds above (pt_kernel_pick.h PtV4BatchKind, kPtV4BatchedKeys) ----
// The generic instances (ENV x row layout x FEXP) of the kind's kernel, unscheduled (job.order, units, cost:
// nullptr) and uncounted, a plain launch on `stream`; job.ncols == job.width, job.col0 == 0 (a device job);
// views.grid_cap honoured.  What a kind reads must be there, the rest may be nullptr:
//   kViews   `scene` (a kernel argument); job.env / env_w / env_h with an env term
//   kScenes  `scenes`; job.env / env_w / env_h with an env term
//   kEnvs    `scenes`, `envs`; job.env_mode is not NONE; job.env, env_w and env_h are not read
//   kBatch   `scenes`, `frames`, and with an env term `envs`; job.env, env_w, env_h, frame_first and nframes
//            are not read (the caller launches only when some view has frames)
// Every kind but kViews runs the preparation kernel (pt_v4_scenes_prep_kernel) on the stream first.
// `stats` (kBatch only, else hipErrorInvalidValue): the kind's statistics instances (kPtV4BatchStatsKeys), which
// also add each view's statistics to stats->of_view; nullptr: the instances above.
hipError_t pt_launch_v4_batched(PtV4BatchKind kind, const PtV4Job& job, const PtV4Scene* scene, const PtV4Views& views,
                                const PtV4Scenes* scenes, const PtV4Envs* envs, const PtV4Frames* frames, hipStream_t stream,
                                const PtV4Stats* stats = nullptr);
