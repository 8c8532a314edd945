// pt_capi.cpp -- the C ABI of libpt_mi355.so (include/pt_mi355.h): validation, frame state,
// host<->device buffer mirroring, dispatch to the HIP kernels (pt_kernel.hip, pt_v4.hip,
// pt_output.hip), and the fan-out of every host-buffer entry point over one or several GPUs.
//
// Reference behaviour mirrored here (paths relative to CPUPerformanceRayTracer/):
//   - frame counter: `static f32 iFrame; iFrame += 1` before rendering (scalar.cpp:798-799,
//     simd.cpp:483-484, simd_tiled.cpp:547);
//   - settings checks of ApplicationState::CheckValidSettings (Application.cpp:36-94), returned
//     as PT_EINVAL instead of __debugbreak();
//   - the caller owns the host buffer, the call returns after it is updated (Application.cpp:474).
//
// Several devices (pt_config.device_count > 1, or PT_MI355_DEVICES): the reference fans a frame's
// tiles out over its CPU threads (simd_tiled.cpp:549-571, v4 :1696-1721); here a frame's ROWS are
// dealt to the devices, row Y to device Y mod N (neighbouring rows cost alike, so every device gets
// the same mix of cheap sky rows and expensive rows into the box).  Every pixel's value depends only
// on its global (x, y) and the frame, so any split renders bit-identical pixels.  Each device keeps
// its own mirror of its rows: a compact sub-image for the row layouts (interleaved, planar8) and a
// full-size buffer of which it owns the rows for the tiled layout (whose rows are not contiguous in
// the host buffer); transfers move only the owned rows (pitched 2D copies).
#include "pt_kernel.h"
#include "pt_guard.h"
#include "pt_kernel_pick.h"
#include "pt_launch_plan.h"
#include "pt_output.h"
#include "pt_v4.h"
#include "pt_v4_batch.h"
#include "../../include/pt_mi355.h"
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <new>
#include <vector>

namespace {

// Tile schedule of a recurring job geometry: the previous launch's per-tile costs, and the order
// built from them (longest tiles first) for the next launch on the same stream.  Per-pixel work
// varies ~10x across the image (rays inside the box bounce, sky rays stop), and with the tiles
// taken in raster order the last-dequeued expensive tiles left most of the chip idle at the end.
// The geometry a schedule belongs to (which renderer, which pixels, how many bounces, which env).
struct SchedKey {
    int32_t kind = 0;   // 0: the diffuse kernels; 1 + env mode: v4
    int32_t width = 0, height = 0, col0 = 0, ncols = 0, row_start = 0, row_stride = 0, nrows = 0, bounces = 0;
    const float* env = nullptr;
    uint32_t ntiles = 0;
    uint32_t split = 0;   // the schedule builder's split factor (pt_plan_split: one-chunk launches only)
    bool operator==(const SchedKey& o) const
    {
        return kind == o.kind && width == o.width && height == o.height && col0 == o.col0 && ncols == o.ncols &&
               row_start == o.row_start && row_stride == o.row_stride && nrows == o.nrows && bounces == o.bounces &&
               env == o.env && ntiles == o.ntiles && split == o.split;
    }
};
struct Sched {
    bool used = false;
    hipStream_t stream = nullptr;
    SchedKey key;
    uint32_t* cost = nullptr;
    uint32_t* order = nullptr;
    uint32_t* units = nullptr;    // 2 ntiles + 2 words: run starts, then the run count (cost: 2 ntiles words,
                                  // order: up to 2 ntiles entries -- split tiles, pt_tile_queue.h)
    uint32_t* nunits() const { return units + 2 * (size_t)key.ntiles + 1; }
    bool have_cost = false;
    bool built = false;           // order/units hold a schedule
    unsigned long long launches = 0;
    unsigned long long last_use = 0;
    // launch variant of the diffuse continuous-tiles kernel (PT_MI355_CT_WAVES=0, the default): the
    // first scheduled launches time the arms (ct_occupancy) between event pairs, the fastest is kept
    hipEvent_t tune_ev[2 * 18] = {};
    uint32_t tuned = 0;           // timed launches enqueued
    uint32_t narms = 0;           // arms timed (2 or 3; 0: not started)
    int32_t tune_nframes = 0;     // the frames of the first timed launch: only launches of that length are timed
    int8_t wide = -1;             // the pick: arm index (-1: not yet)
    // chained launches (launch_chain): per half-tile, the chain sequence number of the last launch
    // that stored its pixels (2 ntiles words), and that number of the geometry's last chained launch
    uint32_t* epoch = nullptr;
    uint32_t chain_seq = 0;
    // camera-hit cache (pt_kernel.h PtJob::cam_cache): one record per pixel of the
    // geometry's tiles, allocated and filled by its first uncounted continuous-tiles launch of at least
    // kCamMinFrames frames.  The records depend on the key's pixels (width .. nrows) and on the scene,
    // which is uploaded once, when the device is set up and has no schedules yet -- so a cache lives
    // at most as long as its Sched.  nullptr: none (yet); cam_off: the allocation failed, never again.
    unsigned long long* cam = nullptr;
    bool cam_off = false;
    uint8_t cam_state = kCamEmpty;   // (pt_launch_plan.h)
};
constexpr int kSchedSlots = 16;
constexpr int kBands = 4;   // PT_FLAG_PIN_HOST: row bands of a pipelined frame
constexpr unsigned kQueueRing = 256;       // tile-queue ring slots (reuse across streams is event-ordered)
constexpr unsigned kViewRing = 4;          // staging blocks of the batched v4 launches (Dev::batch)
// launches per schedule build (g.sched_rebuild; PT_MI355_SCHED_REBUILD): 256 -- a build restarts the
// chained overlap and costs a one-workgroup kernel (~57 us at 1080p); 3-round A/B of chained steps vs 64
// (profiles/r06/r06zl_*): c2 0.2160 vs 0.2189 ms, c4 0.4582 vs 0.4633, v4 0.3286 vs 0.3313
constexpr unsigned long long kSchedRebuildDefault = 256;

// One (logical) device: its streams, scene, tile queues, schedules, env map and the mirror of its
// share of the caller's host accumulator.  Several logical devices may name the same HIP device
// (tests shard a frame over N logical devices on one GPU).
struct Dev {
    int32_t ordinal = 0;
    hipStream_t stream = nullptr;
    PtScene* dscene = nullptr;          // device copy of State::scene
    float* dbuf = nullptr;              // mirror of this device's rows of the host accumulator
    size_t dbuf_cap = 0;
    unsigned long long* dcounters = nullptr;
    uint32_t* derr = nullptr;           // PT_ERR_WORDS kernel error words (PtJob::err)
    float* dct = nullptr;               // continuous-tiles pool slots (PtJob::ct_slots), for dct_waves waves
    uint32_t dct_waves = 0;
    int ct_slot = -1;                   // tile-queue ring slot of the last launch that used dct (its event
                                        // orders the next such launch on another stream: one set of slots)
    uint32_t* herr = nullptr;           // their page-locked host copy (read at every synchronisation)
    unsigned int* dqueue = nullptr;     // ring of kQueueRing tile-queue blocks (PT_QUEUE_WORDS each)
    unsigned queue_next = 0;
    bool queue_pre_zeroed = false;      // the last launch's kernel zeroes ring slot queue_next % kQueueRing
    hipStream_t last_stream = nullptr;  // the stream of the last launch
    // per ring slot: the stream of the last launch that used it and an event recorded after that
    // launch; a launch on another stream waits for it before re-zeroing the slot
    hipStream_t queue_stream[kQueueRing] = {};   // (compared for equality only, never used: it may be
    hipEvent_t queue_event[kQueueRing] = {};     //  a caller's stream that no longer exists)
    // a slot skipped by a change of stream is ordered by the event of the slot before it (recorded
    // after the launch whose kernel zeroes the skipped slot): its index, or -1
    int16_t queue_alias[kQueueRing];
    float* denv = nullptr;              // env map in HBM (pt_set_env_map / textured / v4)
    Sched sched[kSchedSlots];
    unsigned long long sched_clock = 0;
    unsigned long long cam_checked = 0;   // pt_cam_cache_query: records the last pt_count_device launch compared
    float* dtone_in = nullptr;          // output stage scratch
    size_t dtone_in_cap = 0;
    uint32_t* dtone_out = nullptr;
    size_t dtone_out_cap = 0;
    // PT_FLAG_GATHER_ROOT: the root (device 0) assembles the whole accumulator from every device's
    // rows -- each device stores its rows into dgather of the root over xGMI (peer access)
    float* dgather = nullptr;           // root only: W x H x 3
    size_t dgather_cap = 0;
    hipEvent_t ev_gather = nullptr;     // recorded after this device's rows were stored
    bool peer_root = false;             // this device may store into the root's memory
    // batched v4 launches (pt_v4_render_device_views / _scenes / _envs / _batch): a ring of kViewRing blocks
    // shared by the four calls.  A launch fills the next slot's page-locked host block, copies it to the
    // slot's device block on its stream and records the slot's event after its kernel; a slot is reused
    // only once that event has completed (the host waits for it -- four launches back, normally long
    // done).  So a block that an earlier asynchronous launch may still be reading, on this stream or
    // another, is never written, and no stream is made to wait for another.  The block holds what the
    // launch's kind needs (pt_v4_batch.h PtV4BatchLayout).  A block has the size its largest launch so far
    // needed (a scene record is ~2 KiB: 1024 of them ~2 MiB), grown only after the slot's event completed.
    struct BatchSlot {
        unsigned char* host = nullptr;  // page-locked
        unsigned char* dev = nullptr;
        size_t cap = 0;                 // bytes of each
        hipEvent_t done = nullptr;
        bool pending = false;           // done has been recorded
        // pt_v4_render_device_batch_stats under a tonemap pair the render kernel does not fuse: the old slices'
        // packed pixels (nviews x nrows x width u32), written before the render and read by the compare pass
        // after it; grown like the block, and `done` is recorded after that pass
        uint32_t* before = nullptr;
        size_t before_cap = 0;          // u32 elements
    } batch[kViewRing];
    unsigned batch_next = 0;
    // chained launches (pt_render_device_chain, launch_chain): consecutive launches of one geometry
    // alternate on two streams of the library's and overlap on the GPU
    struct Chain {
        hipStream_t st[2] = {};            // the two streams (non-blocking)
        hipEvent_t done[2] = {};           // recorded after each stream's last launch
        bool pending[2] = {};              // done[i] has been recorded
        hipEvent_t ev_caller = nullptr;    // the caller's stream at a chain (re)start
        float* area1 = nullptr;            // a second continuous-tiles slot area (the first: dct)
        unsigned int* qblk = nullptr;      // 4 tile-queue blocks of the continuing launches
        // blocks started by every chained launch so far (monotonic: a stream gate that is evaluated
        // before a restart's launch has started -- its stream waits only for the gate -- must not pass
        // on a count from before the restart), and the blocks those launches have
        unsigned long long* started = nullptr;
        unsigned long long cum = 0;
        Sched* sched = nullptr;            // the live chain's geometry (nullptr: the next chained launch restarts)
        int area = 0;                      // slot area of the live chain's last launch (0: dct, 1: area1)
        int par = 0;                       // stream of the live chain's last launch
        unsigned long long restarts = 0, continued = 0;   // chained launches of each kind (pt_chain_counts)
        // a chained launch's wait ran out on this device (guard PT_G_CHAIN_WAIT, reported by sync_all):
        // chained calls are plain launches from then on ("Residency")
        bool off = false;
    } chain;
};

// The host buffer the device mirrors currently represent, and the geometry they were split by.
struct Mirror {
    const float* host = nullptr;
    size_t bytes = 0;
    int32_t width = 0, height = 0;
    bool tiled = false;
    int32_t tile_w = 0, tile_h = 0;
    bool valid = false;                 // deferred mode: the device copies are authoritative
};

}  // namespace

// An env set (include/pt_mi355.h): `count` textures resident on one device, and their record table.
struct pt_v4_env_set {
    Dev* dev = nullptr;                 // the device of views and scenes launches that holds it
    unsigned char* block = nullptr;     // the one device allocation: table, then texels
    const PtV4EnvRec* table = nullptr;  // == block
    int32_t count = 0;
    pt_v4_env_set* next = nullptr;      // State::env_sets
};

namespace {

struct State {
    bool inited = false;
    pt_config cfg{};
    int ndev = 0;
    Dev dev[PT_MAX_DEVICES];
    PtScene scene{};
    uint32_t frame = 0;                 // value of the reference's static iFrame
    Mirror m;
    // env map (the same texture on every device)
    const float* env_src = nullptr;     // host data the device copies were made from
    int32_t env_w = 0, env_h = 0;
    bool have_env = false;
    pt_v4_env_set* env_sets = nullptr;  // the live env sets (pt_v4_make_env_set), newest first
    // PT_FLAG_PIN_HOST (one device): the registered host buffer, copy streams and band events
    const float* pinned = nullptr;
    size_t pinned_bytes = 0;
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t ev_in[kBands] = {}, ev_done[kBands] = {};
    hipEvent_t ev_q = nullptr;          // work queues: orders banded copies against the stream
    hipEvent_t ev_root_free = nullptr;  // PT_FLAG_GATHER_ROOT: the root's earlier reads of dgather are done
    // v4 renderer (demofox_path_tracing_optimization_v4.cpp): its own iFrame (v4 :34) and scene
    pt_v4_config v4cfg{PT_V4_ENV_EQUIRECT, 1, 1, 8, 1, 1, 1, 1, 1};
    bool v4_scene_ready = false;
    PtV4SceneDesc v4desc{};
    PtV4Scene v4scene{};
    uint32_t v4_frame = 0;
    // the v4 camera (pt_v4_set_camera): InitializeCamera's position and field of view (v4 :1500-1501,
    // :20), the distance computed from it, and the sky window of (v4desc, camera) -- rebuilt by the
    // first job after either changed
    pt_v4_camera v4cam{{0.0f, 0.0f, 40.0f}, 90.0f};
    float v4cam_dist = 1.0f;
    PtV4SkyWin v4sky{-1, {}};
    bool v4sky_ready = false;
    // test hook: PT_MI355_RING_GUARD_CAP (read by pt_init) caps the pools' iteration guards so
    // that it fires -- the error path's own GPU test (tests/test_gpu_state.py)
    uint32_t ring_guard_cap = ~0u;
    int32_t v4_ct_force = 0;   // PT_MI355_V4_CT=1 (read by pt_init): PtV4Job::ct_force (tests)
    uint32_t v4_views_grid = 0;   // PT_MI355_V4_VIEWS_GRID=<blocks> (read by pt_init): PtV4Views::grid_cap (tests: a
                                  // grid of few waves, so that each wave takes tiles of several views)
    uint32_t ct_back_pct = 20;   // PT_MI355_BACK (read by pt_init): PtJob::ct_back_pct (0: none)
    bool back_set = false;       // PT_MI355_BACK given: the occupancy timing keeps it
    uint32_t ct_waves = 0;       // PT_MI355_CT_WAVES (read by pt_init): 5 or 6 waves per SIMD; 0 (default):
                                 // the faster of the two, timed on each geometry's first launches
    // test hook: PT_MI355_CT_WAVES_SEQ (read by pt_init), a string of '5' / '6' cycled over the
    // diffuse continuous-tiles launches -- forced changes of the grid between the launches of one
    // accumulation (tests/test_gpu_configs.py); empty: off
    char ct_seq[64] = {};
    uint32_t ct_seq_len = 0, ct_seq_pos = 0;
    uint32_t split = 1;   // PT_MI355_SPLIT (read by pt_init): tile split factor of the schedule (0: none)
    int64_t test_bad_entry = -1;   // PT_MI355_TEST_BAD_ENTRY (test hook, pt_init)
    bool cam_cache = true;   // PT_MI355_CAM_CACHE=0 (read by pt_init): no camera-hit caches (A/B, tests)
    bool no_ct = false;   // PT_MI355_NO_CT=1 (read by pt_init): one-chunk launches on render_body (A/B)
    uint32_t test_chain_delay = 0;   // PT_MI355_TEST_CHAIN_DELAY=<us> (pt_init): chained launches publish late
    uint32_t unit_mult = 2;          // PT_MI355_UNIT_MULT (pt_init, A/B): the diffuse CT schedule's unit multiple
    unsigned long long sched_rebuild = kSchedRebuildDefault;   // PT_MI355_SCHED_REBUILD (pt_init): launches per schedule build
};

State g;
char g_err[512] = "no error";

int vfail(int code, const char* fmt, va_list ap)
{
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    return code;
}

int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfail(code, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail(PT_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// (kMaxFrame, kMaxDim: pt_v4_batch.h)
#if PT_DIAG
constexpr int kCounterSlots = 32 + 4 * 65536 + 96 * 65536;   // + per-wave records, per-tile log
#else
constexpr int kCounterSlots = 32;
#endif

// The caller's current HIP device is restored when an entry point returns (the library switches to
// each device it drives).
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { (void)hipGetDevice(&prev); }
    ~DeviceGuard()
    {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

int use_dev(const Dev& d)
{
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != d.ordinal) HIP_TRY(hipSetDevice(d.ordinal));
    return PT_OK;
}

int ensure_init()
{
    if (g.inited) return PT_OK;
    return pt_init(nullptr);
}

// ---- shards -----------------------------------------------------------------------------------
// Device d of n owns the global rows d, d + n, ...
int32_t shard_rows(int32_t h, int n, int d) { return d < h ? (h - 1 - d) / n + 1 : 0; }

// Geometry of a host accumulator: size and whether it is tile-major (RenderTile layout).
struct Geo {
    int32_t w = 0, h = 0;
    bool tiled = false;
    int32_t tw = 0, th = 0;
};

// Bytes of device d's mirror: the whole buffer with one device or the tiled layout, else the
// compact rows.
size_t dev_bytes(const Geo& geo, int d)
{
    if (g.ndev == 1 || geo.tiled) return (size_t)geo.w * geo.h * 3 * sizeof(float);
    return (size_t)shard_rows(geo.h, g.ndev, d) * geo.w * 3 * sizeof(float);
}

// A region of the host buffer: the whole frame, or one RenderTile slice (tile index k).
struct Region {
    bool whole = true;
    int32_t tile_x = 0, tile_y = 0;
};

// Copy device d's part of `rg` between the host buffer and its mirror (async on its stream).
int xfer(int d, const Geo& geo, float* host, bool to_device, const Region& rg)
{
    Dev& dv = g.dev[d];
    const hipMemcpyKind kind = to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    const int n = g.ndev;
    if (n == 1) {
        size_t off = 0, len = (size_t)geo.w * geo.h * 3 * sizeof(float);
        if (!rg.whole) {   // simd_tiled.cpp:499-502: the tile is one contiguous slice
            off = ((size_t)rg.tile_y * geo.th * geo.w * 3 + (size_t)rg.tile_x * geo.tw * geo.th * 3) * sizeof(float);
            len = (size_t)geo.tw * geo.th * 3 * sizeof(float);
        }
        char* hp = (char*)host + off;
        char* dp = (char*)dv.dbuf + off;
        HIP_TRY(hipMemcpyAsync(to_device ? (void*)dp : (void*)hp, to_device ? (void*)hp : (void*)dp, len, kind, dv.stream));
        return PT_OK;
    }
    if (!geo.tiled) {   // compact rows: one pitched copy
        const int32_t nr = shard_rows(geo.h, n, d);
        if (nr == 0) return PT_OK;
        const size_t row = (size_t)geo.w * 3 * sizeof(float);
        char* hp = (char*)host + (size_t)d * row;
        if (to_device) HIP_TRY(hipMemcpy2DAsync(dv.dbuf, row, hp, row * n, row, nr, kind, dv.stream));
        else HIP_TRY(hipMemcpy2DAsync(hp, row * n, dv.dbuf, row, row, nr, kind, dv.stream));
        return PT_OK;
    }
    // tiled: every tile is contiguous (TW x TH x 3 floats, raster tile order); the device's rows of a
    // tile are every n-th of its tile rows -- one pitched copy per tile, same offsets on both sides
    const int32_t ntx = geo.w / geo.tw, nty = geo.h / geo.th;
    const size_t tile_f = (size_t)geo.tw * geo.th * 3, trow = (size_t)geo.tw * 3 * sizeof(float);
    const int32_t k0 = rg.whole ? 0 : rg.tile_y * ntx + rg.tile_x, k1 = rg.whole ? ntx * nty : k0 + 1;
    for (int32_t k = k0; k < k1; ++k) {
        const int32_t ty = k / ntx;
        const int32_t ly0 = (int32_t)((((int64_t)d - (int64_t)ty * geo.th) % n + n) % n);
        if (ly0 >= geo.th) continue;
        const int32_t cnt = (geo.th - 1 - ly0) / n + 1;
        const size_t off = (k * tile_f + (size_t)ly0 * geo.tw * 3) * sizeof(float);
        char* hp = (char*)host + off;
        char* dp = (char*)dv.dbuf + off;
        HIP_TRY(hipMemcpy2DAsync(to_device ? (void*)dp : (void*)hp, trow * n, to_device ? (void*)hp : (void*)dp,
                                 trow * n, trow, cnt, kind, dv.stream));
    }
    return PT_OK;
}

// Synchronise every device stream and report what the kernels recorded in their error words since
// the last synchronisation: a tile that a pool's guard abandoned (the ring pool's iteration guard or
// the continuous-tiles pool's chunk / event guards, pt_kernel.hip, pt_v4.hip) leaves a wrong
// accumulator, so no call that waited for such a launch returns PT_OK.  The words are reset when
// reported.  Device jobs on callers' streams are covered once those streams have been synchronised
// (pt_check_device_errors): a launch still running when the words are read and reset may record its
// fault after the reset, and that fault is then reported by the next check.
const char* guard_name(uint32_t id)
{
    switch (id) {
        case PT_G_QUEUE_ENTRY: return "schedule entry outside the launch's tiles";
        case PT_G_NUNITS: return "schedule unit count beyond its entries";
        case PT_G_UNIT_RANGE: return "unit positions outside the schedule";
        case PT_G_SLOT_BASE: return "wave slot area beyond the allocation";
        case PT_G_ITEM_SLOT: return "item radiance slot outside its wave's area";
        case PT_G_PIXEL: return "accumulator element outside the buffer";
        case PT_G_PIXOUT: return "presented pixel outside the pixel buffer";
        case PT_G_ENVQ: return "env miss-queue entry outside the queue";
        case PT_G_SCHED_ORDER: return "schedule builder: order position out of range";
        case PT_G_SCHED_UNIT: return "schedule builder: unit index out of range";
        case PT_G_RECORD: return "item record slot >= 64";
        case PT_G_QUEUE_GROUP: return "queue group out of range";
        case PT_G_VIEW: return "views launch: view index beyond the view table";
        case PT_G_SCENE: return "scenes launch: scene index beyond the scene table, or a record's object counts beyond MAX_OBJECTS";
        case PT_G_ENV: return "envs launch: env index beyond the env set, or a record's width or height not positive";
        case PT_G_FRAMES: return "batch launch: a view's frame range record is invalid; value: the view";
        case PT_G_STATS: return "batch launch with statistics: a view's record beyond the statistics buffer; value: the view";
        case PT_G_CAM_INDEX: return "camera-hit cache record outside the geometry's tiles";
        case PT_G_CAM_RECORD: return "a traced camera hit differs from its cached record; value: tile * 64 + lane";
        case PT_G_CHAIN_WAIT: return "chained launch: the previous launch's tile never became ready; value: the tile | its epoch's lag "
                                     "<< 24 | bit 31 when an atomic read also lags (pt_chain.h)";
        default: return "unknown";
    }
}

int sync_all()
{
    int rc;
    for (int d = 0; d < g.ndev; ++d) {
        Dev& dv = g.dev[d];
        if ((rc = use_dev(dv))) return rc;
        HIP_TRY(hipMemcpyAsync(dv.herr, dv.derr, PT_ERR_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, dv.stream));
    }
    for (int d = 0; d < g.ndev; ++d) {
        if ((rc = use_dev(g.dev[d]))) return rc;
        HIP_TRY(hipStreamSynchronize(g.dev[d].stream));
    }
    for (int d = 0; d < g.ndev; ++d) {
        Dev& dv = g.dev[d];
        const uint32_t guards = dv.herr[PT_ERR_GUARD_COUNT];
        if (dv.herr[0] == 0 && guards == 0) continue;
        const uint32_t n = dv.herr[0], tile = dv.herr[1];
        const unsigned long long first =
            (unsigned long long)dv.herr[PT_ERR_GUARD_FIRST] | ((unsigned long long)dv.herr[PT_ERR_GUARD_FIRST + 1] << 32);
        if ((rc = use_dev(dv))) return rc;
        const uint32_t init[PT_ERR_WORDS] = {0u, ~0u, 0u, 0u, ~0u, ~0u};
        memcpy(dv.herr, init, sizeof(init));
        HIP_TRY(hipMemcpyAsync(dv.derr, dv.herr, sizeof(init), hipMemcpyHostToDevice, dv.stream));
        HIP_TRY(hipStreamSynchronize(dv.stream));
        if (guards && (uint32_t)(first >> 32) == PT_G_CHAIN_WAIT) dv.chain.off = true;
        for (Sched& sc : dv.sched) sc.cam_state = kCamEmpty;   // (a faulted fill launch leaves records unwritten: fill again)
        if (guards)
            return fail(PT_EKERNEL, "device %d: %u kernel bounds guard failure(s), the first: guard %u (%s), value %u; "
                        "pool guards: %u (first tile %u); the accumulator is invalid", dv.ordinal, guards,
                        (uint32_t)(first >> 32), guard_name((uint32_t)(first >> 32)), (uint32_t)first, n, n ? tile : 0u);
        return fail(PT_EKERNEL, "device %d: a pool guard (ring iterations or continuous-tiles chunks) abandoned %u "
                    "tile(s) (first: tile %u of its launch); the accumulator is invalid", dv.ordinal, n, tile);
    }
    return PT_OK;
}

int ensure_dbuf(int d, size_t bytes)
{
    Dev& dv = g.dev[d];
    if (bytes <= dv.dbuf_cap) return PT_OK;
    if (dv.dbuf) {
        HIP_TRY(hipStreamSynchronize(dv.stream));
        HIP_TRY(hipFree(dv.dbuf));
        dv.dbuf = nullptr;
        dv.dbuf_cap = 0;
    }
    if (hipMalloc(&dv.dbuf, bytes) != hipSuccess) {
        dv.dbuf = nullptr;
        return fail(PT_ENOMEM, "hipMalloc(%zu) failed on device %d", bytes, dv.ordinal);
    }
    dv.dbuf_cap = bytes;
    g.m.valid = false;
    return PT_OK;
}

Geo mirror_geo()
{
    Geo geo;
    geo.w = g.m.width;
    geo.h = g.m.height;
    geo.tiled = g.m.tiled;
    geo.tw = g.m.tile_w;
    geo.th = g.m.tile_h;
    return geo;
}

// Deferred mode: a valid mirror is the only up-to-date copy of its host buffer's accumulation.
// Before the mirror is given to another buffer it is written back to its own host buffer (as if
// pt_readback had been called), so alternating buffers loses nothing.  The caller must release a
// deferred buffer (pt_release_buffer) before freeing it.
int flush_mirror()
{
    int rc;
    if (!g.m.valid || !g.m.host) {
        g.m.valid = false;
        return PT_OK;
    }
    const Geo geo = mirror_geo();
    for (int d = 0; d < g.ndev; ++d) {
        if ((rc = use_dev(g.dev[d])) || (rc = xfer(d, geo, (float*)g.m.host, false, Region{}))) return rc;
    }
    if ((rc = sync_all())) return rc;
    g.m.valid = false;
    return PT_OK;
}

void drop_mirror()
{
    g.m = Mirror{};
}

bool same_split(const Geo& geo)
{
    if (g.m.width != geo.w || g.m.height != geo.h) return false;
    if (g.ndev == 1) return true;   // one device mirrors the whole buffer in any layout
    return g.m.tiled == geo.tiled && (!geo.tiled || (g.m.tile_w == geo.tw && g.m.tile_h == geo.th));
}

// Make the device mirrors hold region `rg` of the host buffer `host` (geometry `geo`).  In
// deferred mode an already valid mirror of the same buffer is authoritative and nothing is copied.
int stage_in(float* host, const Geo& geo, const Region& rg)
{
    const bool deferred = (g.cfg.flags & PT_FLAG_DEFER_READBACK) != 0;
    const size_t bytes = (size_t)geo.w * geo.h * 3 * sizeof(float);
    int rc;
    if (g.m.valid) {
        if (g.m.host == host && g.m.bytes != bytes) drop_mirror();   // reallocated in place: never write back
        else if (g.m.host != host || !same_split(geo))
            if ((rc = flush_mirror())) return rc;
    }
    for (int d = 0; d < g.ndev; ++d)
        if ((rc = use_dev(g.dev[d])) || (rc = ensure_dbuf(d, dev_bytes(geo, d)))) return rc;
    if (deferred && g.m.valid) return PT_OK;
    const Region r = deferred ? Region{} : rg;   // first deferred touch: the whole buffer becomes device-resident
    for (int d = 0; d < g.ndev; ++d)
        if ((rc = use_dev(g.dev[d])) || (rc = xfer(d, geo, host, true, r))) return rc;
    g.m.host = host;
    g.m.bytes = bytes;
    g.m.width = geo.w;
    g.m.height = geo.h;
    g.m.tiled = geo.tiled;
    g.m.tile_w = geo.tw;
    g.m.tile_h = geo.th;
    g.m.valid = deferred;
    return PT_OK;
}

int stage_out(float* host, const Geo& geo, const Region& rg)
{
    int rc;
    if (!(g.cfg.flags & PT_FLAG_DEFER_READBACK))
        for (int d = 0; d < g.ndev; ++d)
            if ((rc = use_dev(g.dev[d])) || (rc = xfer(d, geo, host, false, rg))) return rc;
    return sync_all();
}

int check_frame_budget(uint32_t add)
{
    if ((uint64_t)g.frame + add >= kMaxFrame)
        return fail(PT_EINVAL, "frame counter %u + %u exceeds the exact f32 range 2^24", g.frame, add);
    return PT_OK;
}

PtJob base_job(float* buf, int32_t w, int32_t h)
{
    PtJob j{};
    j.buf = buf;
    j.width = w;
    j.height = h;
    j.col0 = 0;
    j.ncols = w;
    j.row_start = 0;
    j.row_stride = 1;
    j.nrows = h;
    j.layout = PT_LAYOUT_INTERLEAVED;
    j.tile_w = j.tile_h = 0;
    j.frame_first = g.frame + 1;
    j.nframes = g.cfg.samples_per_frame;
    j.num_bounces = g.cfg.num_bounces;
    j.guard_cap = g.ring_guard_cap;
    return j;   // (every other field null or zero: the caller, launch_with, prepare and launch_chain set them)
}

void free_sched(Sched& s)
{
    if (s.cost) (void)hipFree(s.cost);
    if (s.order) (void)hipFree(s.order);
    if (s.units) (void)hipFree(s.units);
    if (s.epoch) (void)hipFree(s.epoch);
    if (s.cam) (void)hipFree(s.cam);
    for (hipEvent_t e : s.tune_ev)
        if (e) (void)hipEventDestroy(e);
    s = Sched{};
}

// A schedule's key: the nine members the renderers share, and what differs -- the kind, the tile count
// and the split factor.  v4 takes whole tiles: its per-tile kernel runs launches of < 8 frames (and
// PT_MI355_NO_CT=1), and split tiles measured slower on the continuous-tiles one (0.3666 vs 0.3633 ms at
// 1080p 8 spp).
template <typename Job>
SchedKey sched_key(const Job& j, int32_t kind, uint32_t ntiles, uint32_t split)   // (in SchedKey's member order)
{
    return {kind, j.width, j.height, j.col0, j.ncols, j.row_start, j.row_stride, j.nrows, j.num_bounces, j.env, ntiles, split};
}
SchedKey sched_key(const PtJob& j) { return sched_key(j, 0, pt_job_tiles(j), pt_plan_split(j.nframes, g.split)); }
SchedKey sched_key(const PtV4Job& j)
{
    return sched_key(j, 1 + j.env_mode, (uint32_t)((j.ncols + 7) / 8) * (uint32_t)((j.nrows + 7) / 8), 0u);
}

bool cam_launch_qualifies(const Sched& s, int32_t nframes)
{
    return pt_cam_launch_qualifies(s.cam_off, nframes, pt_cam_cache_wanted(g.cam_cache, s.key.kind, s.key.ntiles));
}

// The camera-hit cache fields of a launch of `s`'s geometry on `st` that is stream-ordered after the
// geometry's earlier launches -- or a continuing chained one, which neither fills nor settles a cache
// (pt_cam_chain_may_continue).  A counted launch never fills: it traces the camera rays for its counters,
// and compares them with a valid cache.
void cam_cache_job(Sched* s, PtJob& j, bool count, hipStream_t st)
{
    j.cam_cache = nullptr;
    j.cam_mode = PT_CAM_NONE;
    if (!s || !j.ct_slots || !cam_launch_qualifies(*s, j.nframes)) return;
    if (s->cam_state == kCamFilled) s->cam_state = kCamSettled;
    if (s->cam_state == kCamEmpty && count) return;
    if (!s->cam) {
        // every record a miss until the fill launch stores it (a tile that a faulted fill launch
        // abandoned then reads as sky, never as an arbitrary primitive)
        const size_t bytes = pt_cam_cache_bytes(s->key.ntiles);
        if (hipMalloc(&s->cam, bytes) != hipSuccess || hipMemsetAsync(s->cam, 0xff, bytes, st) != hipSuccess) {
            (void)hipGetLastError();
            if (s->cam) (void)hipFree(s->cam);
            s->cam = nullptr;
            s->cam_off = true;   // launches without a cache: correct, only slower
            return;
        }
    }
    j.cam_cache = s->cam;
    j.cam_mode = s->cam_state == kCamEmpty ? PT_CAM_FILL : PT_CAM_USE;
}

Sched* find_sched(Dev& dv, const SchedKey& key, hipStream_t st)
{
    const uint32_t n = key.ntiles;
    if (n < kSchedMinTiles) return nullptr;
    Sched* lru = &dv.sched[0];
    for (Sched& s : dv.sched) {
        if (s.used && s.stream == st && s.key == key) {
            s.last_use = ++dv.sched_clock;
            return &s;
        }
        if (!s.used || (lru->used && s.last_use < lru->last_use)) lru = &s;
    }
    if (lru->used) {   // evict: its buffers may still be read by a launch (its stream may be gone)
        (void)hipDeviceSynchronize();
        if (dv.chain.sched == lru) dv.chain.sched = nullptr;   // (its chain ends: the next chained launch restarts)
        free_sched(*lru);
    }
    Sched s;
    if (hipMalloc(&s.cost, 2 * (size_t)n * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&s.order, 2 * (size_t)n * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&s.units, (2 * (size_t)n + 2) * sizeof(uint32_t)) != hipSuccess) {
        free_sched(s);
        return nullptr;   // unscheduled launch (raster order): correct, only slower
    }
    s.used = true;
    s.stream = st;
    s.key = key;
    s.last_use = ++dv.sched_clock;
    *lru = s;
    return lru;
}

int slot_event(Dev& dv, unsigned slot)
{
    if (!dv.queue_event[slot]) HIP_TRY(hipEventCreateWithFlags(&dv.queue_event[slot], hipEventDisableTiming));
    return PT_OK;
}

// The event ordering the last use of ring slot `slot` (nullptr: never used).
hipEvent_t slot_order(const Dev& dv, unsigned slot)
{
    const int a = dv.queue_alias[slot];
    return a >= 0 ? dv.queue_event[a] : dv.queue_event[slot];
}

// The schedule and queue fields of a launch of geometry `key` on stream `st`.
struct LaunchSched {
    unsigned slot = 0;   // tile-queue ring slot (queue_done after the launch)
    unsigned int* queue = nullptr;
    unsigned int* queue_next = nullptr;   // the next ring slot, zeroed by this launch's kernel
    const uint32_t* order = nullptr;
    const uint32_t* units = nullptr;
    const uint32_t* nunits = nullptr;
    uint32_t* cost = nullptr;
    Sched* sched = nullptr;   // with a built schedule
    Sched* geo = nullptr;     // the geometry's Sched, built or not
    void use(Sched& s) { sched = &s, order = s.order, units = s.units, nunits = s.nunits(); }   // (s is built)
};
// Order `st` after every chained launch of the device and end the live chain (launch_chain): a
// launch that is not a continuing chained one may use what the chained launches use -- the slot
// areas, the geometry's schedule, the accumulator.
int chain_join(Dev& dv, hipStream_t st)
{
    for (int i = 0; i < 2; ++i) {
        if (!dv.chain.pending[i]) continue;
        if (hipEventQuery(dv.chain.done[i]) == hipSuccess) {
            dv.chain.pending[i] = false;
        } else {
            (void)hipGetLastError();   // (hipErrorNotReady)
            HIP_TRY(hipStreamWaitEvent(st, dv.chain.done[i], 0));
        }
    }
    dv.chain.sched = nullptr;
    return PT_OK;
}

int use_queue_slot(Dev& dv, hipStream_t st, LaunchSched* ls);

// key.split: the schedule builder's tile split factor (pt_launch_schedule; 0: whole tiles).  *sched_st:
// the stream that identifies the geometry's schedule (launch_chain: the caller's stream, which may be
// the null stream; nullptr: st).
int use_sched(Dev& dv, const SchedKey& key, hipStream_t st, LaunchSched* ls, const hipStream_t* sched_st = nullptr)
{
    *ls = LaunchSched{};
    int rc;
    if ((rc = chain_join(dv, st))) return rc;
    if (Sched* s = find_sched(dv, key, sched_st ? *sched_st : st)) {
        ls->geo = s;
        const PtSchedStep step = pt_plan_sched_step(s->have_cost, s->built, s->launches, g.sched_rebuild);
        if (step.builds) {
            // units of twice the adaptive cost for the diffuse kernels' continuous-tiles pool, whose
            // lanes no longer idle in a unit's tail while the dequeues still cost (A/B, 60 launches:
            // 1080p 8 spp 0.2497 vs 0.2525 ms, env 16 spp 0.4911 vs 0.4961, 4K 8 spp 0.8185 vs 0.8202;
            // 3x: 0.2513 / 0.4965 / 0.8356)
            const uint32_t unit_mult = key.kind == 0 && !g.no_ct ? g.unit_mult : 1u;
            hipError_t e = pt_launch_schedule(s->cost, s->order, s->units, s->nunits(), s->key.ntiles, key.split, unit_mult,
                                              st, dv.derr);
            if (e != hipSuccess) return fail(PT_EHIP, "schedule launch failed: %s", hipGetErrorString(e));
            s->built = true;
            if (g.test_bad_entry >= 0 && (uint32_t)g.test_bad_entry < 2u * s->key.ntiles)   // (test hook, below)
                HIP_TRY(hipMemsetAsync(s->order + g.test_bad_entry, 0xff, sizeof(uint32_t), st));
        }
        if (s->built) ls->use(*s);
        if (step.records) {
            ls->cost = s->cost;
            s->have_cost = true;
        }
        ++s->launches;
    }
    return use_queue_slot(dv, st, ls);
}

// The tile-queue fields of a launch on `st` (use_sched's second half; a views launch, which has no
// schedule, takes only these).
int use_queue_slot(Dev& dv, hipStream_t st, LaunchSched* ls)
{
    // Ring slots are used in order.  Each render kernel zeroes the NEXT slot's counters at its start,
    // so a launch after a launched kernel on the same stream finds its slot zero.  After a launch on
    // another stream that slot may still be being zeroed: it is skipped (its next user waits for that
    // kernel) and this launch zeroes the slot after it with a memset on its own stream, so launches on
    // different streams overlap.  A slot whose previous user ran on another stream is waited for
    // before it is zeroed or used.
    // Nothing is ever enqueued on a stream other than `st` (a previous launch's stream may be a
    // caller's stream that has been destroyed since): the skipped slot takes the previous slot's
    // event, recorded by queue_done right after the launch whose kernel zeroes it.
    unsigned slot = dv.queue_next++ % kQueueRing;
    bool pre = dv.queue_pre_zeroed;
    if (pre && dv.last_stream != st) {
        const unsigned prev = (slot + kQueueRing - 1) % kQueueRing;
        dv.queue_alias[slot] = (int16_t)prev;
        dv.queue_stream[slot] = dv.queue_stream[prev];
        slot = dv.queue_next++ % kQueueRing;
        pre = false;
    }
    ls->slot = slot;
    if (hipEvent_t ev = slot_order(dv, slot); ev && dv.queue_stream[slot] != st) HIP_TRY(hipStreamWaitEvent(st, ev, 0));
    ls->queue = dv.dqueue + (size_t)slot * PT_QUEUE_WORDS;
    if (!pre) HIP_TRY(hipMemsetAsync(ls->queue, 0, PT_QUEUE_WORDS * sizeof(unsigned), st));
    dv.queue_pre_zeroed = false;   // (set by queue_done once this launch's kernel is enqueued)
    const unsigned next = (slot + 1) % kQueueRing;
    if (hipEvent_t ev = slot_order(dv, next); ev && dv.queue_stream[next] != st) HIP_TRY(hipStreamWaitEvent(st, ev, 0));
    ls->queue_next = dv.dqueue + (size_t)next * PT_QUEUE_WORDS;
    return PT_OK;
}

// After the launch that used ring slot `slot` was enqueued on `st`; `zeroed_next`: its kernel ran
// (a launch with nothing to render returns without one) and zeroes the next slot.
int queue_done(Dev& dv, unsigned slot, hipStream_t st, bool zeroed_next)
{
    int rc;
    if ((rc = slot_event(dv, slot))) return rc;
    HIP_TRY(hipEventRecord(dv.queue_event[slot], st));
    dv.queue_stream[slot] = st;
    dv.queue_alias[slot] = -1;
    dv.queue_pre_zeroed = zeroed_next;
    dv.last_stream = st;
    return PT_OK;
}

// The continuous-tiles pools' slot area (pt_kernel.hip render_body_ct, pt_v4.hip pt_v4_ct_kernel) for
// a launch in ring slot ls.slot on `st`: nullptr (the per-tile pool kernels) with PT_MI355_NO_CT=1.
// The device's slot area (Dev::dct), allocated on first use: 12 KiB per wave of the resident grid
// (~75 MB).  Left null when the allocation fails (the per-tile pools then: correct, slower).
void ct_area_alloc(Dev& dv)
{
    if (dv.dct) return;
    const uint32_t w = pt_ct_resident_waves();
    if (hipMalloc(&dv.dct, (size_t)w * pt_ct_wave_floats() * sizeof(float)) == hipSuccess) dv.dct_waves = w;
    else dv.dct = nullptr, (void)hipGetLastError();
}

int use_ct_slots(Dev& dv, const LaunchSched& ls, hipStream_t st, float** slots, uint32_t* waves)
{
    *slots = nullptr;
    *waves = 0;
    if (g.no_ct) return PT_OK;
    ct_area_alloc(dv);
    *slots = dv.dct;
    *waves = dv.dct_waves;
    if (dv.dct) {   // launches on several streams share the slots: one after the other
        if (dv.ct_slot >= 0 && dv.queue_stream[dv.ct_slot] != st)
            if (hipEvent_t ev = slot_order(dv, (unsigned)dv.ct_slot)) HIP_TRY(hipStreamWaitEvent(st, ev, 0));
        dv.ct_slot = (int)ls.slot;
    }
    return PT_OK;
}

// The launch variant of a continuous-tiles launch (PtJob::ct_wide, ct_back_pct; the arms and why:
// pt_launch_plan.h): here, the events and the state.  *tev: the pair to record around a timed launch.
int ct_occupancy(const LaunchSched& ls, PtJob& j, hipEvent_t** tev, bool count)
{
    *tev = nullptr;
    j.ct_wide = g.ct_waves == 6 ? 1u : 0u;
    if (g.ct_seq_len && j.ct_slots && !j.env) {   // (test hook: the forced sequence)
        j.ct_wide = g.ct_seq[g.ct_seq_pos++ % g.ct_seq_len] == '6' ? 1u : 0u;
        return PT_OK;
    }
    Sched* s = ls.sched;
    const bool env = j.env != nullptr;
    if (g.ct_waves || !j.ct_slots || !s || (env && !pt_plan_env_arms(env, j.ct_back_pct, g.back_set))) return PT_OK;
    const auto apply = [&](int arm) {
        const PtVariant v = pt_plan_variant(env, arm, j.ct_back_pct, g.back_set);
        j.ct_wide = v.wide;
        j.ct_back_pct = v.back_pct;
    };
    // only uncounted launches of the first timed launch's length are timed: a counted launch (the
    // bench's work-count pass) or one of another length sharing the geometry's schedule would bias the
    // arms' sums; they run the interim choice below.  The first timed launch fixes the
    // arms (and the length).
    const bool timeable = !count && (s->tune_nframes == 0 || s->tune_nframes == j.nframes);
    if (!s->narms && timeable) s->narms = pt_plan_narms(env, j.ct_back_pct, g.back_set);
    const uint32_t per_round = pt_plan_round_launches(s->narms), nt = pt_plan_tune_launches(s->narms);
    const auto arm_of = [&](uint32_t t) { return pt_plan_arm_of(s->narms, t); };
    if (s->wide >= 0) {
        apply(s->wide);
    } else if (s->tuned < nt && timeable) {
        s->tune_nframes = j.nframes;
        hipEvent_t* ev = &s->tune_ev[2 * s->tuned];
        for (int i = 0; i < 2; ++i)
            if (!ev[i]) HIP_TRY(hipEventCreate(&ev[i]));
        apply(arm_of(s->tuned++));
        *tev = ev;
    } else if (nt && s->tuned >= nt && hipEventQuery(s->tune_ev[2 * nt - 1]) == hipSuccess) {
        float t[3] = {0.f, 0.f, 0.f};
        for (uint32_t i = per_round; i < nt; ++i) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, s->tune_ev[2 * i], s->tune_ev[2 * i + 1]));
            t[arm_of(i)] += ms;
        }
        int best = 0;
        for (int a = 1; a < (int)s->narms; ++a)
            if (t[a] < t[best]) best = a;
        s->wide = (int8_t)best;
        apply(best);
    } else {
        (void)hipGetLastError();   // (hipErrorNotReady: the timed launches are still running)
        apply(pt_plan_interim_arm(env, j.nframes));
    }
    return PT_OK;
}

// What differs between the renderers in a launch, besides the schedule's key: what the device, the
// configuration and the launch variant set in the job (prepare), and the kernel entry point (enqueue).
// The diffuse kernels time their arms on a geometry's first launches and cache camera hits; v4 has one
// variant and no cache.  cont: a continuing chained launch (launch_chain), which takes the chained share.
int prepare(const Dev& dv, const LaunchSched& ls, PtJob& j, hipStream_t st, bool count, bool cont, hipEvent_t** tev)
{
    int rc;
    j.scene = dv.dscene;
    j.ct_back_pct = pt_plan_back(j.nframes, g.ct_back_pct);
    if ((rc = ct_occupancy(ls, j, tev, count))) return rc;
    if (cont) j.ct_back_pct = pt_plan_chain_back(j.env != nullptr, j.ct_back_pct, g.back_set);
    cam_cache_job(ls.geo, j, count, st);
    return PT_OK;
}
int prepare(const Dev& dv, const LaunchSched&, PtV4Job& j, hipStream_t, bool, bool cont, hipEvent_t**)
{
    if (j.env_mode != PT_V4_ENV_NONE) j.env = dv.denv;
    j.ct_force = g.v4_ct_force;
    j.ct_back_pct = cont ? pt_plan_chain_back_v4(j.nframes, g.ct_back_pct, g.back_set) : pt_plan_back(j.nframes, g.ct_back_pct);
    return PT_OK;
}
int enqueue(const LaunchSched& ls, const PtJob& j, hipStream_t st, bool count, bool*, uint32_t* n)
{
    hipError_t e = pt_launch_render(j, st, count, n);
    if (e != hipSuccess) return fail(PT_EHIP, "render launch failed: %s", hipGetErrorString(e));
    if (j.cam_mode == PT_CAM_FILL && *n) ls.geo->cam_state = kCamFilled;   // (a continuous-tiles kernel ran)
    return PT_OK;
}
int enqueue(const LaunchSched&, const PtV4Job& j, hipStream_t st, bool count, bool* presented, uint32_t* n)
{
    hipError_t e = pt_launch_v4(j, g.v4scene, st, count, presented, n);
    return e == hipSuccess ? PT_OK : fail(PT_EHIP, "v4 render launch failed: %s", hipGetErrorString(e));
}

// What plain and continuing chained launches share: the job `j`, whose slot area is set, takes the
// schedule and queue fields of `ls` (PtJob and PtV4Job name them alike) and is enqueued on `st`, between
// ct_occupancy's event pair if it is timed.  *blocks: the continuous-tiles grid launched (0: none).
template <typename Job>
int launch_with(Dev& dv, Job& j, const LaunchSched& ls, hipStream_t st, bool count, bool cont, bool* presented, uint32_t* blocks)
{
    int rc;
    j.queue = ls.queue;
    j.queue_next = ls.queue_next;
    j.order = ls.order;
    j.units = ls.units;
    j.nunits = ls.nunits;
    j.cost = ls.cost;
    j.err = dv.derr;
    hipEvent_t* tev = nullptr;
    if ((rc = prepare(dv, ls, j, st, count, cont, &tev))) return rc;
    if (tev) HIP_TRY(hipEventRecord(tev[0], st));
    if ((rc = enqueue(ls, j, st, count, presented, blocks))) return rc;
    if (tev) HIP_TRY(hipEventRecord(tev[1], st));
    return PT_OK;
}

// A plain launch of either renderer.  *ct_blocks: as launch_with's; sched_st: see use_sched; *presented: pt_launch_v4's
// (all optional; the v4 pool's slots per wave: pt_v4_ct_wave_floats() <= pt_ct_wave_floats(), pt_v4.hip)
template <typename Job>
int launch(Dev& dv, Job j, hipStream_t st, bool count, uint32_t* ct_blocks = nullptr, const hipStream_t* sched_st = nullptr,
           bool* presented = nullptr)
{
    LaunchSched ls;
    int rc;
    uint32_t blocks = 0;
    if ((rc = use_dev(dv)) || (rc = use_sched(dv, sched_key(j), st, &ls, sched_st)) ||
        (rc = use_ct_slots(dv, ls, st, &j.ct_slots, &j.ct_waves)) ||
        (rc = launch_with(dv, j, ls, st, count, false, presented, &blocks)))
        return rc;
    if (ct_blocks) *ct_blocks = blocks;
    return queue_done(dv, ls.slot, st, j.ncols > 0 && j.nrows > 0 && j.nframes > 0);   // (the entry point's early return)
}

// Chained launches (pt_render_device_chain).  A progressive renderer launches the same geometry again
// and again; back to back on one stream, each launch's end leaves the chip partly idle (c2: the queue
// runs dry ~170 us into a ~234 us launch and the last waves finish their chunks while the others have
// exited).  Consecutive chained launches alternate between two streams, so the next
// launch's blocks take the CUs the finishing waves free.  Each pixel's frames still fold in order:
// the kernel touches a tile's pixels only after the previous launch has stored them (the tile epochs,
// render_body_ct), and nothing else passes between the two launches -- each has its own tile-queue
// block, slot area and started counter, and the schedule they share is read-only while they overlap.
// Deadlock freedom: a launch waits only for its predecessor's tiles, and its stream starts it only
// after every block of the predecessor has started (hipStreamWaitValue64 on the chain's started
// counter), so the oldest running launch never waits and all of its waves are resident: it completes,
// then the next oldest, and so on (the kernel's bounded wait is a report, not a mechanism).
// A chained launch RESTARTS the chain -- its stream waits for the caller's stream and every chained
// launch before it, as a plain launch would -- when another launch came between (any launch on the
// device ends the live chain: chain_join), on the geometry's first launches (schedule not built, launch
// variant being timed), when it builds the schedule or records the costs it is built from, or when it
// is not a continuous-tiles launch.  Otherwise it CONTINUES: it does not wait for the caller's stream
// (the caller promises that nothing enqueued there since its previous chained call is needed by this
// one, include/pt_mi355.h) -- only for its predecessor's blocks to have started.  Every chained launch
// is joined back into the caller's stream (it waits for the launch's event), so work the caller
// enqueues afterwards sees it complete.
int chain_setup(Dev& dv, Sched& sc)
{
    Dev::Chain& c = dv.chain;
    for (int i = 0; i < 2; ++i) {
        if (!c.st[i]) HIP_TRY(hipStreamCreateWithFlags(&c.st[i], hipStreamNonBlocking));
        if (!c.done[i]) HIP_TRY(hipEventCreateWithFlags(&c.done[i], hipEventDisableTiming));
    }
    if (!c.ev_caller) HIP_TRY(hipEventCreateWithFlags(&c.ev_caller, hipEventDisableTiming));
    if (!c.qblk && hipMalloc(&c.qblk, 4 * PT_QUEUE_WORDS * sizeof(unsigned)) != hipSuccess)
        return fail(PT_ENOMEM, "hipMalloc(chain queue blocks) failed");
    if (!c.started) {   // (never reset: a gate evaluated early must not see a count from before a restart)
        if (hipMalloc(&c.started, sizeof(unsigned long long)) != hipSuccess)
            return fail(PT_ENOMEM, "hipMalloc(chain counter) failed");
        HIP_TRY(hipMemset(c.started, 0, sizeof(unsigned long long)));
        c.cum = 0;
    }
    if (!c.area1 && dv.dct &&
        hipMalloc(&c.area1, (size_t)dv.dct_waves * pt_ct_wave_floats() * sizeof(float)) != hipSuccess)
        return fail(PT_ENOMEM, "hipMalloc(second slot area) failed");
    if (!sc.epoch) {
        if (hipMalloc(&sc.epoch, 2 * (size_t)sc.key.ntiles * sizeof(uint32_t)) != hipSuccess)
            return fail(PT_ENOMEM, "hipMalloc(tile epochs) failed");
        HIP_TRY(hipMemset(sc.epoch, 0, 2 * (size_t)sc.key.ntiles * sizeof(uint32_t)));
        sc.chain_seq = 0;
    }
    return PT_OK;
}

// Whether the launch variant no longer depends on timing (the diffuse kernels time their arms on a
// geometry's first launches; v4 has one variant).
bool chain_variant_fixed(const PtJob& j, const Sched& sc)
{
    const bool env = j.env != nullptr;   // (without arms: ct_occupancy leaves it the fixed variant)
    return g.ct_waves || g.ct_seq_len || sc.wide >= 0 ||
           (env && !pt_plan_env_arms(env, pt_plan_back(j.nframes, g.ct_back_pct), g.back_set));
}
bool chain_variant_fixed(const PtV4Job&, const Sched&) { return true; }

template <typename Job>
int launch_chain(Dev& dv, Job j, hipStream_t s)
{
    int rc;
    if ((rc = use_dev(dv))) return rc;
    Dev::Chain& c = dv.chain;
    // (the continuous-tiles pool and a scheduled geometry: the tile epochs live in its schedule)
    Sched* sc = c.off || g.no_ct || j.ncols <= 0 || j.nrows <= 0 || j.nframes <= 0 ? nullptr : find_sched(dv, sched_key(j), s);
    if (sc) {
        ct_area_alloc(dv);
        if ((rc = chain_setup(dv, *sc))) return rc;
    }
    if (!sc || !dv.dct || !c.area1) return launch(dv, j, s, false);   // (a plain launch: use_sched joins the chain)
    // what the plain launch's use_sched does for this launch: build the schedule (restart), record the
    // costs it is built from (a launch that records them may continue: the overlapped launches before
    // it do not write them, and the next launch, which builds from them, restarts)
    const PtSchedStep step = pt_plan_sched_step(sc->have_cost, sc->built, sc->launches, g.sched_rebuild);
    // (the camera-hit cache: the launch that fills it and the one after it restart -- no launch reads
    // records while another may still be writing them)
    const bool cont = pt_plan_chain_continues(
        c.sched == sc, sc->built, step.builds, chain_variant_fixed(j, *sc),
        pt_cam_chain_may_continue(cam_launch_qualifies(*sc, j.nframes), sc->cam != nullptr, sc->cam_state));
    const uint32_t seq = sc->chain_seq + 1;
    const int par = cont ? c.par ^ 1 : 0;
    hipStream_t X = c.st[par];
    j.tile_epoch = sc->epoch;
    j.chain_seq = seq;
    j.started = c.started;
    j.chain_delay = g.test_chain_delay;
    uint32_t blocks = 0;
    if (!cont) {
        // restart: after the caller's stream and every chained launch (the plain launch's use_sched joins them)
        HIP_TRY(hipEventRecord(c.ev_caller, s));
        HIP_TRY(hipStreamWaitEvent(X, c.ev_caller, 0));
        if ((rc = chain_join(dv, X))) return rc;
        HIP_TRY(hipMemsetAsync(c.qblk, 0, 4 * PT_QUEUE_WORDS * sizeof(unsigned), X));
        j.chain_wait = 0;
        if ((rc = launch(dv, j, X, false, &blocks, &s))) return rc;   // (slot area dct)
        c.area = 0;
    } else {
        // continue: once every block of the previous launch has started
        HIP_TRY(hipStreamWaitValue64(X, c.started, c.cum, hipStreamWaitValueGte, ~0ull));
        j.chain_wait = seq - 1;
        LaunchSched ls;
        ls.geo = sc;
        ls.use(*sc);
        ls.queue = c.qblk + (size_t)(seq % 4u) * PT_QUEUE_WORDS;
        ls.queue_next = c.qblk + (size_t)((seq + 2u) % 4u) * PT_QUEUE_WORDS;   // (the launch after next: this stream's)
        ls.cost = step.records ? sc->cost : nullptr;
        const int area = c.area ^ 1;
        j.ct_slots = area ? c.area1 : dv.dct;
        j.ct_waves = dv.dct_waves;
        if ((rc = launch_with(dv, j, ls, X, false, true, nullptr, &blocks))) return rc;
        // (committed once the kernel is enqueued: a failed launch leaves the chain as its predecessor
        // left it, and the next one does not take the slot area of a launch that may still be running)
        c.area = area;
        if (step.records) sc->have_cost = true;
        ++sc->launches;
    }
    c.cum += blocks;
    sc->chain_seq = seq;
    ++(cont ? c.continued : c.restarts);
    HIP_TRY(hipEventRecord(c.done[par], X));
    c.pending[par] = true;
    HIP_TRY(hipStreamWaitEvent(s, c.done[par], 0));
    // a launch that did not run a continuous-tiles pool published no epochs and counted no blocks:
    // the next chained launch restarts
    c.sched = blocks ? sc : nullptr;
    c.par = par;
    return PT_OK;
}

void unpin()
{
    if (g.pinned) {
        (void)hipDeviceSynchronize();
        (void)hipHostUnregister((void*)g.pinned);
    }
    g.pinned = nullptr;
    g.pinned_bytes = 0;
}

bool pin(const float* p, size_t bytes)
{
    if (g.pinned == p && g.pinned_bytes == bytes) return true;
    unpin();
    if (hipHostRegister((void*)p, bytes, hipHostRegisterDefault) != hipSuccess) {
        (void)hipGetLastError();
        return false;   // e.g. already page-locked by the caller: unpipelined path
    }
    g.pinned = p;
    g.pinned_bytes = bytes;
    return true;
}

// PT_FLAG_PIN_HOST (one device, without deferred readback) and `buf` page-locked: the frame job `j`
// (whole image, either renderer) is split into kBands row bands (multiples of row_align rows:
// contiguous in every layout) whose upload, render (`run(band_job)` on the device stream) and
// download overlap on three streams.  Returns with the downloads queued on g.s_out; *used = false if
// the path does not apply.
template <typename Job, typename Run>
int render_bands(float* buf, const Job& j, int32_t row_align, Run&& run, bool* used)
{
    int rc;
    const size_t bytes = (size_t)j.width * j.height * 3 * sizeof(float);
    *used = false;
    if (g.ndev != 1 || !(g.cfg.flags & PT_FLAG_PIN_HOST) || (g.cfg.flags & PT_FLAG_DEFER_READBACK)) return PT_OK;
    Dev& dv = g.dev[0];
    if ((rc = use_dev(dv))) return rc;
    if (!pin(buf, bytes)) return PT_OK;
    *used = true;
    if ((rc = ensure_dbuf(0, bytes))) return rc;
    drop_mirror();
    const int32_t w = j.width, h = j.height;
    int32_t rows = (h + kBands - 1) / kBands;
    rows = (rows + row_align - 1) / row_align * row_align;
    int k = 0;
    for (int32_t r0 = 0; r0 < h && k < kBands; r0 += rows, ++k) {
        const int32_t r1 = r0 + rows < h ? r0 + rows : h;
        const size_t off = (size_t)r0 * w * 3, len = (size_t)(r1 - r0) * w * 3 * sizeof(float);
        HIP_TRY(hipMemcpyAsync(dv.dbuf + off, buf + off, len, hipMemcpyHostToDevice, g.s_in));
        HIP_TRY(hipEventRecord(g.ev_in[k], g.s_in));
        HIP_TRY(hipStreamWaitEvent(dv.stream, g.ev_in[k], 0));
        Job b = j;
        b.row_start = r0;
        b.nrows = r1 - r0;
        b.buf = j.layout == PT_LAYOUT_TILED_PLANAR8 ? dv.dbuf : dv.dbuf + off;   // tiled: global offsets
        if ((rc = run(b))) return rc;
        HIP_TRY(hipEventRecord(g.ev_done[k], dv.stream));
        HIP_TRY(hipStreamWaitEvent(g.s_out, g.ev_done[k], 0));
        HIP_TRY(hipMemcpyAsync(buf + off, dv.dbuf + off, len, hipMemcpyDeviceToHost, g.s_out));
    }
    return PT_OK;
}

// Device d's share of a whole-frame job `j` (global geometry): its rows d::n, into its mirror.
template <typename Job>
Job shard_job(const Job& j, int d)
{
    Job b = j;
    b.buf = g.dev[d].dbuf;
    if (g.ndev > 1) {
        b.row_start = j.row_start + d;
        b.row_stride = g.ndev;
        b.nrows = shard_rows(j.nrows, g.ndev, d);
    }
    return b;
}

// Device d's rows of one tile job (tiled layout: rows are global, the buffer is full-size).
template <typename Job>
Job tile_shard_job(const Job& j, int d)
{
    Job b = j;
    b.buf = g.dev[d].dbuf;
    if (g.ndev > 1) {
        const int32_t ly0 = (int32_t)((((int64_t)d - j.row_start) % g.ndev + g.ndev) % g.ndev);
        b.row_start = j.row_start + ly0;
        b.row_stride = g.ndev;
        b.nrows = ly0 < j.nrows ? (j.nrows - 1 - ly0) / g.ndev + 1 : 0;
    }
    return b;
}

Geo geo_of(int32_t w, int32_t h, int32_t layout, int32_t tw, int32_t th)
{
    Geo geo;
    geo.w = w;
    geo.h = h;
    geo.tiled = layout == PT_LAYOUT_TILED_PLANAR8;
    geo.tw = tw;
    geo.th = th;
    return geo;
}

// One frame call on a host buffer: the job `j` (whole image) is rendered into the device mirrors
// of `buf` -- pipelined in row bands with PT_FLAG_PIN_HOST on one device, otherwise upload, render,
// download in turn (every device's share enqueued before any is waited for).
int render_frame(float* buf, PtJob j, int32_t row_align)
{
    int rc;
    const uint32_t spf = (uint32_t)g.cfg.samples_per_frame;
    bool banded = false;
    if ((rc = render_bands(buf, j, row_align, [](const PtJob& b) { return launch(g.dev[0], b, g.dev[0].stream, false); },
                           &banded)))
        return rc;
    if (banded) {
        g.frame += spf;
        HIP_TRY(hipStreamSynchronize(g.s_out));
        return sync_all();
    }
    const Geo geo = geo_of(j.width, j.height, j.layout, j.tile_w, j.tile_h);
    if ((rc = stage_in(buf, geo, Region{}))) return rc;
    for (int d = 0; d < g.ndev; ++d)
        if ((rc = launch(g.dev[d], shard_job(j, d), g.dev[d].stream, false))) return rc;
    g.frame += spf;
    return stage_out(buf, geo, Region{});
}

int grow(Dev& dv, void** p, size_t* cap, size_t bytes)
{
    if (bytes <= *cap) return PT_OK;
    if (*p) {
        HIP_TRY(hipStreamSynchronize(dv.stream));
        (void)hipFree(*p);
        *p = nullptr;
        *cap = 0;
    }
    if (hipMalloc(p, bytes) != hipSuccess) {
        *p = nullptr;
        return fail(PT_ENOMEM, "hipMalloc(%zu) failed", bytes);
    }
    *cap = bytes;
    return PT_OK;
}

// the accumulator geometry the output stage accepts (the layouts' own constraints)
int check_tone_args(const void* accum, const void* out, int32_t w, int32_t h, int32_t layout, int32_t tw, int32_t th,
                    int32_t format)
{
    if (!accum || !out) return fail(PT_EINVAL, "null accumulator/output");
    if (w <= 0 || h <= 0 || (int64_t)w * h > (int64_t)1 << 30) return fail(PT_EINVAL, "invalid size %dx%d", w, h);
    if (format != PT_PIXEL_RGBA8 && format != PT_PIXEL_XRGB8) return fail(PT_EINVAL, "unknown pixel format %d", format);
    if (layout == PT_LAYOUT_INTERLEAVED) return PT_OK;
    if (w % 8) return fail(PT_EINVAL, "planar layouts need width %% 8 == 0 (got %d)", w);
    if (layout == PT_LAYOUT_PLANAR8) return PT_OK;
    if (layout != PT_LAYOUT_TILED_PLANAR8) return fail(PT_EINVAL, "unknown layout %d", layout);
    if (tw <= 0 || th <= 0 || tw % 8 || w % tw || h % th)
        return fail(PT_EINVAL, "tiles %dx%d do not divide %dx%d (tile width multiple of 8)", tw, th, w, h);
    return PT_OK;
}

PtToneJob tone_job(const float* accum, int32_t w, int32_t h, int32_t layout, int32_t tw, int32_t th, uint32_t* out,
                   int32_t format)
{
    PtToneJob j{};
    j.accum = accum;
    j.width = w;
    j.height = h;
    j.layout = layout;
    j.tile_w = tw;
    j.tile_h = th;
    j.out = out;
    j.format = format;
    j.fast_aces = g.v4cfg.fast_aces;     // USE_FAST_APPROXIMATE_ACES_TONEMAP (flags.h:63)
    j.fast_gamma = g.v4cfg.fast_gamma;   // USE_FAST_APPROXIMATE_GAMMA (flags.h:62)
    return j;
}

// The output stage of the mirrored accumulator, per device on its own rows: every device converts
// its mirror (its compact rows, or the full-size tiled buffer of which it owns rows d::n) and copies
// its rows of the w x h pixel image into `out` (host).  Enqueued only; the caller synchronises.
int tone_mirror(int32_t layout, int32_t tw, int32_t th, uint32_t* out, int32_t format)
{
    int rc;
    const int32_t w = g.m.width, h = g.m.height;
    const int n = g.ndev;
    for (int d = 0; d < n; ++d) {
        Dev& dv = g.dev[d];
        if ((rc = use_dev(dv))) return rc;
        const bool compact = n > 1 && layout != PT_LAYOUT_TILED_PLANAR8;
        const int32_t nr = n > 1 ? shard_rows(h, n, d) : h;
        if (nr == 0) continue;
        const int32_t rows = compact ? nr : h;   // rows of the image this device converts
        if ((rc = grow(dv, (void**)&dv.dtone_out, &dv.dtone_out_cap, (size_t)w * rows * sizeof(uint32_t)))) return rc;
        const PtToneJob j = tone_job(dv.dbuf, w, rows, layout, tw, th, dv.dtone_out, format);
        hipError_t e = pt_launch_tonemap(j, dv.stream);
        if (e != hipSuccess) return fail(PT_EHIP, "tonemap launch failed: %s", hipGetErrorString(e));
        const size_t row = (size_t)w * sizeof(uint32_t);
        if (n == 1) {
            HIP_TRY(hipMemcpyAsync(out, dv.dtone_out, row * h, hipMemcpyDeviceToHost, dv.stream));
        } else {
            const uint32_t* src = compact ? dv.dtone_out : dv.dtone_out + (size_t)d * w;
            HIP_TRY(hipMemcpy2DAsync(out + (size_t)d * w, row * n, src, compact ? row : row * n, row, nr,
                                     hipMemcpyDeviceToHost, dv.stream));
        }
    }
    return PT_OK;
}

// PT_FLAG_GATHER_ROOT (several devices, deferred accumulator): assemble the whole accumulator of the
// mirrored buffer in the root's dgather.  Every device stores its own rows there (a kernel on its own
// stream, after its renders; remote stores over its xGMI link), then the root stream waits for all of
// them.  *out = the assembled W x H x 3 buffer (mirror layout) on the root, ordered on its stream.
int gather_root(float** out)
{
    int rc;
    const Geo geo = mirror_geo();
    const int n = g.ndev;
    Dev& r = g.dev[0];
    if ((rc = use_dev(r))) return rc;
    if (n == 1) {
        *out = r.dbuf;
        return PT_OK;
    }
    for (int d = 1; d < n; ++d)
        if (!g.dev[d].peer_root)
            return fail(PT_ESTATE, "PT_FLAG_GATHER_ROOT: device %d has no peer access to device %d", g.dev[d].ordinal,
                        r.ordinal);
    const size_t bytes = (size_t)geo.w * geo.h * 3 * sizeof(float);
    if ((rc = grow(r, (void**)&r.dgather, &r.dgather_cap, bytes))) return rc;
    HIP_TRY(hipEventRecord(g.ev_root_free, r.stream));   // (the root's earlier tonemap / copy of dgather)
    for (int d = 0; d < n; ++d) {
        Dev& dv = g.dev[d];
        if ((rc = use_dev(dv))) return rc;
        if (d > 0) HIP_TRY(hipStreamWaitEvent(dv.stream, g.ev_root_free, 0));
        PtScatterJob j{};
        j.src = dv.dbuf;
        j.dst = r.dgather;
        j.width = geo.w;
        j.height = geo.h;
        j.layout = geo.tiled ? PT_LAYOUT_TILED_PLANAR8 : PT_LAYOUT_INTERLEAVED;   // (planar8 rows: same bytes)
        j.tile_w = geo.tw;
        j.tile_h = geo.th;
        j.dev = d;
        j.ndev = n;
        j.nrows = shard_rows(geo.h, n, d);
        hipError_t e = pt_launch_scatter_rows(j, dv.stream);
        if (e != hipSuccess) return fail(PT_EHIP, "gather launch failed: %s", hipGetErrorString(e));
        if (d > 0) HIP_TRY(hipEventRecord(dv.ev_gather, dv.stream));
    }
    if ((rc = use_dev(r))) return rc;
    for (int d = 1; d < n; ++d) HIP_TRY(hipStreamWaitEvent(r.stream, g.dev[d].ev_gather, 0));
    *out = r.dgather;
    return PT_OK;
}

// The output stage of the deferred accumulator into host pixels: per device on its own rows, or
// (PT_FLAG_GATHER_ROOT) gathered on the root and converted there.  Enqueued; the caller synchronises.
int tone_output(int32_t layout, int32_t tw, int32_t th, uint32_t* out, int32_t format)
{
    int rc;
    if (g.ndev == 1 || !(g.cfg.flags & PT_FLAG_GATHER_ROOT)) return tone_mirror(layout, tw, th, out, format);
    float* acc = nullptr;
    if ((rc = gather_root(&acc))) return rc;
    Dev& r = g.dev[0];
    const int32_t w = g.m.width, h = g.m.height;
    if ((rc = grow(r, (void**)&r.dtone_out, &r.dtone_out_cap, (size_t)w * h * sizeof(uint32_t)))) return rc;
    const PtToneJob j = tone_job(acc, w, h, layout, tw, th, r.dtone_out, format);
    hipError_t e = pt_launch_tonemap(j, r.stream);
    if (e != hipSuccess) return fail(PT_EHIP, "tonemap launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(out, r.dtone_out, (size_t)w * h * sizeof(uint32_t), hipMemcpyDeviceToHost, r.stream));
    return PT_OK;
}

int check_frame_args(const float* buf, int32_t w, int32_t h, int32_t nc)
{
    if (!buf) return fail(PT_EINVAL, "null buffer");
    if (w <= 0 || h <= 0) return fail(PT_EINVAL, "invalid size %dx%d", w, h);
    if (nc != 3) return fail(PT_EINVAL, "NumChannels must be 3 (RGB f32), got %d", nc);
    if ((int64_t)w * h > (int64_t)1 << 30) return fail(PT_EINVAL, "image too large");
    if (w > kMaxDim || h > kMaxDim) return fail(PT_EINVAL, "image side > 2^24 (f32 pixel coordinates inexact)");
    return PT_OK;
}

int tiled_settings(int32_t w, int32_t h, int32_t ntx, int32_t nty, int32_t tw, int32_t th)
{
    // CheckValidSettings (Application.cpp:36-94) + the tile cover DemofoxRenderSimdTiled assumes
    if (ntx <= 0 || nty <= 0 || tw <= 0 || th <= 0) return fail(PT_EINVAL, "invalid tiling");
    if (tw % 8) return fail(PT_EINVAL, "tile width %d must be a multiple of 8 (SIMD lane width)", tw);
    if (w % 8) return fail(PT_EINVAL, "image width %d must be a multiple of 8", w);
    if (w % ntx || h % nty) return fail(PT_EINVAL, "image %dx%d not divisible into %dx%d tiles", w, h, ntx, nty);
    if (ntx * tw != w || nty * th != h) return fail(PT_EINVAL, "tiles %dx(%d) x %dx(%d) do not cover %dx%d", ntx, tw, nty, th, w, h);
    return PT_OK;
}

int check_texture(const pt_texture* t)
{
    if (!t->data) return fail(PT_EINVAL, "texture has no data");
    if (t->width <= 0 || t->height <= 0) return fail(PT_EINVAL, "invalid texture size %dx%d", t->width, t->height);
    if (t->components != 3) return fail(PT_EINVAL, "texture must have 3 components (RGB f32), got %d", t->components);
    if ((int64_t)t->width * t->height > (int64_t)1 << 28) return fail(PT_EINVAL, "texture too large");
    return PT_OK;
}

void release_env()
{
    for (int d = 0; d < g.ndev; ++d) {
        Dev& dv = g.dev[d];
        if (dv.denv) {
            (void)use_dev(dv);
            (void)hipStreamSynchronize(dv.stream);
            (void)hipFree(dv.denv);
        }
        dv.denv = nullptr;
    }
    g.env_w = g.env_h = 0;
    g.env_src = nullptr;
    g.have_env = false;
}

int upload_env(const pt_texture* t)
{
    int rc;
    if ((rc = check_texture(t))) return rc;
    const size_t bytes = (size_t)t->width * t->height * 3 * sizeof(float);
    release_env();
    for (int d = 0; d < g.ndev; ++d) {
        Dev& dv = g.dev[d];
        if ((rc = use_dev(dv))) return rc;
        if (hipMalloc(&dv.denv, bytes) != hipSuccess) {
            dv.denv = nullptr;
            release_env();
            return fail(PT_ENOMEM, "hipMalloc(env %zu) failed on device %d", bytes, dv.ordinal);
        }
        HIP_TRY(hipMemcpyAsync(dv.denv, t->data, bytes, hipMemcpyHostToDevice, dv.stream));
    }
    if ((rc = sync_all())) return rc;
    g.env_w = t->width;
    g.env_h = t->height;
    g.env_src = t->data;
    g.have_env = true;
    return PT_OK;
}

// ---- env sets (pt_v4_make_env_set; pt_v4.h PtV4Envs) ----
// One device allocation per set: the table of `count` PtV4EnvRec at its start, then the texels of every
// texture in index order, each on a 256-byte boundary.  Immutable after its one upload.
bool env_set_live(const pt_v4_env_set* s)
{
    for (const pt_v4_env_set* p = g.env_sets; p; p = p->next)
        if (p == s) return true;
    return false;
}

// unlink and free a live set (its device's stream is synchronised first: no launch reads it any more)
void release_env_set(pt_v4_env_set* s)
{
    for (pt_v4_env_set** p = &g.env_sets; *p; p = &(*p)->next)
        if (*p == s) {
            *p = s->next;
            break;
        }
    (void)use_dev(*s->dev);
    (void)hipStreamSynchronize(s->dev->stream);
    (void)hipFree(s->block);
    delete s;
}

// RenderTile argument checks (simd_tiled.cpp:489-535 assumptions; Application.cpp:36-94)
int check_tile(const pt_buffer_info* b, const pt_tile_info* t)
{
    int rc;
    if (!b || !t) return fail(PT_EINVAL, "null tile/buffer info");
    if ((rc = check_frame_args(b->data, b->width, b->height, b->num_channels))) return rc;
    const int32_t tw = t->tile_width, th = t->tile_height;
    if (tw <= 0 || th <= 0 || tw % 8) return fail(PT_EINVAL, "tile width %d must be a positive multiple of 8", tw);
    if (t->tile_x < 0 || t->tile_y < 0) return fail(PT_EINVAL, "negative tile index");
    if (t->tile_min_x != t->tile_x * tw || t->tile_max_x != t->tile_min_x + tw - 1 ||
        t->tile_min_y != t->tile_y * th || t->tile_max_y != t->tile_min_y + th - 1)
        return fail(PT_EINVAL, "tile bounds inconsistent with (TileX, TileY, TileWidth, TileHeight)");
    if (t->tile_max_x >= b->width || t->tile_max_y >= b->height) return fail(PT_EINVAL, "tile outside the buffer");
    if (b->width % tw) return fail(PT_EINVAL, "buffer width %d not a multiple of tile width %d", b->width, tw);
    if (g.ndev > 1 && b->height % th)
        return fail(PT_EINVAL, "several devices: buffer height %d must be a multiple of the tile height %d", b->height, th);
    return PT_OK;
}

// the diffuse-path job of one tile at the current frame (env: the config-4 miss term)
PtJob tile_job(const pt_buffer_info* b, const pt_tile_info* t, bool env)
{
    PtJob j = base_job(nullptr, b->width, b->height);
    j.layout = PT_LAYOUT_TILED_PLANAR8;
    j.tile_w = t->tile_width;
    j.tile_h = t->tile_height;
    j.col0 = t->tile_min_x;
    j.ncols = t->tile_width;
    j.row_start = t->tile_min_y;
    j.nrows = t->tile_height;
    j.frame_first = g.frame - (uint32_t)g.cfg.samples_per_frame + 1;
    if (env) {
        j.env_w = g.env_w;
        j.env_h = g.env_h;
    }
    return j;
}

PtJob with_env(PtJob j, const Dev& dv, bool env)
{
    if (env) j.env = dv.denv;
    return j;
}

// ---- v4 helpers ----------------------------------------------------------------------------------

int v4_rebuild()
{
    if (pt_v4_build_scene(&g.v4desc, &g.v4scene))
        return fail(PT_EINVAL, "v4 scene exceeds MAX_OBJECTS (%d quads + %d spheres, %d materials; limit %d)",
                    g.v4desc.nquads, g.v4desc.nspheres, g.v4desc.nmat, PT_V4_MAX_OBJECTS);
    g.v4_scene_ready = true;
    g.v4sky_ready = false;
    return PT_OK;
}

// The sky window of the current (scene, camera) (pt_v4_skywin.h): host arithmetic, built on first use
// after a scene edit or a camera change.  PT_MI355_V4_SKYWIN=0: no window (A/B timing, tests).
bool v4_skywin_off()
{
    static const bool off = getenv("PT_MI355_V4_SKYWIN") && !strcmp(getenv("PT_MI355_V4_SKYWIN"), "0");
    return off;
}

void v4_sky_window_of(const float position[3], PtV4SkyWin* out)   // the current scene seen from `position`
{
    pt_v4_sky_window_for(v4_skywin_off(), g.v4desc, position, out);
}

const PtV4SkyWin& v4_sky_window()
{
    if (!g.v4sky_ready) {
        v4_sky_window_of(g.v4cam.position, &g.v4sky);
        g.v4sky_ready = true;
    }
    return g.v4sky;
}

int v4_ensure_scene()
{
    if (g.v4_scene_ready) return PT_OK;
    pt_v4_default_scene_desc(&g.v4desc);   // InitializeGlobalRenderResources -> InitializeScene (v4 :1650-1654)
    return v4_rebuild();
}

// what a job takes from the pt_v4_config
void v4_config_fields(PtV4Job* j)
{
    j->random_jitter = g.v4cfg.random_jitter;
    j->rejection = g.v4cfg.rejection;
    j->accumulate = g.v4cfg.accumulate_frames;   // ACCUMULATE_FRAMES (flags.h:60)
    j->fast_exp = g.v4cfg.fast_exp;              // USE_FAST_APPROXIMATE_EXP (flags.h:64)
}

// what a job (PtJob, PtV4Job) takes from a device job: its rows, layout, frame range and bounces
template <class Job>
void device_job_fields(Job* j, const pt_device_job& dj)
{
    j->row_start = dj.row_start;
    j->row_stride = dj.row_stride;
    j->nrows = dj.nrows;
    j->layout = dj.layout;
    j->frame_first = dj.frame_first;
    j->nframes = dj.nframes;
    j->num_bounces = dj.num_bounces;
}

PtV4Job v4_job(float* buf, int32_t w, int32_t h)
{
    PtV4Job j{};
    j.buf = buf;
    j.width = w;
    j.height = h;
    j.col0 = 0;
    j.ncols = w;
    j.row_start = 0;
    j.row_stride = 1;
    j.nrows = h;
    j.layout = PT_LAYOUT_INTERLEAVED;
    j.frame_first = g.v4_frame + 1;
    j.nframes = 1;   // NUM_SAMPLES_PER_FRAME = 1: one frame per DemofoxRenderOptV4 call
    j.num_bounces = g.v4cfg.num_bounces;
    j.env_mode = PT_V4_ENV_NONE;
    v4_config_fields(&j);
    memcpy(j.cam_pos, g.v4cam.position, sizeof(j.cam_pos));
    j.cam_dist = g.v4cam_dist;
    // the literal-geometry instances also carry the default camera as literals (pt_v4_camera_is_default)
    j.default_scene = pt_v4_is_default_geometry(g.v4scene) && pt_v4_camera_is_default(j.cam_pos, j.cam_dist) ? 1 : 0;
    j.sky = v4_sky_window();   // (read by the generic instances only)
    return j;
}

int v4_use_env(PtV4Job& j)
{
    if (g.v4cfg.env_mode == PT_V4_ENV_NONE) return PT_OK;
    if (!g.have_env) return fail(PT_ESTATE, "v4 env mode %d without an env map", g.v4cfg.env_mode);
    j.env_mode = g.v4cfg.env_mode;
    j.env_w = g.env_w;
    j.env_h = g.env_h;
    return PT_OK;
}

// The logical device a device-resident job runs on: the device holding its buffer.
int dev_of(const void* p, Dev** out)
{
    if (g.ndev == 1) {
        *out = &g.dev[0];
        return PT_OK;
    }
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PT_EINVAL, "device job buffer is not device memory");
    }
    for (int d = 0; d < g.ndev; ++d)
        if (g.dev[d].ordinal == a.device) {
            *out = &g.dev[d];
            return PT_OK;
        }
    return fail(PT_ESTATE, "device job on device %d, which the library was not initialised with", a.device);
}

int parse_device_list(const char* s, pt_config* c)
{
    if (!s || !*s) return 0;
    int n = 0;
    if (!strcmp(s, "all")) {
        int cnt = 0;
        if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return 0;
        for (int i = 0; i < cnt && i < PT_MAX_DEVICES; ++i) c->devices[n++] = i;
    } else {
        const char* p = s;
        while (*p && n < PT_MAX_DEVICES) {
            char* end = nullptr;
            const long v = strtol(p, &end, 10);
            if (end == p || v < 0) return 0;
            c->devices[n++] = (int32_t)v;
            p = end;
            while (*p == ',' || *p == ' ') ++p;
        }
    }
    if (n == 0) return 0;
    c->device = c->devices[0];
    c->device_count = n;
    return n;
}

void free_dev(Dev& dv)
{
    if (use_dev(dv)) return;
    if (dv.stream) (void)hipStreamSynchronize(dv.stream);
    if (dv.dbuf) (void)hipFree(dv.dbuf);
    if (dv.dcounters) (void)hipFree(dv.dcounters);
    if (dv.derr) (void)hipFree(dv.derr);
    if (dv.dct) (void)hipFree(dv.dct);
    if (dv.herr) (void)hipHostFree(dv.herr);
    if (dv.dscene) (void)hipFree(dv.dscene);
    if (dv.dqueue) (void)hipFree(dv.dqueue);
    if (dv.denv) (void)hipFree(dv.denv);
    if (dv.dtone_in) (void)hipFree(dv.dtone_in);
    if (dv.dtone_out) (void)hipFree(dv.dtone_out);
    if (dv.dgather) (void)hipFree(dv.dgather);
    if (dv.ev_gather) (void)hipEventDestroy(dv.ev_gather);
    for (Dev::BatchSlot& s : dv.batch) {
        if (s.pending) (void)hipEventSynchronize(s.done);   // (its launch may run on a caller's stream)
        if (s.done) (void)hipEventDestroy(s.done);
        if (s.dev) (void)hipFree(s.dev);
        if (s.host) (void)hipHostFree(s.host);
        if (s.before) (void)hipFree(s.before);
    }
    for (Sched& sc : dv.sched)
        if (sc.used) free_sched(sc);
    for (hipEvent_t& e : dv.queue_event)
        if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < 2; ++i) {
        if (dv.chain.st[i]) (void)hipStreamSynchronize(dv.chain.st[i]), (void)hipStreamDestroy(dv.chain.st[i]);
        if (dv.chain.done[i]) (void)hipEventDestroy(dv.chain.done[i]);
    }
    if (dv.chain.ev_caller) (void)hipEventDestroy(dv.chain.ev_caller);
    if (dv.chain.area1) (void)hipFree(dv.chain.area1);
    if (dv.chain.qblk) (void)hipFree(dv.chain.qblk);
    if (dv.chain.started) (void)hipFree(dv.chain.started);
    if (dv.stream) (void)hipStreamDestroy(dv.stream);
    dv = Dev{};
}

int init_dev(Dev& dv, int32_t ordinal)
{
    dv = Dev{};
    dv.ordinal = ordinal;
    for (int16_t& a : dv.queue_alias) a = -1;
    HIP_TRY(hipSetDevice(ordinal));
    HIP_TRY(hipStreamCreateWithFlags(&dv.stream, hipStreamNonBlocking));
    if (hipMalloc(&dv.dcounters, kCounterSlots * sizeof(unsigned long long)) != hipSuccess)
        return fail(PT_ENOMEM, "hipMalloc(counters) failed");
    if (hipMalloc(&dv.derr, PT_ERR_WORDS * sizeof(uint32_t)) != hipSuccess) return fail(PT_ENOMEM, "hipMalloc(err) failed");
    if (hipHostMalloc(&dv.herr, PT_ERR_WORDS * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess)
        return fail(PT_ENOMEM, "hipHostMalloc(err) failed");
    {
        const uint32_t init[PT_ERR_WORDS] = {0u, ~0u, 0u, 0u, ~0u, ~0u};   // (pt_kernel.h: the words' meaning)
        HIP_TRY(hipMemcpy(dv.derr, init, sizeof(init), hipMemcpyHostToDevice));
        memcpy(dv.herr, init, sizeof(init));
    }
    if (hipMalloc(&dv.dqueue, (size_t)kQueueRing * PT_QUEUE_WORDS * sizeof(unsigned)) != hipSuccess)
        return fail(PT_ENOMEM, "hipMalloc(queue) failed");
    if (hipMalloc(&dv.dscene, sizeof(PtScene)) != hipSuccess) return fail(PT_ENOMEM, "hipMalloc(scene) failed");
    HIP_TRY(hipEventCreateWithFlags(&dv.ev_gather, hipEventDisableTiming));
    HIP_TRY(hipMemcpy(dv.dscene, &g.scene, sizeof(PtScene), hipMemcpyHostToDevice));
    {   // the chained-launch wait bound (pt_chain.h; test hook PT_MI355_TEST_CHAIN_POLLS, else the default --
        // set on every init: the device symbols outlive pt_shutdown)
        const char* tp = getenv("PT_MI355_TEST_CHAIN_POLLS");
        const uint32_t polls = tp ? (uint32_t)strtoul(tp, nullptr, 10) : 0u;
        HIP_TRY(pt_set_chain_polls(polls));
        HIP_TRY(pt_v4_set_chain_polls(polls));
    }
    return PT_OK;
}

}  // namespace

int pt_internal_fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfail(code, fmt, ap);
    va_end(ap);
    return code;
}

extern "C" {

void pt_default_config(pt_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->device = 0;
    c->num_bounces = 4;          // c_numBounces, scalar.cpp:19
    c->samples_per_frame = 1;    // NUM_SAMPLES_PER_FRAME, global_preprocessor_flags.h:30
    c->flags = 0;
    c->ambient[0] = c->ambient[1] = c->ambient[2] = 0.1f;   // scalar.cpp:307
    c->device_count = 1;
    c->devices[0] = 0;
    // the devices of a host that never calls pt_init (the reference-shaped drop-in): PT_MI355_DEVICES
    // = "all" or a list of HIP ordinals ("0,1,2,3"; repeats make logical shards of one GPU)
    parse_device_list(getenv("PT_MI355_DEVICES"), c);
}

int pt_init(const pt_config* cfg)
{
    pt_config c;
    if (cfg) c = *cfg;
    else pt_default_config(&c);
    if (c.num_bounces < 0 || c.num_bounces > 1024) return fail(PT_EINVAL, "num_bounces %d out of range", c.num_bounces);
    if (c.samples_per_frame < 1 || c.samples_per_frame > 65536)
        return fail(PT_EINVAL, "samples_per_frame %d out of range", c.samples_per_frame);
    if (c.device_count < 0 || c.device_count > PT_MAX_DEVICES)
        return fail(PT_EINVAL, "device_count %d out of range [0, %d]", c.device_count, PT_MAX_DEVICES);
    if (c.device_count <= 1) {   // one device: `device` (devices[] ignored)
        c.device_count = 1;
        c.devices[0] = c.device;
    }
    if (const char* cw = getenv("PT_MI355_CT_WAVES"); cw && strcmp(cw, "5") && strcmp(cw, "6") && strcmp(cw, "0"))
        return fail(PT_EINVAL, "PT_MI355_CT_WAVES=%s: 5, 6 or 0 (timed per geometry)", cw);
    if (g.inited) pt_shutdown();
    DeviceGuard guard;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    for (int d = 0; d < c.device_count; ++d)
        if (c.devices[d] < 0 || c.devices[d] >= ndev)
            return fail(PT_EHIP, "device %d not available (%d devices)", c.devices[d], ndev);
    c.device = c.devices[0];
    g.cfg = c;
    pt_build_demofox_scene(&g.scene, c.ambient);
    int rc;
    g.ndev = c.device_count;
    for (int d = 0; d < g.ndev; ++d)
        if ((rc = init_dev(g.dev[d], c.devices[d]))) {
            g.inited = true;   // release what was created
            pt_shutdown();
            return rc;
        }
    // peer access to the root for PT_FLAG_GATHER_ROOT (MI355X nodes: every GPU pair over xGMI)
    for (int d = 0; d < g.ndev; ++d) {
        Dev& dv = g.dev[d];
        if (dv.ordinal == g.dev[0].ordinal) {
            dv.peer_root = true;
            continue;
        }
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, dv.ordinal, g.dev[0].ordinal) != hipSuccess || !can) continue;
        HIP_TRY(hipSetDevice(dv.ordinal));
        const hipError_t e = hipDeviceEnablePeerAccess(g.dev[0].ordinal, 0);
        if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) dv.peer_root = true;
        (void)hipGetLastError();
    }
    HIP_TRY(hipSetDevice(g.dev[0].ordinal));
    HIP_TRY(hipEventCreateWithFlags(&g.ev_root_free, hipEventDisableTiming));
    HIP_TRY(hipStreamCreateWithFlags(&g.s_in, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&g.s_out, hipStreamNonBlocking));
    for (int k = 0; k < kBands; ++k) {
        HIP_TRY(hipEventCreateWithFlags(&g.ev_in[k], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&g.ev_done[k], hipEventDisableTiming));
    }
    HIP_TRY(hipEventCreateWithFlags(&g.ev_q, hipEventDisableTiming));
    g.frame = 0;
    g.ring_guard_cap = ~0u;
    g.cam_cache = !(getenv("PT_MI355_CAM_CACHE") && !strcmp(getenv("PT_MI355_CAM_CACHE"), "0"));
    g.no_ct = getenv("PT_MI355_NO_CT") && !strcmp(getenv("PT_MI355_NO_CT"), "1");
    g.test_chain_delay = getenv("PT_MI355_TEST_CHAIN_DELAY") ? (uint32_t)strtoul(getenv("PT_MI355_TEST_CHAIN_DELAY"), nullptr, 10) : 0u;
    g.sched_rebuild = getenv("PT_MI355_SCHED_REBUILD") ? std::max<unsigned long long>(2ull, strtoull(getenv("PT_MI355_SCHED_REBUILD"), nullptr, 10))
                                                        : kSchedRebuildDefault;
    g.unit_mult = getenv("PT_MI355_UNIT_MULT") ? std::max<uint32_t>(1u, (uint32_t)strtoul(getenv("PT_MI355_UNIT_MULT"), nullptr, 10)) : 2u;
    g.v4_ct_force = getenv("PT_MI355_V4_CT") && !strcmp(getenv("PT_MI355_V4_CT"), "1");
    g.v4_views_grid = getenv("PT_MI355_V4_VIEWS_GRID") ? (uint32_t)strtoul(getenv("PT_MI355_V4_VIEWS_GRID"), nullptr, 10) : 0u;
    g.ct_back_pct = 20;
    g.back_set = false;
    if (const char* bk = getenv("PT_MI355_BACK")) g.ct_back_pct = (uint32_t)strtoul(bk, nullptr, 10), g.back_set = true;
    g.ct_waves = 0;
    if (const char* cw = getenv("PT_MI355_CT_WAVES")) g.ct_waves = (uint32_t)strtoul(cw, nullptr, 10);
    g.ct_seq_len = g.ct_seq_pos = 0;
    if (const char* sq = getenv("PT_MI355_CT_WAVES_SEQ")) {
        for (const char* c = sq; *c && g.ct_seq_len < sizeof(g.ct_seq); ++c)
            if (*c == '5' || *c == '6') g.ct_seq[g.ct_seq_len++] = *c;
    }
    // test hook: PT_MI355_TEST_BAD_ENTRY=<position> overwrites that entry of every schedule built with
    // ~0u (a tile outside the launch) -- the queue's entry guard must report it (tests/test_gpu_guards.py)
    g.test_bad_entry = -1;
    if (const char* be = getenv("PT_MI355_TEST_BAD_ENTRY")) g.test_bad_entry = (int64_t)strtoll(be, nullptr, 10);
    g.split = 1;
    if (const char* sp = getenv("PT_MI355_SPLIT")) g.split = (uint32_t)strtoul(sp, nullptr, 10);
    if (const char* cap = getenv("PT_MI355_RING_GUARD_CAP")) {
        const unsigned long v = strtoul(cap, nullptr, 10);
        if (v > 0 && v < 0xfffffffful) g.ring_guard_cap = (uint32_t)v;
    }
    g.inited = true;
    return PT_OK;
}

void pt_shutdown(void)
{
    if (!g.inited) return;
    DeviceGuard guard;
    while (g.env_sets) release_env_set(g.env_sets);
    for (int d = 0; d < g.ndev; ++d) free_dev(g.dev[d]);
    if (g.ndev > 0) (void)hipSetDevice(g.cfg.devices[0]);
    unpin();
    for (int k = 0; k < kBands; ++k) {
        if (g.ev_in[k]) (void)hipEventDestroy(g.ev_in[k]);
        if (g.ev_done[k]) (void)hipEventDestroy(g.ev_done[k]);
    }
    if (g.ev_q) (void)hipEventDestroy(g.ev_q);
    if (g.ev_root_free) (void)hipEventDestroy(g.ev_root_free);
    if (g.s_in) (void)hipStreamDestroy(g.s_in);
    if (g.s_out) (void)hipStreamDestroy(g.s_out);
    g = State{};
}

const char* pt_last_error(void) { return g_err; }

int pt_set_frame(uint32_t frame)
{
    if (frame >= kMaxFrame) return fail(PT_EINVAL, "frame %u >= 2^24", frame);
    g.frame = frame;
    return PT_OK;
}

uint32_t pt_get_frame(void) { return g.frame; }

int pt_render_scalar(float* buf, int32_t w, int32_t h, int32_t nc)
{
    int rc;
    if ((rc = check_frame_args(buf, w, h, nc)) || (rc = ensure_init())) return rc;
    if ((rc = check_frame_budget((uint32_t)g.cfg.samples_per_frame))) return rc;
    DeviceGuard guard;
    return render_frame(buf, base_job(nullptr, w, h), 8);
}

int pt_render_simd(float* buf, int32_t w, int32_t h, int32_t nc)
{
    int rc;
    if ((rc = check_frame_args(buf, w, h, nc)) || (rc = ensure_init())) return rc;
    if (w % 8) return fail(PT_EINVAL, "image width %d must be a multiple of 8 (SIMD lane width)", w);
    if ((rc = check_frame_budget((uint32_t)g.cfg.samples_per_frame))) return rc;
    DeviceGuard guard;
    PtJob j = base_job(nullptr, w, h);
    j.layout = PT_LAYOUT_PLANAR8;
    return render_frame(buf, j, 8);
}

int pt_render_simd_tiled(float* buf, int32_t w, int32_t h, int32_t ntx, int32_t nty, int32_t tw, int32_t th, int32_t nc)
{
    int rc;
    if ((rc = check_frame_args(buf, w, h, nc)) || (rc = ensure_init())) return rc;
    if ((rc = tiled_settings(w, h, ntx, nty, tw, th))) return rc;
    if ((rc = check_frame_budget((uint32_t)g.cfg.samples_per_frame))) return rc;
    DeviceGuard guard;
    PtJob j = base_job(nullptr, w, h);
    j.layout = PT_LAYOUT_TILED_PLANAR8;
    j.tile_w = tw;
    j.tile_h = th;
    return render_frame(buf, j, th);
}

int pt_set_env_map(const pt_texture* tex)
{
    int rc;
    if ((rc = ensure_init())) return rc;
    DeviceGuard guard;
    if (!tex) {
        release_env();
        return PT_OK;
    }
    return upload_env(tex);
}

int pt_v4_make_env_set(const pt_texture* texs, int32_t n, pt_v4_env_set** out)
{
    int rc;
    if (!texs) return fail(PT_EINVAL, "null texture array");
    if (!out) return fail(PT_EINVAL, "null env set result");
    if (n < 1 || n > PT_V4_MAX_VIEWS) return fail(PT_EINVAL, "%d textures outside [1, %d]", n, PT_V4_MAX_VIEWS);
    const auto up256 = [](size_t b) { return (b + 255u) & ~(size_t)255u; };
    std::vector<size_t> off((size_t)n);
    size_t bytes = up256((size_t)n * sizeof(PtV4EnvRec));
    for (int32_t i = 0; i < n; ++i) {
        if ((rc = check_texture(&texs[i]))) {
            char why[400];
            snprintf(why, sizeof(why), "%s", g_err);
            return fail(rc, "texture %d: %s", i, why);
        }
        off[(size_t)i] = bytes;
        bytes += up256((size_t)texs[i].width * texs[i].height * 3 * sizeof(float));
    }
    if ((rc = ensure_init())) return rc;
    DeviceGuard guard;
    Dev& dv = g.dev[0];
    if ((rc = use_dev(dv))) return rc;
    // staged on the host, so that table and texels travel in one copy
    std::unique_ptr<unsigned char[]> host(new (std::nothrow) unsigned char[bytes]);
    std::unique_ptr<pt_v4_env_set> set(new (std::nothrow) pt_v4_env_set);
    if (!host || !set) return fail(PT_ENOMEM, "no host memory to stage an env set of %zu bytes", bytes);
    if (hipMalloc((void**)&set->block, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PT_ENOMEM, "hipMalloc(env set, %zu bytes) failed on device %d", bytes, dv.ordinal);
    }
    memset(host.get(), 0, off[0]);
    PtV4EnvRec* const rec = reinterpret_cast<PtV4EnvRec*>(host.get());
    for (int32_t i = 0; i < n; ++i) {
        const size_t tb = (size_t)texs[i].width * texs[i].height * 3 * sizeof(float);
        rec[i] = PtV4EnvRec{reinterpret_cast<const float*>(set->block + off[(size_t)i]), texs[i].width, texs[i].height};
        memcpy(host.get() + off[(size_t)i], texs[i].data, tb);
        memset(host.get() + off[(size_t)i] + tb, 0, up256(tb) - tb);
    }
    hipError_t e = hipMemcpyAsync(set->block, host.get(), bytes, hipMemcpyHostToDevice, dv.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dv.stream);
    if (e != hipSuccess) {
        (void)hipFree(set->block);
        return fail(PT_EHIP, "env set upload failed: %s", hipGetErrorString(e));
    }
    set->dev = &dv;
    set->table = reinterpret_cast<const PtV4EnvRec*>(set->block);
    set->count = n;
    set->next = g.env_sets;
    g.env_sets = set.get();
    *out = set.release();
    return PT_OK;
}

void pt_v4_free_env_set(pt_v4_env_set* set)
{
    if (!set || !env_set_live(set)) return;   // (NULL, freed already, or released by pt_shutdown)
    DeviceGuard guard;
    release_env_set(set);
}

static int ensure_env(const pt_texture* tex)
{
    int rc;
    if ((rc = check_texture(tex))) return rc;
    if (!g.have_env || g.env_src != tex->data || g.env_w != tex->width || g.env_h != tex->height)
        return upload_env(tex);
    return PT_OK;
}

int pt_render_simt_textured(float* buf, int32_t w, int32_t h, int32_t ntx, int32_t nty, int32_t tw, int32_t th,
                            int32_t nc, const pt_texture* tex)
{
    int rc;
    if (!tex) return fail(PT_EINVAL, "null texture");
    if ((rc = check_frame_args(buf, w, h, nc)) || (rc = ensure_init())) return rc;
    if ((rc = tiled_settings(w, h, ntx, nty, tw, th)) || (rc = check_texture(tex))) return rc;
    if ((rc = check_frame_budget((uint32_t)g.cfg.samples_per_frame))) return rc;
    DeviceGuard guard;
    if ((rc = ensure_env(tex))) return rc;
    PtJob j = base_job(nullptr, w, h);
    j.layout = PT_LAYOUT_TILED_PLANAR8;   // RenderTile, simt_textured.cpp:491-533
    j.tile_w = tw;
    j.tile_h = th;
    j.env_w = g.env_w;
    j.env_h = g.env_h;
    const uint32_t spf = (uint32_t)g.cfg.samples_per_frame;
    bool banded = false;
    if ((rc = render_bands(buf, j, th, [](const PtJob& b) {
             return launch(g.dev[0], with_env(b, g.dev[0], true), g.dev[0].stream, false);
         }, &banded)))
        return rc;
    if (banded) {
        g.frame += spf;
        HIP_TRY(hipStreamSynchronize(g.s_out));
        return sync_all();
    }
    const Geo geo = geo_of(w, h, j.layout, tw, th);
    if ((rc = stage_in(buf, geo, Region{}))) return rc;
    for (int d = 0; d < g.ndev; ++d)
        if ((rc = launch(g.dev[d], with_env(shard_job(j, d), g.dev[d], true), g.dev[d].stream, false))) return rc;
    g.frame += spf;
    return stage_out(buf, geo, Region{});
}

int pt_begin_frame(void)
{
    int rc;
    if ((rc = ensure_init())) return rc;
    if ((rc = check_frame_budget((uint32_t)g.cfg.samples_per_frame))) return rc;
    g.frame += (uint32_t)g.cfg.samples_per_frame;
    return PT_OK;
}

int pt_render_tile(const pt_buffer_info* b, const pt_tile_info* t)
{
    int rc;
    if ((rc = ensure_init()) || (rc = check_tile(b, t))) return rc;
    if (g.frame < (uint32_t)g.cfg.samples_per_frame)
        return fail(PT_ESTATE, "RenderTile before the first frame was started (pt_begin_frame)");
    DeviceGuard guard;
    const Geo geo = geo_of(b->width, b->height, PT_LAYOUT_TILED_PLANAR8, t->tile_width, t->tile_height);
    Region rg;
    rg.whole = false;
    rg.tile_x = t->tile_x;
    rg.tile_y = t->tile_y;
    if ((rc = stage_in(b->data, geo, rg))) return rc;
    const PtJob j = tile_job(b, t, false);
    for (int d = 0; d < g.ndev; ++d)
        if ((rc = launch(g.dev[d], tile_shard_job(j, d), g.dev[d].stream, false))) return rc;
    return stage_out(b->data, geo, rg);
}

int pt_readback(float* buf)
{
    if (!g.inited || !g.m.valid || buf != g.m.host)
        return fail(PT_ESTATE, "no deferred device accumulator for this buffer");
    DeviceGuard guard;
    int rc;
    const Geo geo = mirror_geo();
    if (g.ndev > 1 && (g.cfg.flags & PT_FLAG_GATHER_ROOT)) {   // assembled on the root: one copy
        float* acc = nullptr;
        if ((rc = gather_root(&acc))) return rc;
        HIP_TRY(hipMemcpyAsync(buf, acc, g.m.bytes, hipMemcpyDeviceToHost, g.dev[0].stream));
        return sync_all();
    }
    for (int d = 0; d < g.ndev; ++d)
        if ((rc = use_dev(g.dev[d])) || (rc = xfer(d, geo, buf, false, Region{}))) return rc;
    return sync_all();
}

int pt_gather_root(const float* buf, const float** device_accum)
{
    if (!device_accum) return fail(PT_EINVAL, "null output pointer");
    if (!g.inited || !g.m.valid || buf != g.m.host)
        return fail(PT_ESTATE, "no deferred device accumulator for this buffer");
    DeviceGuard guard;
    int rc;
    float* acc = nullptr;
    if ((rc = gather_root(&acc)) || (rc = sync_all())) return rc;
    *device_accum = acc;
    return PT_OK;
}

int pt_release_buffer(const void* buf)
{
    if (!g.inited) return PT_OK;
    DeviceGuard guard;
    if (!buf || buf == (const void*)g.m.host) {
        (void)sync_all();   // nothing in flight may still copy into it
        drop_mirror();
    }
    if (g.pinned && (!buf || buf == (const void*)g.pinned)) unpin();
    return PT_OK;
}

static int device_job(const pt_device_job* dj, PtJob* j)
{
    int rc;
    if ((rc = pt_check_device_job(dj, fail))) return rc;   // (pt_v4_batch.h)
    *j = base_job(dj->buf, dj->width, dj->height);
    device_job_fields(j, *dj);
    if (dj->use_env) {
        if (!g.have_env) return fail(PT_ESTATE, "use_env without an env map (pt_set_env_map)");
        j->env_w = g.env_w;
        j->env_h = g.env_h;
    }
    return PT_OK;
}

#if PT_DIAG
static void diag_dump(const unsigned long long* h)
{
    fprintf(stderr, "PT_DIAG cycles: A %llu take %llu dir %llu trace %llu shade %llu C %llu tile %llu\n",
            h[PT_CNT_N + 0], h[PT_CNT_N + 1], h[PT_CNT_N + 2], h[PT_CNT_N + 3], h[PT_CNT_N + 4], h[PT_CNT_N + 5],
            h[PT_CNT_N + 6]);
    fprintf(stderr, "PT_DIAG wave lifetimes %llu memtime ticks, %llu realtime (100 MHz) ticks\n", h[PT_CNT_N + 7],
            h[PT_CNT_N + 10]);
    const unsigned long long r0 = h[PT_CNT_N + 12];
    fprintf(stderr, "PT_DIAG realtime (us from first start): last start %.1f, first end %.1f, last end %.1f\n",
            (h[PT_CNT_N + 8] - r0) * 0.01, (h[PT_CNT_N + 9] - r0) * 0.01, (h[PT_CNT_N + 11] - r0) * 0.01);
    if (const char* path = getenv("PT_DIAG_OUT")) {
        FILE* f = fopen(path, "wb");
        if (f) {
            fwrite(h + 32, sizeof(unsigned long long), 4 * 65536 + 96 * 65536, f);
            fclose(f);
        }
    }
}
#endif

int pt_tonemap_device(const float* accum, int32_t w, int32_t h, int32_t layout, int32_t tw, int32_t th, uint32_t* out,
                      int32_t format, void* stream)
{
    int rc;
    if ((rc = ensure_init()) || (rc = check_tone_args(accum, out, w, h, layout, tw, th, format))) return rc;
    DeviceGuard guard;
    Dev* dv = nullptr;
    if ((rc = dev_of(accum, &dv)) || (rc = use_dev(*dv))) return rc;
    const PtToneJob j = tone_job(accum, w, h, layout, tw, th, out, format);
    hipError_t e = pt_launch_tonemap(j, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PT_EHIP, "tonemap launch failed: %s", hipGetErrorString(e));
    return PT_OK;
}

int pt_tonemap(const float* accum, int32_t w, int32_t h, int32_t layout, int32_t tw, int32_t th, uint32_t* out,
               int32_t format)
{
    int rc;
    if ((rc = ensure_init()) || (rc = check_tone_args(accum, out, w, h, layout, tw, th, format))) return rc;
    DeviceGuard guard;
    const size_t in_bytes = (size_t)w * h * 3 * sizeof(float), out_bytes = (size_t)w * h * sizeof(uint32_t);
    const bool tiled = layout == PT_LAYOUT_TILED_PLANAR8;
    if (g.m.valid && accum == g.m.host && g.m.bytes == in_bytes && g.m.width == w && g.m.height == h &&
        (g.ndev == 1 || (g.m.tiled == tiled && (!tiled || (g.m.tile_w == tw && g.m.tile_h == th))))) {
        // the deferred accumulator is already in HBM: each device converts its own rows (or the root
        // converts the gathered image, PT_FLAG_GATHER_ROOT)
        if ((rc = tone_output(layout, tw, th, out, format))) return rc;
        return sync_all();
    }
    Dev& dv = g.dev[0];
    if ((rc = use_dev(dv))) return rc;
    if ((rc = grow(dv, (void**)&dv.dtone_in, &dv.dtone_in_cap, in_bytes))) return rc;
    HIP_TRY(hipMemcpyAsync(dv.dtone_in, accum, in_bytes, hipMemcpyHostToDevice, dv.stream));
    if ((rc = grow(dv, (void**)&dv.dtone_out, &dv.dtone_out_cap, out_bytes))) return rc;
    const PtToneJob j = tone_job(dv.dtone_in, w, h, layout, tw, th, dv.dtone_out, format);
    hipError_t e = pt_launch_tonemap(j, dv.stream);
    if (e != hipSuccess) return fail(PT_EHIP, "tonemap launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(out, dv.dtone_out, out_bytes, hipMemcpyDeviceToHost, dv.stream));
    HIP_TRY(hipStreamSynchronize(dv.stream));
    return PT_OK;
}

int pt_render_device(const pt_device_job* dj, void* stream)
{
    int rc;
    PtJob j;
    Dev* dv = nullptr;
    DeviceGuard guard;
    if ((rc = ensure_init()) || (rc = device_job(dj, &j)) || (rc = dev_of(dj->buf, &dv))) return rc;
    if (dj->use_env) j.env = dv->denv;
#if PT_DIAG   // diagnostic build: with PT_DIAG_OUT set, a device launch records and dumps its
              // timeline (synchronous); without it launches run as usual (warm-up at full clocks)
    if (!getenv("PT_DIAG_OUT")) return launch(*dv, j, (hipStream_t)stream, false);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(dv->dcounters, 0, kCounterSlots * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(dv->dcounters + PT_CNT_N + 9, 0xff, sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(dv->dcounters + PT_CNT_N + 12, 0xff, sizeof(unsigned long long), st));
    j.counters = dv->dcounters;
    if ((rc = launch(*dv, j, st, false))) return rc;
    static unsigned long long h[kCounterSlots];
    HIP_TRY(hipMemcpyAsync(h, dv->dcounters, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    diag_dump(h);
    return PT_OK;
#else
    return launch(*dv, j, (hipStream_t)stream, false);
#endif
}

int pt_render_device_chain(const pt_device_job* dj, void* stream)
{
    int rc;
    PtJob j;
    Dev* dv = nullptr;
    DeviceGuard guard;
    if ((rc = ensure_init()) || (rc = device_job(dj, &j)) || (rc = dev_of(dj->buf, &dv))) return rc;
    if (dj->use_env) j.env = dv->denv;
#if PT_DIAG
    if (getenv("PT_DIAG_OUT")) return pt_render_device(dj, stream);   // (the diagnostic timeline: one launch)
#endif
    return launch_chain(*dv, j, (hipStream_t)stream);
}

int pt_chain_counts(uint64_t* restarts, uint64_t* continued)
{
    if (!restarts || !continued) return fail(PT_EINVAL, "null output");
    *restarts = *continued = 0;
    for (int d = 0; d < (g.inited ? g.ndev : 0); ++d) {
        *restarts += g.dev[d].chain.restarts;
        *continued += g.dev[d].chain.continued;
    }
    return PT_OK;
}

int pt_render_device_present(const pt_device_job* dj, uint32_t* pixels, int32_t format, void* stream)
{
    int rc;
    PtJob j;
    Dev* dv = nullptr;
    DeviceGuard guard;
    if (!pixels) return fail(PT_EINVAL, "null pixel buffer");
    if (format != PT_PIXEL_RGBA8 && format != PT_PIXEL_XRGB8) return fail(PT_EINVAL, "unknown pixel format %d", format);
    if ((rc = ensure_init()) || (rc = device_job(dj, &j)) || (rc = dev_of(dj->buf, &dv))) return rc;
    if (dj->use_env) j.env = dv->denv;
    j.pix_out = pixels;
    j.pix_xrgb = format == PT_PIXEL_XRGB8;
    return launch(*dv, j, (hipStream_t)stream, false);
}

int pt_launch_variant(const pt_device_job* dj, int32_t* waves, int32_t* back_pct)
{
    int rc;
    PtJob j;
    Dev* dv = nullptr;
    if (!waves || !back_pct) return fail(PT_EINVAL, "null output");
    *waves = 0;
    *back_pct = 0;
    if ((rc = ensure_init()) || (rc = device_job(dj, &j)) || (rc = dev_of(dj->buf, &dv))) return rc;
    if (dj->use_env) j.env = dv->denv;
    if (g.no_ct) return PT_OK;   // (the per-tile pools)
    const bool env = j.env != nullptr;
    const uint32_t dflt = pt_plan_back(j.nframes, g.ct_back_pct);
    const SchedKey key = sched_key(j);
    // fixed (ct_occupancy): by the switch, or a geometry that is never scheduled, so never timed
    if (g.ct_waves || key.ntiles < kSchedMinTiles) {
        *waves = env ? pt_ct_env_waves() : g.ct_waves ? (int32_t)g.ct_waves : 5;
        *back_pct = (int32_t)dflt;
        return PT_OK;
    }
    for (const Sched& s : dv->sched) {
        if (!s.used || !(s.key == key) || s.wide < 0) continue;
        const PtVariant v = pt_plan_variant(env, s.wide, dflt, g.back_set);   // (the pick, as ct_occupancy applies it)
        *waves = env ? pt_ct_env_waves() : v.wide ? 6 : 5;
        *back_pct = (int32_t)v.back_pct;
        return PT_OK;
    }
    return PT_OK;   // (undecided)
}

int pt_count_device(const pt_device_job* dj, void* stream, pt_work_counts* out)
{
    int rc;
    PtJob j;
    Dev* dv = nullptr;
    DeviceGuard guard;
    if (!out) return fail(PT_EINVAL, "null counts");
    if ((rc = ensure_init()) || (rc = device_job(dj, &j)) || (rc = dev_of(dj->buf, &dv)) || (rc = use_dev(*dv))) return rc;
    if (dj->use_env) j.env = dv->denv;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(dv->dcounters, 0, kCounterSlots * sizeof(unsigned long long), st));
#if PT_DIAG
    HIP_TRY(hipMemsetAsync(dv->dcounters + PT_CNT_N + 9, 0xff, sizeof(unsigned long long), st));    // min
    HIP_TRY(hipMemsetAsync(dv->dcounters + PT_CNT_N + 12, 0xff, sizeof(unsigned long long), st));   // min
#endif
    j.counters = dv->dcounters;
    if ((rc = launch(*dv, j, st, true))) return rc;
    static unsigned long long h[kCounterSlots];
    HIP_TRY(hipMemcpyAsync(h, dv->dcounters, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
#if PT_DIAG
    diag_dump(h);
#endif
    if ((rc = sync_all())) return rc;   // the launch's error words
    out->segments = h[PT_CNT_SEGMENTS];
    out->lane_slots = h[PT_CNT_LANE_SLOTS];
    out->samples = h[PT_CNT_SAMPLES];
    out->escaped = h[PT_CNT_ESCAPED];
    out->primary = h[PT_CNT_PRIMARY];
    out->quad_fallbacks = h[PT_CNT_FALLBACK];
    out->sphere_fallbacks = 0;
    out->sky_skipped = h[PT_CNT_SKY];
    dv->cam_checked = h[PT_CNT_CAM_CHECKED];
    return PT_OK;
}

int pt_cam_cache_query(const pt_device_job* dj, void* stream, int32_t* state, uint64_t* compared)
{
    int rc;
    PtJob j;
    Dev* dv = nullptr;
    if (!state || !compared) return fail(PT_EINVAL, "null output");
    *state = PT_CAM_CACHE_NONE;
    *compared = 0;
    if ((rc = ensure_init()) || (rc = device_job(dj, &j)) || (rc = dev_of(dj->buf, &dv))) return rc;
    if (dj->use_env) j.env = dv->denv;
    *compared = dv->cam_checked;
    const SchedKey key = sched_key(j);
    for (const Sched& s : dv->sched) {
        if (!s.used || s.stream != (hipStream_t)stream || !(s.key == key)) continue;
        if (s.cam && cam_launch_qualifies(s, j.nframes))
            *state = s.cam_state == kCamEmpty ? PT_CAM_CACHE_EMPTY : s.cam_state == kCamFilled ? PT_CAM_CACHE_FILLED : PT_CAM_CACHE_SETTLED;
        break;
    }
    return PT_OK;
}

int pt_check_device_errors(void)
{
    if (!g.inited) return PT_OK;
    DeviceGuard guard;
    return sync_all();
}

int32_t pt_initialized_device(void) { return g.inited ? g.dev[0].ordinal : -1; }

int32_t pt_build_checked(void) { return PT_CHECKED ? 1 : 0; }

int32_t pt_device_count(void) { return g.inited ? g.ndev : 0; }

int32_t pt_device_ordinal(int32_t i) { return g.inited && i >= 0 && i < g.ndev ? g.dev[i].ordinal : -1; }

int pt_unpin_host(const void* buf)
{
    if (!g.inited || !g.pinned) return PT_OK;
    if (buf && buf != (const void*)g.pinned) return PT_OK;
    DeviceGuard guard;
    unpin();
    return PT_OK;
}

// ---- v4 renderer -------------------------------------------------------------------------------

void pt_v4_default_config(pt_v4_config* c)
{
    if (!c) return;
    c->env_mode = PT_V4_ENV_EQUIRECT;   // USE_ENV_MAP 1, USE_ENV_CUBEMAP 0
    c->random_jitter = 1;               // USE_RANDOM_JITTER_TEXTURE_SAMPLING 1
    c->rejection = 1;                   // USE_UNIT_VECTOR_REJECTION_SAMPLING 1
    c->num_bounces = 8;                 // c_numBounces, v4 :23
    c->output_to_screen = 1;            // OUTPUT_TO_SCREEN = !RENDER_OFFLINE
    c->accumulate_frames = 1;           // ACCUMULATE_FRAMES 1
    c->fast_aces = 1;                   // USE_FAST_APPROXIMATE_ACES_TONEMAP 1
    c->fast_gamma = 1;                  // USE_FAST_APPROXIMATE_GAMMA 1
    c->fast_exp = 1;                    // USE_FAST_APPROXIMATE_EXP 1
}

int pt_v4_set_config(const pt_v4_config* c)
{
    if (!c) return fail(PT_EINVAL, "null v4 config");
    if (c->env_mode < PT_V4_ENV_NONE || c->env_mode > PT_V4_ENV_CUBEMAP) return fail(PT_EINVAL, "unknown env mode %d", c->env_mode);
    if (c->num_bounces < 0 || c->num_bounces > 1024) return fail(PT_EINVAL, "num_bounces %d out of range", c->num_bounces);
    g.v4cfg = *c;
    g.v4cfg.random_jitter = c->random_jitter != 0;
    g.v4cfg.rejection = c->rejection != 0;
    g.v4cfg.output_to_screen = c->output_to_screen != 0;
    g.v4cfg.accumulate_frames = c->accumulate_frames != 0;
    g.v4cfg.fast_aces = c->fast_aces != 0;
    g.v4cfg.fast_gamma = c->fast_gamma != 0;
    g.v4cfg.fast_exp = c->fast_exp != 0;
    return PT_OK;
}

int pt_v4_get_config(pt_v4_config* c)
{
    if (!c) return fail(PT_EINVAL, "null v4 config");
    *c = g.v4cfg;
    return PT_OK;
}

int pt_v4_initialize_global_render_resources(void)
{
    int rc;
    if ((rc = ensure_init())) return rc;
    return v4_ensure_scene();
}

int pt_v4_reinitialize_render_tile_data(void)
{
    // Resize reallocated the render target (Application.cpp:142-154): the old buffer is gone, so
    // neither its page-lock nor its deferred device copy may outlive it (dropped, not written back)
    return pt_release_buffer(nullptr);
}

int pt_v4_initialize_scene(void)
{
    pt_v4_default_scene_desc(&g.v4desc);
    return v4_rebuild();
}

int pt_v4_clear_scene(void)
{
    memset(&g.v4desc, 0, sizeof(g.v4desc));
    return v4_rebuild();
}

int pt_v4_add_material(const pt_v4_material* m)
{
    int rc;
    if (!m) return fail(PT_EINVAL, "null material");
    if ((rc = v4_ensure_scene())) return rc;
    if (g.v4desc.nmat >= PT_V4_MAX_OBJECTS) return fail(PT_EINVAL, "more than MAX_MATERIALS (%d) materials", PT_V4_MAX_OBJECTS);
    static_assert(sizeof(pt_v4_material) == sizeof(PtV4Mat), "material layout");
    memcpy(&g.v4desc.mat[g.v4desc.nmat], m, sizeof(PtV4Mat));
    const int idx = g.v4desc.nmat++;
    if ((rc = v4_rebuild())) return rc;
    return idx;   // AddMaterialToScene returns scene.NumMaterials++ (v4 :1387)
}

int pt_v4_add_quad(const float v[12])
{
    int rc;
    if (!v) return fail(PT_EINVAL, "null quad");
    if ((rc = v4_ensure_scene())) return rc;
    if (g.v4desc.nquads + g.v4desc.nspheres >= PT_V4_MAX_OBJECTS)
        return fail(PT_EINVAL, "more than MAX_OBJECTS (%d) objects", PT_V4_MAX_OBJECTS);
    memcpy(g.v4desc.quad[g.v4desc.nquads++], v, 12 * sizeof(float));
    if ((rc = v4_rebuild())) return rc;
    return g.v4desc.nquads;   // v4 :1394
}

int pt_v4_add_sphere(const float pr[4])
{
    int rc;
    if (!pr) return fail(PT_EINVAL, "null sphere");
    if ((rc = v4_ensure_scene())) return rc;
    if (g.v4desc.nquads + g.v4desc.nspheres >= PT_V4_MAX_OBJECTS)
        return fail(PT_EINVAL, "more than MAX_OBJECTS (%d) objects", PT_V4_MAX_OBJECTS);
    memcpy(g.v4desc.sphere[g.v4desc.nspheres++], pr, 4 * sizeof(float));
    if ((rc = v4_rebuild())) return rc;
    return g.v4desc.nquads;   // v4 :1400 returns NumQuadObjects
}

int pt_v4_set_frame(uint32_t frame)
{
    if (frame >= kMaxFrame) return fail(PT_EINVAL, "frame %u >= 2^24", frame);
    g.v4_frame = frame;
    return PT_OK;
}

uint32_t pt_v4_get_frame(void) { return g.v4_frame; }

int pt_v4_get_scene_tables(float* out, int32_t n, int32_t* nq, int32_t* ns)
{
    int rc;
    if ((rc = v4_ensure_scene())) return rc;
    const PtV4Scene& s = g.v4scene;
    const int32_t need = 18 * s.nquads + 4 * s.nspheres + 17 * PT_V4_MAX_OBJECTS;
    if (nq) *nq = s.nquads;
    if (ns) *ns = s.nspheres;
    if (!out || n < need) return need;
    float* o = out;
    for (int i = 0; i < s.nquads; ++i) {
        memcpy(o, &s.quad[i], sizeof(PtV4Quad));
        o += 18;
    }
    for (int i = 0; i < s.nspheres; ++i) {
        memcpy(o, s.sph[i], 4 * sizeof(float));
        o += 4;
    }
    memcpy(o, s.mat, sizeof(s.mat));
    return need;
}

void pt_v4_default_camera(pt_v4_camera* c)
{
    if (!c) return;
    c->position[0] = 0.0f;   // camera.Position = float3(0, 0, c_cameraDistance * 40), v4 :1501
    c->position[1] = 0.0f;
    c->position[2] = 1.0f * 40.0f;
    c->fov_degrees = 90.0f;  // c_FOVDegrees, v4 :20
}

int pt_v4_set_camera(const pt_v4_camera* c)
{
    int rc;
    float dist = 0.0f;
    if (!c) return fail(PT_EINVAL, "null v4 camera");
    if ((rc = pt_v4_check_camera(c, &dist, -1, fail))) return rc;   // (pt_v4_batch.h)
    g.v4cam = *c;
    g.v4cam_dist = dist;
    g.v4sky_ready = false;
    // a live v4 chain ends: the next chained launch restarts, as after any other non-chained launch.
    // (The tile schedules are kept: the order only affects speed, and the periodic rebuild picks the new
    // view's costs up, as after a scene edit -- DESIGN.md 3b.)
    for (int d = 0; d < g.ndev; ++d)
        if (g.dev[d].chain.sched && g.dev[d].chain.sched->key.kind >= 1) g.dev[d].chain.sched = nullptr;
    return PT_OK;
}

int pt_v4_get_camera(pt_v4_camera* c, float* distance)
{
    if (!c) return fail(PT_EINVAL, "null v4 camera");
    *c = g.v4cam;
    if (distance) *distance = g.v4cam_dist;
    return PT_OK;
}

int pt_v4_get_sky_window(float* rects, int32_t n, int32_t* nrects)
{
    int rc;
    if (!nrects) return fail(PT_EINVAL, "null nrects");
    if ((rc = v4_ensure_scene())) return rc;
    const PtV4SkyWin& w = v4_sky_window();
    *nrects = w.nrects;
    const int32_t need = w.nrects > 0 ? 4 * w.nrects : 0;
    if (!rects || n < need) return need;
    memcpy(rects, w.rect, (size_t)need * sizeof(float));
    return need;
}

int pt_render_opt_v4(float* buf, int32_t w, int32_t h, int32_t ntx, int32_t nty, int32_t tw, int32_t th, int32_t nc,
                     const pt_texture* tex, void* screen)
{
    int rc;
    if ((rc = check_frame_args(buf, w, h, nc)) || (rc = ensure_init())) return rc;
    if ((rc = tiled_settings(w, h, ntx, nty, tw, th))) return rc;
    if ((int64_t)ntx * nty > 1024) return fail(PT_EINVAL, "%d x %d tiles exceed NumMaxThreads (1024, v4 :1341)", ntx, nty);
    if ((rc = v4_ensure_scene())) return rc;
    if (g.v4_frame + 1u >= kMaxFrame) return fail(PT_EINVAL, "v4 frame counter exceeds the exact f32 range 2^24");
    DeviceGuard guard;
    if (g.v4cfg.env_mode != PT_V4_ENV_NONE) {
        if (!tex) return fail(PT_EINVAL, "env mode %d needs a texture", g.v4cfg.env_mode);
        if ((rc = ensure_env(tex))) return rc;
    }
    PtV4Job j = v4_job(nullptr, w, h);
    j.layout = PT_LAYOUT_TILED_PLANAR8;   // RenderTile v4 :1186-1191
    j.tile_w = tw;
    j.tile_h = th;
    if ((rc = v4_use_env(j))) return rc;
    bool banded = false;   // PT_FLAG_PIN_HOST: bands of whole tile rows
    if ((rc = render_bands(buf, j, th, [](const PtV4Job& b) { return launch(g.dev[0], b, g.dev[0].stream, false); },
                           &banded)))
        return rc;
    const Geo geo = geo_of(w, h, PT_LAYOUT_TILED_PLANAR8, tw, th);
    bool presented = false;   // the render launch wrote the screen pixels (fused OutputToScreen)
    if (!banded) {
        if ((rc = stage_in(buf, geo, Region{}))) return rc;
        for (int d = 0; d < g.ndev; ++d) {
            PtV4Job jd = shard_job(j, d);
            // RenderTile + OutputToScreen in one pass, as the reference's worker does per tile (v4
            // :1562-1564): one device, the presenting configuration (pt_pick_v4_normalise decides)
            if (screen && g.v4cfg.output_to_screen && g.ndev == 1) {
                Dev& dv = g.dev[d];
                if ((rc = grow(dv, (void**)&dv.dtone_out, &dv.dtone_out_cap, (size_t)w * h * sizeof(uint32_t)))) return rc;
                jd.pix_out = dv.dtone_out;
                jd.pix_xrgb = 1;
                jd.pix_fast_tone = g.v4cfg.fast_aces && g.v4cfg.fast_gamma ? 1 : 0;
            }
            if ((rc = launch(g.dev[d], jd, g.dev[d].stream, false, nullptr, nullptr, &presented))) return rc;
        }
    }
    g.v4_frame += 1;   // iFrame += 1.0f (v4 :1703), before rendering
    if (screen && g.v4cfg.output_to_screen) {   // OutputToScreen per tile (v4 :1562-1564)
        if (presented) {
            Dev& dv = g.dev[0];
            HIP_TRY(hipMemcpyAsync(screen, dv.dtone_out, (size_t)w * h * sizeof(uint32_t), hipMemcpyDeviceToHost, dv.stream));
        } else if (banded) {
            Dev& dv = g.dev[0];
            const size_t out_bytes = (size_t)w * h * sizeof(uint32_t);
            if ((rc = grow(dv, (void**)&dv.dtone_out, &dv.dtone_out_cap, out_bytes))) return rc;
            const PtToneJob tj = tone_job(dv.dbuf, w, h, PT_LAYOUT_TILED_PLANAR8, tw, th, dv.dtone_out, PT_PIXEL_XRGB8);
            hipError_t e = pt_launch_tonemap(tj, dv.stream);
            if (e != hipSuccess) return fail(PT_EHIP, "tonemap launch failed: %s", hipGetErrorString(e));
            HIP_TRY(hipMemcpyAsync(screen, dv.dtone_out, out_bytes, hipMemcpyDeviceToHost, dv.stream));
        } else if ((rc = tone_output(PT_LAYOUT_TILED_PLANAR8, tw, th, (uint32_t*)screen, PT_PIXEL_XRGB8))) {
            return rc;
        }
    }
    if (banded) {
        HIP_TRY(hipStreamSynchronize(g.s_out));
        return sync_all();
    }
    return stage_out(buf, geo, Region{});
}

int pt_copy_output_to_file(const float* buf, int32_t w, int32_t h, int32_t ntx, int32_t nty, int32_t tw, int32_t th,
                           int32_t nc, void* file_pixels)
{
    int rc;
    if ((rc = check_frame_args(buf, w, h, nc)) || (rc = ensure_init())) return rc;
    if ((rc = tiled_settings(w, h, ntx, nty, tw, th))) return rc;
    if (g.v4_frame + 1u >= kMaxFrame) return fail(PT_EINVAL, "v4 frame counter exceeds the exact f32 range 2^24");
    if ((rc = pt_tonemap(buf, w, h, PT_LAYOUT_TILED_PLANAR8, tw, th, (uint32_t*)file_pixels, PT_PIXEL_RGBA8))) return rc;
    g.v4_frame += 1;   // v4 :1738
    return PT_OK;
}

static int v4_device_job(const pt_device_job* dj, PtV4Job* j4)
{
    int rc;
    if (!dj) return fail(PT_EINVAL, "null device job");
    pt_device_job geo = *dj;   // geometry / frame checks of the scalar-path jobs
    geo.use_env = 0;
    PtJob j;
    if ((rc = device_job(&geo, &j)) || (rc = v4_ensure_scene())) return rc;
    *j4 = v4_job(dj->buf, dj->width, dj->height);
    device_job_fields(j4, *dj);
    if (dj->use_env) {
        if (g.v4cfg.env_mode == PT_V4_ENV_NONE) return fail(PT_ESTATE, "use_env with v4 env mode NONE");
        if ((rc = v4_use_env(*j4))) return rc;
    }
    return PT_OK;
}

int pt_v4_render_device(const pt_device_job* dj, void* stream)
{
    int rc;
    PtV4Job j;
    Dev* dv = nullptr;
    DeviceGuard guard;
    if ((rc = ensure_init()) || (rc = v4_device_job(dj, &j)) || (rc = dev_of(dj->buf, &dv))) return rc;
    return launch(*dv, j, (hipStream_t)stream, false);
}

// pt_render_device_present for v4: the continuous-tiles kernel's presenting instances write the pixels
// with the accumulator (pt_pick_v4_normalise, pt_pick_v4_ct_takes); a launch that did not present -- fewer than 8 frames, the
// per-tile pool, sampling flags without a presenting instance, a tonemap pair other than the default
// fast ACES / gamma, nothing to render -- is followed by the stand-alone pass over the job's rows.
int pt_v4_render_device_present(const pt_device_job* dj, uint32_t* pixels, int32_t format, void* stream)
{
    int rc;
    PtV4Job j;
    Dev* dv = nullptr;
    DeviceGuard guard;
    if (!pixels) return fail(PT_EINVAL, "null pixel buffer");
    if (format != PT_PIXEL_RGBA8 && format != PT_PIXEL_XRGB8) return fail(PT_EINVAL, "unknown pixel format %d", format);
    if ((rc = ensure_init()) || (rc = v4_device_job(dj, &j)) || (rc = dev_of(dj->buf, &dv))) return rc;
    j.pix_out = pixels;
    j.pix_rows = 1;
    j.pix_xrgb = format == PT_PIXEL_XRGB8;
    j.pix_fast_tone = g.v4cfg.fast_aces && g.v4cfg.fast_gamma ? 1 : 0;
    bool presented = false;
    if ((rc = launch(*dv, j, (hipStream_t)stream, false, nullptr, nullptr, &presented)) || presented) return rc;
    const PtToneJob tj = tone_job(j.buf, j.ncols, j.nrows, j.layout, 0, 0, pixels, format);   // (the v4 config's flags)
    hipError_t e = pt_launch_tonemap(tj, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PT_EHIP, "tonemap launch failed: %s", hipGetErrorString(e));
    return PT_OK;
}

int pt_v4_render_device_chain(const pt_device_job* dj, void* stream)
{
    int rc;
    PtV4Job j;
    Dev* dv = nullptr;
    DeviceGuard guard;
    if ((rc = ensure_init()) || (rc = v4_device_job(dj, &j)) || (rc = dev_of(dj->buf, &dv))) return rc;
    return launch_chain(*dv, j, (hipStream_t)stream);
}

static_assert(sizeof(pt_v4_scene_desc) == sizeof(PtV4SceneDesc) && offsetof(pt_v4_scene_desc, quads) == offsetof(PtV4SceneDesc, quad) &&
              offsetof(pt_v4_scene_desc, spheres) == offsetof(PtV4SceneDesc, sphere) &&
              offsetof(pt_v4_scene_desc, materials) == offsetof(PtV4SceneDesc, mat) &&
              offsetof(pt_v4_scene_desc, nmaterials) == offsetof(PtV4SceneDesc, nmat),
              "pt_v4_scene_desc is PtV4SceneDesc");

int pt_v4_get_scene_desc(pt_v4_scene_desc* out)
{
    int rc;
    if (!out) return fail(PT_EINVAL, "null scene description");
    if ((rc = v4_ensure_scene())) return rc;
    memcpy(out, &g.v4desc, sizeof(*out));
    return PT_OK;
}

// The batched v4 launches (include/pt_mi355.h; pt_v4.h PtV4Views ... PtV4Frames).  The four public calls are
// one function: `kind` says which call it is, and the arguments travel as a pt_v4_batch (the views, scenes and
// envs calls fill one; they leave `frames` NULL and never read it).  What a kind reads, where that lies in the
// block of the device's batch ring (Dev::batch), every check -- all made before the first HIP call -- and the
// block's contents are pt_v4_batch.h's; here is the sequence around them.  The launch is a plain, unscheduled
// one of the kind's instances (pt_launch_v4_batched) -- it joins (ends) a live chain and takes a tile-queue ring
// slot like every plain launch, and touches no geometry's schedule state.  Of the process-wide scene, camera and
// frame counter only the scene is read, by a views launch (a kernel argument, g.v4scene) and by an envs or batch
// launch without `scenes`: the job is made from the arguments and the pt_v4_config alone.
//   `stats` (pt_v4_render_device_batch_stats; kBatch only): the same call, which also leaves each view's
//           statistics in `stats` -- cleared on the stream first, also when nothing renders.  Under the default
//           tonemap pair the batch kind's statistics instances compare as they store (pt_v4.h PtV4Stats); under
//           any other pair the old slices are packed into the slot's scratch before the render and the compare
//           pass (pt_output.h PtStatsJob) takes the place of the conversion pass.
using V4BatchKind = PtV4BatchKind;   // (pt_kernel_pick.h: kViews, kScenes, kEnvs, kBatch)

static_assert(sizeof(pt_v4_view_stats) == sizeof(PtV4ViewStats) && offsetof(pt_v4_view_stats, sum_delta) == offsetof(PtV4ViewStats, sum_delta) &&
                  offsetof(pt_v4_view_stats, changed) == offsetof(PtV4ViewStats, changed) &&
                  offsetof(pt_v4_view_stats, max_delta) == offsetof(PtV4ViewStats, max_delta),
              "pt_v4_view_stats is PtV4ViewStats");

// Nothing renders (every view has 0 frames, or no rows): the records are still cleared on the stream.
static int v4_stats_clear_only(const pt_device_job* dj, pt_v4_view_stats* stats, int32_t nviews, void* stream)
{
    int rc;
    Dev* dv = nullptr;
    DeviceGuard guard;
    if ((rc = ensure_init()) || (rc = dev_of(dj->buf, &dv)) || (rc = use_dev(*dv))) return rc;
    HIP_TRY(hipMemsetAsync(stats, 0, (size_t)nviews * sizeof(pt_v4_view_stats), (hipStream_t)stream));
    return PT_OK;
}

// The job of a batched launch: v4_device_job's without the process-wide camera (the views' records carry the
// cameras and the windows) -- the arguments and the config.
static int v4_batch_job(const pt_device_job& dj, const PtV4BatchShape& shape, PtV4Job* out)
{
    int rc;
    PtV4Job j{};
    j.buf = dj.buf;
    j.width = dj.width;
    j.height = dj.height;
    j.col0 = 0;
    j.ncols = dj.width;
    device_job_fields(&j, dj);
    j.env_mode = PT_V4_ENV_NONE;
    v4_config_fields(&j);
    j.sky = PtV4SkyWin{-1, {}};
    if (shape.env_set()) {
        j.env_mode = g.v4cfg.env_mode;   // (job.env, env_w, env_h stay null: the views' records carry the textures)
    } else if (shape.frames) {
        // use_env 0 or env mode NONE: the ambient; else pt_set_env_map's texture as the one record of a staged table
        if (dj.use_env && (rc = v4_use_env(j))) return rc;
    } else if (dj.use_env) {
        if (g.v4cfg.env_mode == PT_V4_ENV_NONE) return fail(PT_ESTATE, "use_env with v4 env mode NONE");
        if ((rc = v4_use_env(j))) return rc;
    }
    *out = j;
    return PT_OK;
}

// The next slot of the device's batch ring, free to be written: its previous launch (kViewRing launches back) has
// finished, its block holds `need` bytes and its statistics scratch `scratch_px` pixels (0: none wanted).  The
// ring's cursor advances whether or not the slot can be had.
static int batch_slot_acquire(Dev& dv, size_t need, size_t scratch_px, Dev::BatchSlot** out)
{
    Dev::BatchSlot& ss = dv.batch[dv.batch_next++ % kViewRing];
    if (!ss.done) HIP_TRY(hipEventCreateWithFlags(&ss.done, hipEventDisableTiming));
    if (ss.pending) {   // the slot's previous launch still reads the block: wait for it
        HIP_TRY(hipEventSynchronize(ss.done));
        ss.pending = false;
    }
    if (ss.cap < need) {   // (no launch reads the slot's block now)
        if (ss.host) (void)hipHostFree(ss.host);
        if (ss.dev) (void)hipFree(ss.dev);
        ss.host = ss.dev = nullptr;
        ss.cap = 0;
        const size_t cap = (need + 4095u) & ~(size_t)4095u;
        if (hipHostMalloc((void**)&ss.host, cap, hipHostMallocDefault) != hipSuccess) {
            ss.host = nullptr;
            return fail(PT_ENOMEM, "hipHostMalloc(batch block, %zu bytes) failed", cap);
        }
        if (hipMalloc((void**)&ss.dev, cap) != hipSuccess) {
            (void)hipHostFree(ss.host);
            ss.host = ss.dev = nullptr;
            return fail(PT_ENOMEM, "hipMalloc(batch block, %zu bytes) failed", cap);
        }
        ss.cap = cap;
    }
    if (ss.before_cap < scratch_px) {   // (likewise: no launch reads the slot's scratch now)
        if (ss.before) (void)hipFree(ss.before);
        ss.before = nullptr;
        ss.before_cap = 0;
        if (hipMalloc((void**)&ss.before, scratch_px * sizeof(uint32_t)) != hipSuccess) {
            ss.before = nullptr;
            return fail(PT_ENOMEM, "hipMalloc(batch statistics scratch, %zu bytes) failed", scratch_px * sizeof(uint32_t));
        }
        ss.before_cap = scratch_px;
    }
    *out = &ss;
    return PT_OK;
}

static int v4_batched_launch(const pt_device_job* dj, V4BatchKind kind, const pt_v4_batch& args, void* stream,
                             pt_v4_view_stats* stats = nullptr)
{
    int rc;
    const bool views = kind == V4BatchKind::kViews;
    const PtV4BatchShape shape = pt_v4_batch_shape(kind, args, dj ? dj->use_env : 0, g.v4cfg.env_mode);
    if (shape.current_scene && (rc = v4_ensure_scene())) return rc;   // (host only)
    const pt_v4_env_set* const envs = shape.env_set() ? args.envs : nullptr;
    const bool live = envs && env_set_live(envs);
    const PtV4BatchState state{g.v4cfg.env_mode, live, live ? envs->count : 0, &g.v4desc, v4_skywin_off()};
    std::vector<float> dist;
    bool nothing = false;
    if ((rc = pt_v4_batch_check(dj, shape, args, state, &dist, &nothing, fail))) return rc;
    const int32_t nviews = args.nviews, nscenes = pt_v4_batch_nscenes(shape, args);
    if (nothing) return stats ? v4_stats_clear_only(dj, stats, nviews, stream) : PT_OK;

    Dev* dvp = nullptr;
    DeviceGuard guard;
    PtV4Job j;
    if ((rc = ensure_init()) || (views && (rc = v4_ensure_scene())) || (rc = v4_batch_job(*dj, shape, &j))) return rc;
    if ((rc = dev_of(dj->buf, &dvp)) || (rc = use_dev(*dvp))) return rc;
    Dev& dv = *dvp;
    if (envs && envs->dev != dvp)
        return fail(PT_EINVAL, "the env set lives on device %d, the job's buffer on device %d", envs->dev->ordinal, dv.ordinal);
    hipStream_t st = (hipStream_t)stream;
    if (!envs && j.env_mode != PT_V4_ENV_NONE) j.env = dv.denv;
    j.err = dv.derr;
    // the render kernel writes the pixels with the default tonemap pair; any other pair: a second pass
    const bool fused = args.pixels && g.v4cfg.fast_aces && g.v4cfg.fast_gamma;
    j.pix_xrgb = args.format == PT_PIXEL_XRGB8;
    // and so with the statistics: compared in the render kernel, or (any other pair) around it
    const bool stats_fused = stats && g.v4cfg.fast_aces && g.v4cfg.fast_gamma, stats_pass = stats && !stats_fused;
    if (stats) HIP_TRY(hipMemsetAsync(stats, 0, (size_t)nviews * sizeof(pt_v4_view_stats), st));

    const PtV4BatchLayout lay = pt_v4_batch_layout(shape, nscenes, nviews);
    Dev::BatchSlot* ssp = nullptr;
    if ((rc = batch_slot_acquire(dv, lay.need, stats_pass ? (size_t)nviews * (size_t)dj->nrows * (size_t)dj->width : 0u, &ssp))) return rc;
    Dev::BatchSlot& ss = *ssp;
    if ((rc = pt_v4_batch_fill(ss.host, lay, shape, *dj, args, state, dist.data(), PtV4EnvRec{dv.denv, j.env_w, j.env_h}, fail))) return rc;
    HIP_TRY(hipMemcpyAsync(ss.dev, ss.host, lay.need, hipMemcpyHostToDevice, st));

    LaunchSched ls;
    if ((rc = chain_join(dv, st)) || (rc = use_queue_slot(dv, st, &ls))) return rc;
    j.queue = ls.queue;
    j.queue_next = ls.queue_next;
    const PtV4Views va{pt_v4_batch_views(ss.dev, lay), nviews, fused ? args.pixels : nullptr, g.v4_views_grid};
    const PtV4Scenes sa{pt_v4_batch_scenes(ss.dev, lay), nscenes, pt_v4_batch_scene_map(ss.dev, lay)};
    const int32_t* const emap = pt_v4_batch_env_map(ss.dev, lay);
    const PtV4Envs ea = envs               ? PtV4Envs{envs->table, envs->count, emap}
                        : shape.staged_env ? PtV4Envs{pt_v4_batch_env_rec(ss.dev, lay), 1, emap}
                                           : PtV4Envs{nullptr, 0, nullptr};
    const PtV4Frames fa{pt_v4_batch_frames(ss.dev, lay)};
    hipError_t e;
    if (stats_pass) {
        // the old slices as the display would show them, before the render overwrites them (after chain_join: a
        // live chain's last launch may still write them).  The slices lie back to back: one image.
        e = pt_launch_tonemap(tone_job(j.buf, j.ncols, j.nrows * nviews, j.layout, 0, 0, ss.before, PT_PIXEL_XRGB8), st);
        if (e != hipSuccess) return fail(PT_EHIP, "tonemap launch failed: %s", hipGetErrorString(e));
    }
    const PtV4Stats sta{reinterpret_cast<PtV4ViewStats*>(stats)};
    // (what the kind does not read is not passed; a views launch renders the process-wide scene)
    e = pt_launch_v4_batched(kind, j, views ? &g.v4scene : nullptr, va, views ? nullptr : &sa, ea.table ? &ea : nullptr,
                             shape.frames ? &fa : nullptr, st, stats_fused ? &sta : nullptr);
    if (e != hipSuccess) {
        static const char* const name[] = {"views", "scenes", "envs", "batch"};   // (PtV4BatchKind's order)
        return fail(PT_EHIP, "v4 %s launch failed: %s", name[(int)kind], hipGetErrorString(e));
    }
    HIP_TRY(hipEventRecord(ss.done, st));
    ss.pending = true;
    if ((rc = queue_done(dv, ls.slot, st, true))) return rc;
    if (stats_pass) {
        // the new slices against the scratch, per view; it writes the pixels too, so no conversion pass follows
        PtStatsJob sj{};
        sj.tone = tone_job(j.buf, j.ncols, j.nrows, j.layout, 0, 0, args.pixels, args.format);
        sj.nviews = nviews;
        sj.before = ss.before;
        sj.ranges = fa.range_of_view;
        sj.stats = sta.of_view;
        sj.err = j.err;
        e = pt_launch_tonemap_stats(sj, st);
        if (e != hipSuccess) return fail(PT_EHIP, "statistics pass launch failed: %s", hipGetErrorString(e));
        HIP_TRY(hipEventRecord(ss.done, st));   // (again: the pass reads the slot's ranges and scratch)
    } else if (args.pixels && !fused) {
        // (the slices lie back to back: one image of nviews x nrows rows in either row layout)
        const PtToneJob tj = tone_job(j.buf, j.ncols, j.nrows * nviews, j.layout, 0, 0, args.pixels, args.format);
        e = pt_launch_tonemap(tj, st);
        if (e != hipSuccess) return fail(PT_EHIP, "tonemap launch failed: %s", hipGetErrorString(e));
    }
    return PT_OK;
}
int pt_v4_render_device_views(const pt_device_job* dj, const pt_v4_camera* cams, int32_t nviews, uint32_t* pixels,
                              int32_t format, void* stream)
{
    pt_v4_batch a{};
    a.cams = cams;
    a.nviews = nviews;
    a.pixels = pixels;
    a.format = format;
    return v4_batched_launch(dj, V4BatchKind::kViews, a, stream);
}

int pt_v4_render_device_scenes(const pt_device_job* dj, const pt_v4_scene_desc* scenes, int32_t nscenes, const pt_v4_camera* cams,
                               const int32_t* scene_of_view, int32_t nviews, uint32_t* pixels, int32_t format, void* stream)
{
    pt_v4_batch a{};
    a.cams = cams;
    a.nviews = nviews;
    a.scenes = scenes;
    a.nscenes = nscenes;
    a.scene_of_view = scene_of_view;
    a.pixels = pixels;
    a.format = format;
    return v4_batched_launch(dj, V4BatchKind::kScenes, a, stream);
}

int pt_v4_render_device_envs(const pt_device_job* dj, const pt_v4_env_set* envs, const int32_t* env_of_view,
                             const pt_v4_scene_desc* scenes, int32_t nscenes, const int32_t* scene_of_view, const pt_v4_camera* cams,
                             int32_t nviews, uint32_t* pixels, int32_t format, void* stream)
{
    pt_v4_batch a{};
    a.cams = cams;
    a.nviews = nviews;
    a.scenes = scenes;
    a.nscenes = nscenes;
    a.scene_of_view = scene_of_view;
    a.envs = envs;
    a.env_of_view = env_of_view;
    a.pixels = pixels;
    a.format = format;
    return v4_batched_launch(dj, V4BatchKind::kEnvs, a, stream);
}

static_assert(sizeof(pt_v4_frame_range) == sizeof(PtV4FrameRange) && offsetof(pt_v4_frame_range, nframes) == offsetof(PtV4FrameRange, nframes),
              "pt_v4_frame_range is PtV4FrameRange");

int pt_v4_render_device_batch(const pt_device_job* dj, const pt_v4_batch* b, void* stream)
{
    if (!b) return fail(PT_EINVAL, "null batch");
    return v4_batched_launch(dj, V4BatchKind::kBatch, *b, stream);
}

int pt_v4_render_device_batch_stats(const pt_device_job* dj, const pt_v4_batch* b, pt_v4_view_stats* stats, void* stream)
{
    if (!b) return fail(PT_EINVAL, "null batch");
    if (!stats) return fail(PT_EINVAL, "null statistics buffer");
    return v4_batched_launch(dj, V4BatchKind::kBatch, *b, stream, stats);
}

int pt_v4_count_device(const pt_device_job* dj, void* stream, pt_work_counts* out)
{
    int rc;
    PtV4Job j;
    Dev* dv = nullptr;
    DeviceGuard guard;
    if (!out) return fail(PT_EINVAL, "null counts");
    if ((rc = ensure_init()) || (rc = v4_device_job(dj, &j)) || (rc = dev_of(dj->buf, &dv)) || (rc = use_dev(*dv))) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(dv->dcounters, 0, kCounterSlots * sizeof(unsigned long long), st));
    j.counters = dv->dcounters;
    if ((rc = launch(*dv, j, st, true))) return rc;
    unsigned long long h[6];
    HIP_TRY(hipMemcpyAsync(h, dv->dcounters, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out->segments = h[0];
    out->lane_slots = h[3];
    out->samples = (uint64_t)dj->width * (uint64_t)dj->nrows * (uint64_t)dj->nframes;
    out->escaped = h[2];
    out->primary = out->samples;   // one camera ray per sample (jittered)
    out->quad_fallbacks = 0;
    out->sphere_fallbacks = h[4];
    out->sky_skipped = h[5];
    return PT_OK;
}

int pt_v4_begin_frame(void)
{
    if (g.v4_frame + 1u >= kMaxFrame) return fail(PT_EINVAL, "v4 frame counter exceeds the exact f32 range 2^24");
    g.v4_frame += 1;
    return PT_OK;
}

// ---- tile work queue ------------------------------------------------------------------------------

}  // extern "C"

struct pt_work_queue {
    int32_t renderer = PT_RENDERER_SIMD_TILED;
    std::vector<std::pair<pt_buffer_info, pt_tile_info>> entries;
    bool pending = false;   // an async completion not yet waited for
};

namespace {

// Render the queued entries: per buffer (in first-use order) either one full-frame launch per device
// (the entries are exactly the buffer's NTX x NTY tiles) or per tile one launch per device; uploads /
// downloads of only what is rendered.  Everything is enqueued on the device streams; `wait`
// synchronises at the end.
int run_queue(pt_work_queue* q, bool wait)
{
    int rc;
    if ((rc = ensure_init())) return rc;
    const bool v4 = q->renderer == PT_RENDERER_V4;
    if (v4) {
        if (g.v4_frame < 1) return fail(PT_ESTATE, "v4 work queue before the first frame (pt_v4_begin_frame)");
        if ((rc = v4_ensure_scene())) return rc;
    } else if (g.frame < (uint32_t)g.cfg.samples_per_frame) {
        return fail(PT_ESTATE, "work queue before the first frame was started (pt_begin_frame)");
    }
    const bool env = q->renderer == PT_RENDERER_SIMT_TEXTURED;
    if (env && !g.have_env) return fail(PT_ESTATE, "textured work queue without an env map (pt_set_env_map)");
    DeviceGuard guard;
    Dev& d0 = g.dev[0];
    std::vector<bool> done(q->entries.size(), false);
    for (size_t i = 0; i < q->entries.size(); ++i) {
        if (done[i]) continue;
        const pt_buffer_info& b = q->entries[i].first;
        std::vector<size_t> mine;
        for (size_t k = i; k < q->entries.size(); ++k)
            if (!done[k] && q->entries[k].first.data == b.data) {
                const pt_buffer_info& bk = q->entries[k].first;
                if (bk.width != b.width || bk.height != b.height)
                    return fail(PT_EINVAL, "entries of one buffer disagree on its size");
                mine.push_back(k);
                done[k] = true;
            }
        const pt_tile_info& t0 = q->entries[mine[0]].second;
        const int32_t tw = t0.tile_width, th = t0.tile_height;
        for (size_t k : mine) {
            const pt_tile_info& t = q->entries[k].second;
            if (t.tile_width != tw || t.tile_height != th)
                return fail(PT_EINVAL, "entries of one buffer disagree on the tile size");
        }
        bool full = b.width % tw == 0 && b.height % th == 0 &&
                    mine.size() == (size_t)(b.width / tw) * (size_t)(b.height / th);
        if (full) {   // exactly every tile once?
            std::vector<char> seen((size_t)(b.width / tw) * (b.height / th), 0);
            for (size_t k : mine) {
                const pt_tile_info& t = q->entries[k].second;
                const size_t id = (size_t)t.tile_y * (b.width / tw) + t.tile_x;
                if (seen[id]) {
                    full = false;
                    break;
                }
                seen[id] = 1;
            }
        }
        const Geo geo = geo_of(b.width, b.height, PT_LAYOUT_TILED_PLANAR8, tw, th);
        if (full && g.ndev == 1 && (g.cfg.flags & PT_FLAG_PIN_HOST) && !(g.cfg.flags & PT_FLAG_DEFER_READBACK)) {
            // A whole frame of tiles with PT_FLAG_PIN_HOST: the frame calls' band pipeline (bands of
            // whole tile rows, upload / render / download overlapped on three streams).  The bands'
            // copies run on s_in / s_out, so they are ordered after the work already queued on
            // the device stream (an earlier buffer's download from the mirror), and that stream --
            // which the completion calls synchronise -- after the last download.
            if ((rc = use_dev(d0))) return rc;
            HIP_TRY(hipEventRecord(g.ev_q, d0.stream));
            HIP_TRY(hipStreamWaitEvent(g.s_in, g.ev_q, 0));
            bool banded = false;
            if (v4) {
                PtV4Job j = v4_job(nullptr, b.width, b.height);
                j.layout = PT_LAYOUT_TILED_PLANAR8;
                j.tile_w = tw;
                j.tile_h = th;
                j.frame_first = g.v4_frame;
                if ((rc = v4_use_env(j))) return rc;
                rc = render_bands(b.data, j, th, [](const PtV4Job& bj) { return launch(g.dev[0], bj, g.dev[0].stream, false); },
                                  &banded);
            } else {
                pt_tile_info t = t0;
                t.tile_min_x = 0;
                t.tile_min_y = 0;
                PtJob j = tile_job(&b, &t, env);
                j.ncols = b.width;
                j.nrows = b.height;
                if (env)
                    rc = render_bands(b.data, j, th, [](const PtJob& bj) {
                        return launch(g.dev[0], with_env(bj, g.dev[0], true), g.dev[0].stream, false);
                    }, &banded);
                else
                    rc = render_bands(b.data, j, th, [](const PtJob& bj) { return launch(g.dev[0], bj, g.dev[0].stream, false); },
                                      &banded);
            }
            if (rc) return rc;
            if (banded) {
                HIP_TRY(hipEventRecord(g.ev_q, g.s_out));
                HIP_TRY(hipStreamWaitEvent(d0.stream, g.ev_q, 0));
                continue;
            }
        }
        // one job per device for the whole frame, or per tile
        std::vector<Region> regions;
        if (full) {
            regions.push_back(Region{});
        } else {
            for (size_t k : mine) {
                Region rg;
                rg.whole = false;
                rg.tile_x = q->entries[k].second.tile_x;
                rg.tile_y = q->entries[k].second.tile_y;
                regions.push_back(rg);
            }
        }
        for (const Region& rg : regions)
            if ((rc = stage_in(b.data, geo, rg))) return rc;
        for (const Region& rg : regions) {
            // the frame as one "tile" region in the tiled layout, or the entry's tile
            const int32_t col0 = rg.whole ? 0 : rg.tile_x * tw, row0 = rg.whole ? 0 : rg.tile_y * th;
            const int32_t ncols = rg.whole ? b.width : tw, nrows = rg.whole ? b.height : th;
            for (int d = 0; d < g.ndev; ++d) {
                Dev& dv = g.dev[d];
                if (v4) {
                    PtV4Job j = v4_job(nullptr, b.width, b.height);
                    j.layout = PT_LAYOUT_TILED_PLANAR8;
                    j.tile_w = tw;
                    j.tile_h = th;
                    j.col0 = col0;
                    j.ncols = ncols;
                    j.row_start = row0;
                    j.nrows = nrows;
                    j.frame_first = g.v4_frame;   // the frame pt_v4_begin_frame started
                    if ((rc = v4_use_env(j)) || (rc = launch(dv, tile_shard_job(j, d), dv.stream, false))) return rc;
                } else {
                    pt_tile_info t{};
                    t.tile_width = tw;
                    t.tile_height = th;
                    t.tile_min_x = col0;
                    t.tile_min_y = row0;
                    PtJob j = tile_job(&b, &t, env);
                    j.ncols = ncols;
                    j.nrows = nrows;
                    if ((rc = launch(dv, with_env(tile_shard_job(j, d), dv, env), dv.stream, false))) return rc;
                }
            }
        }
        if (!(g.cfg.flags & PT_FLAG_DEFER_READBACK))
            for (const Region& rg : regions)
                for (int d = 0; d < g.ndev; ++d)
                    if ((rc = use_dev(g.dev[d])) || (rc = xfer(d, geo, b.data, false, rg))) return rc;
        // the mirror holds one buffer at a time: another buffer of the queue must not start
        // overwriting it before this one's downloads are done (stream order guarantees that)
    }
    q->entries.clear();
    if (wait) {
        if ((rc = sync_all())) return rc;
        q->pending = false;
    } else {
        q->pending = true;
    }
    return PT_OK;
}

}  // namespace

extern "C" {

pt_work_queue* pt_make_work_queue(int32_t renderer)
{
    if (renderer < PT_RENDERER_SIMD_TILED || renderer > PT_RENDERER_V4) {
        fail(PT_EINVAL, "unknown renderer %d", renderer);
        return nullptr;
    }
    pt_work_queue* q = new (std::nothrow) pt_work_queue;
    if (!q) {
        fail(PT_ENOMEM, "out of host memory");
        return nullptr;
    }
    q->renderer = renderer;
    q->entries.reserve(1024);   // WORK_QUEUE_MAX_ENTRIES (work_queue.h:16)
    return q;
}

int pt_add_work_queue_entry(pt_work_queue* q, const pt_buffer_info* b, const pt_tile_info* t)
{
    int rc;
    if (!q) return fail(PT_EINVAL, "null queue");
    if ((rc = check_tile(b, t))) return rc;
    if (q->entries.size() >= 1023)   // the ring holds MaxEntryCount - 1 (work_queue.cpp:42 assert)
        return fail(PT_EINVAL, "work queue full (WORK_QUEUE_MAX_ENTRIES 1024)");
    q->entries.emplace_back(*b, *t);
    return PT_OK;
}

int pt_complete_all_work(pt_work_queue* q)
{
    if (!q) return fail(PT_EINVAL, "null queue");
    return run_queue(q, true);
}

int pt_complete_all_work_async(pt_work_queue* q)
{
    if (!q) return fail(PT_EINVAL, "null queue");
    return run_queue(q, false);
}

int pt_wait_work(pt_work_queue* q)
{
    if (!q) return fail(PT_EINVAL, "null queue");
    if (q->pending && g.inited) {
        DeviceGuard guard;
        int rc;
        if ((rc = sync_all())) return rc;
    }
    q->pending = false;
    return PT_OK;
}

int32_t pt_work_queue_size(const pt_work_queue* q) { return q ? (int32_t)q->entries.size() : 0; }

void pt_free_work_queue(pt_work_queue* q)
{
    if (!q) return;
    if (q->pending && g.inited) {
        DeviceGuard guard;
        (void)sync_all();
    }
    delete q;
}

}  // extern "C"
