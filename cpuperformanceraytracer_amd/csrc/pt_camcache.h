// pt_camcache.h -- the camera-hit cache's record format, modes and size rule (PtJob::cam_cache in
// pt_kernel.h, Sched::cam in pt_capi.cpp).  Plain C++ without HIP: the kernels, the host
// layer and the host check (tests/native/check_camcache.cpp) share it.
#pragma once
#include <stddef.h>
#include <stdint.h>

enum PtCamMode : uint32_t {
    PT_CAM_NONE = 0,   // trace the camera rays
    PT_CAM_FILL = 1,   // trace them and store the records
    PT_CAM_USE = 2,    // load the records of a completed PT_CAM_FILL launch instead of tracing
};

// A record: the hit distance's f32 bits in the high word; the primitive (kCamMiss: none), the flag and
// the quad fallback bit in the low word.  An all-ones record (the buffer's initial state) is a miss.
constexpr uint32_t kCamMiss = 0xffu;
constexpr unsigned long long pt_cam_pack(uint32_t best_bits, int32_t id, int32_t flag, int32_t fb)
{
    return ((unsigned long long)best_bits << 32) | (uint32_t)(id < 0 ? kCamMiss : (uint32_t)id & 0xffu) |
           (flag ? 0x100u : 0u) | (fb ? 0x200u : 0u);
}
constexpr uint32_t pt_cam_best_bits(unsigned long long r) { return (uint32_t)(r >> 32); }
constexpr int32_t pt_cam_id(unsigned long long r)
{
    return ((uint32_t)r & 0xffu) == kCamMiss ? -1 : (int32_t)((uint32_t)r & 0xffu);
}
constexpr int32_t pt_cam_flag(unsigned long long r) { return (int32_t)(((uint32_t)r >> 8) & 1u); }
constexpr int32_t pt_cam_fb(unsigned long long r) { return (int32_t)(((uint32_t)r >> 9) & 1u); }

// The largest cache a geometry gets: 128 MiB holds 3840 x 2160 (66 MB) and anything up to 16.7 Mpixel;
// 7680 x 4320 (265 MB) runs without one.  A device keeps at most 16 geometries (pt_capi.cpp
// kSchedSlots), so the caches stay below 2 GiB, under 1 % of the MI355X's HBM.
constexpr size_t kCamCacheMaxBytes = (size_t)128 << 20;
constexpr size_t pt_cam_cache_bytes(uint32_t ntiles) { return (size_t)ntiles * 64u * sizeof(unsigned long long); }
constexpr bool pt_cam_cache_fits(uint32_t ntiles) { return pt_cam_cache_bytes(ntiles) <= kCamCacheMaxBytes; }
// Whether a geometry gets a cache: the diffuse kernels only (schedule kind 0; v4's camera rays are
// jittered), unless switched off (PT_MI355_CAM_CACHE=0) or larger than the cap.
constexpr bool pt_cam_cache_wanted(bool enabled, int32_t kind, uint32_t ntiles)
{
    return enabled && kind == 0 && pt_cam_cache_fits(ntiles);
}
