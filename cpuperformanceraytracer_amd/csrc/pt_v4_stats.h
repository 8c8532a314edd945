// pt_v4_stats.h -- per-view convergence statistics of a v4 batch (pt_v4_render_device_batch_stats): what one
// pixel contributes and how a wave's sums reach the view's record.  Shared by the render kernel's statistics
// form (pt_v4.hip pt_v4_batch_stats_kernel, the default tonemap pair) and the compare pass (pt_output.hip
// pt_tonemap_stats_kernel, any other pair), so both routes count the same thing.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_v4.h"   // PtV4ViewStats

// One pixel: `before` and `after` are packed with xrgb (0x00RRGGBB, pt_tonemap.h) whatever the caller's pixel
// format, so the result does not depend on it and the top byte never counts.  Returns the sum of the three
// channels' |after - before| (<= 765) in bits 0..15 and the largest of them (<= 255) in bits 16..23: zero
// exactly when R, G and B are all equal.
__device__ __forceinline__ uint32_t v4_stats_delta(uint32_t before, uint32_t after)
{
    const int dr = abs((int)((after >> 16) & 255u) - (int)((before >> 16) & 255u));
    const int dg = abs((int)((after >> 8) & 255u) - (int)((before >> 8) & 255u));
    const int db = abs((int)(after & 255u) - (int)(before & 255u));
    return (uint32_t)(dr + dg + db) | ((uint32_t)max(dr, max(dg, db)) << 16);
}

// A wave's 64 such values (0 for a lane without a pixel) reduced to one of the same form: the sums added
// (64 x 765 < 2^16, so the fields never meet), the maxima maximised -- ONE register travels through the six
// butterfly steps and every lane ends with the wave's value.  Integers only: the order does not matter.
__device__ __forceinline__ uint32_t v4_stats_wave(uint32_t d)
{
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)d, off);
        d = ((d & 0xffffu) + (o & 0xffffu)) | (max(d >> 16, o >> 16) << 16);
    }
    return d;
}

// One lane of the wave: the three atomics on the view's record (add, add, max; no value returned).
__device__ __forceinline__ void v4_stats_commit(PtV4ViewStats* rec, unsigned long long sum, uint32_t changed, uint32_t mx)
{
    atomicAdd(&rec->sum_delta, sum);
    atomicAdd(&rec->changed, changed);
    atomicMax(&rec->max_delta, mx);
}
