// pt_output.h -- internal interface of the output-stage kernel (pt_output.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pt_kernel.h"

#include "../../include/pt_mi355.h"   // PT_PIXEL_RGBA8 / PT_PIXEL_XRGB8

struct PtToneJob {
    const float* accum;       // device accumulator (PtLayout)
    int32_t width, height;
    int32_t layout;
    int32_t tile_w, tile_h;   // PT_LAYOUT_TILED_PLANAR8
    uint32_t* out;            // device, width * height packed pixels, row 0 = top
    int32_t format;           // PT_PIXEL_*
    int32_t fast_aces;        // USE_FAST_APPROXIMATE_ACES_TONEMAP (else the unfused fit with '/')
    int32_t fast_gamma;       // USE_FAST_APPROXIMATE_GAMMA (else 1.055 powf(x, 1/2.4) - 0.055)
};

hipError_t pt_launch_tonemap(const PtToneJob& job, hipStream_t stream);

// ---- per-view statistics of a v4 batch, the second-pass route (pt_v4_render_device_batch_stats) ----
// The render kernel compares as it stores only under the default tonemap pair.  Any other pair: before the
// render the old slices are packed into scratch (pt_launch_tonemap itself, format XRGB8 -- the slices lie back
// to back, one image of nviews x nrows rows); after it this pass packs the new values with the same pair,
// compares the R, G, B bytes with the scratch and adds each wave's sums to its view's record (pt_v4.h
// PtV4ViewStats: integer atomics add, add, max) -- and writes the pixels in `format` when `out` is given, in
// place of the conversion pass.  Views of 0 frames are not compared (their record stays zero); their pixels
// are still written.  Row layouts only.
struct PtV4ViewStats;
struct PtV4FrameRange;
struct PtStatsJob {
    PtToneJob tone;                  // accum, width, layout, the pair; height = nrows of ONE view; out / format: the
                                     // pixels (nviews x nrows x width) or nullptr
    int32_t nviews;
    const uint32_t* before;          // nviews x nrows x width, 0x00RRGGBB of the old slices
    const PtV4FrameRange* ranges;    // device memory, one record per view (nframes > 0: compared)
    PtV4ViewStats* stats;            // device memory, nviews records, cleared by the caller
    uint32_t* err;                   // the job's error words (pt_guard.h), nullptr = not recorded
};
hipError_t pt_launch_tonemap_stats(const PtStatsJob& job, hipStream_t stream);

// Several devices, PT_FLAG_GATHER_ROOT: device `dev` of `ndev` writes the global rows it owns
// (Y = dev + k * ndev) from its mirror into the root device's full-size accumulator -- remote stores
// over xGMI (peer access), each device over its own link.  Row layouts: the mirror holds the rows
// compactly; tiled layout: the mirror is full-size (same offsets as the root's).
struct PtScatterJob {
    const float* src;         // this device's mirror
    float* dst;               // the root's W x H x 3 buffer
    int32_t width, height;
    int32_t layout;
    int32_t tile_w, tile_h;   // PT_LAYOUT_TILED_PLANAR8
    int32_t dev, ndev, nrows; // owned rows
};

hipError_t pt_launch_scatter_rows(const PtScatterJob& job, hipStream_t stream);
