// keyframe_render_dev.h — a keyframe map rendered into a view (include/hnet.h hnet_op_keyframe_render, hnet_sessions_keyframe_render): what
// capi_keyframe_render.hip, keyframes_internal.h and kernels_keyframe_render.hip share.  The device compiles include/hnet_keyframe_render.h itself (host +
// device functions): render_setup, render_sample, render_pixel and seam_add are the functions tests/test_keyframe_render_rule.py pins on the host.
#pragma once
#include "keyframe_map_dev.h"

#pragma clang force_cuda_host_device begin
#include "../../include/hnet_keyframe_render.h"
#pragma clang force_cuda_host_device end

namespace hnet {

using RenderOpts = hnet_keyframe_render::Opts;       // = hnet_keyframe_render_opts
using RenderRec = hnet_keyframe_render::Record;      // = hnet_keyframe_render_rec
constexpr int RENDER_MAX = hnet_keyframe_render::MAX_ENTRIES;
// One slot's table, written by the setup and read by the render with scalar loads (it is uniform over a workgroup): per entry S (view pixel ->
// keyframe position), links and serial, and the mask of the entries that take part
struct RenderTab { double S[RENDER_MAX][9]; int32_t links[RENDER_MAX], serial[RENDER_MAX]; int32_t used_mask, pad; };
static_assert(sizeof(RenderOpts) == 16 && sizeof(RenderRec) == 224 && sizeof(RenderTab) == 648 && sizeof(hnet_keyframe_render::Counters) == 144, "packed layouts");

// The tile of one workgroup of the render: 64 x 16 pixels, a row of 64 per wavefront and step (kernels_keyframe_render.hip)
constexpr int RENDER_TILE_W = 64, RENDER_TILE_H = 16;

// What is rendered: the entries [n_sessions][capacity] and images [n_sessions][capacity][NPIX] of a map (capacity 1 .. 8; the operator-level call is one
// session of m entries), and, for a call without views, the sessions' states
struct RenderSource { const uint8_t* img; const MapEntry* entry; const KeyState* state; int n_sessions, capacity; };

// One wavefront per slot b < n (ids [n]: the sessions): lane j < capacity runs render_setup of entry j against the slot's view - views[b] [9], or with
// views null hnet_keyframe_map::origin_curr of the session's state - into tab[b]; rec[b] gets the view, used_mask and skipped_mask and zero counters
// (every byte written).  An id outside the table: no entry takes part, the view is written as given (identity without one), skipped_mask = 0.
hipError_t launch_keyframe_render_setup(const int32_t* ids, int n, const RenderSource& src, const double* views, RenderTab* tab, RenderRec* rec, hipStream_t s);
// Grid (tiles, n), 256 lanes: out_img [n][height][width] and out_cover [n][height][width] written in full, the counters of rec[b] advanced by one
// 64-bit atomic add per non-zero counter and workgroup
hipError_t launch_keyframe_render(const int32_t* ids, int n, const RenderSource& src, const RenderTab* tab, const RenderOpts& opts, uint8_t* out_img,
                                  uint8_t* out_cover, RenderRec* rec, hipStream_t s);

}  // namespace hnet
