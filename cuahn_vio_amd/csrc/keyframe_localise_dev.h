// keyframe_localise_dev.h — a camera localised against its rendered keyframe map (include/hnet.h hnet_op_keyframe_localise): what
// capi_keyframe_localise.hip and kernels_keyframe_localise.hip share.  The device compiles include/hnet_keyframe_localise.h itself (host + device
// functions): start and decide_localise are the functions tests/test_keyframe_localise_cpu.py pins on the host.
#pragma once
#include "keyframe_render_dev.h"
#include "photo_masked_dev.h"

#pragma clang force_cuda_host_device begin
#include "../../include/hnet_keyframe_localise.h"
#pragma clang force_cuda_host_device end

namespace hnet {

using LocaliseOpts = hnet_localise::Opts;      // = hnet_keyframe_localise_opts
using LocaliseRec = hnet_localise::Localise;   // = hnet_keyframe_localise
static_assert(sizeof(LocaliseOpts) == 104 && sizeof(LocaliseRec) == 1808, "packed layouts");

// x0 [n][8] <- hnet_localise::start of the render records rrec [n] (used_mask and n_covered: after the render launch)
hipError_t launch_keyframe_localise_start(const RenderRec* rrec, int n, const LocaliseOpts& opts, float* x0, hipStream_t s);
// The sessions form, after launch_keyframe_render_setup with null views: tab[b].used_mask and rrec[b].used_mask <- set-up AND eligible
// (hnet_localise::eligible_mask of the session's map state; an id outside the table keeps its empty mask)
hipError_t launch_keyframe_localise_eligible(const int32_t* ids, int n, const MapStore& map, RenderTab* tab, RenderRec* rrec, hipStream_t s);
// curr[b] <- ring[slot[b]] for slot[b] in 0 .. n_slots - 1 (nothing copied otherwise: the slot's start is quiet NaNs then, whatever the render said), a uint4 per
// lane, and x0 [n][8] as launch_keyframe_localise_start
hipError_t launch_keyframe_localise_gather(const int32_t* slot, int n, const uint8_t* ring, int n_slots, const RenderRec* rrec, const LocaliseOpts& opts,
                                           uint8_t* curr, float* x0, hipStream_t s);
// One wavefront per slot b < n: the lanes copy the level-0 alignment record arec[b] into out[b].rec - zeros when nothing was aligned - and lane 0 runs
// decide_localise on the render record's view, used_mask and n_covered.  ids == nullptr, the operator-level form: the entries of slot b are
// map.entry + b capacity and there is no state.  Otherwise the session ids[b]'s state, map state and entries, rewritten in place when opts.apply and the
// verdict say so; an id outside the table: no state is read or written and the verdict is NO_MAP.  Every byte of out[b] is written.
hipError_t launch_keyframe_localise_decide(const int32_t* ids, int n, const RenderRec* rrec, const RobustRec* arec, KeyState* state, const MapStore& map,
                                           const LocaliseOpts& opts, LocaliseRec* out, hipStream_t s);

}  // namespace hnet
