// keyframe_map_dev.h — a map of keyframes per session and the revisit against it (include/hnet.h hnet_sessions_enable_keyframe_map,
// hnet_sessions_keyframe_revisit): what capi_keyframe.hip and kernels_keyframe_map.hip share.  The device compiles
// include/hnet_keyframe_map.h itself (host + device functions): note, relative, grid_inside, offer and decide_revisit are the functions
// tests/test_keyframe_map_cpu.py pins on the host.
#pragma once
#include "keyframe_dev.h"

#pragma clang force_cuda_host_device begin
#include "../../include/hnet_keyframe_map.h"
#pragma clang force_cuda_host_device end

namespace hnet {

using MapEntry = hnet_keyframe_map::Entry;       // = hnet_keyframe_map_entry; the table is [N][M]
using MapState = hnet_keyframe_map::MapState;    // = hnet_keyframe_map_state; [N]
using MapRevisit = hnet_keyframe_map::Revisit;   // = hnet_keyframe_revisit
using MapOpts = hnet_keyframe_map::Opts;         // = hnet_keyframe_revisit_opts
static_assert(sizeof(MapEntry) == 88 && sizeof(MapState) == 16 && sizeof(MapRevisit) == sizeof(RobustRec) + 304 && sizeof(MapOpts) == sizeof(RobustOpts) + 32,
              "packed layouts");

// The map of N sessions with M slots each: images [N][M][NPIX], entries [N][M], states [N]
struct MapStore { uint8_t* img; MapEntry* entry; MapState* state; int n_sessions, capacity; };

// ---- after a track's commit (ids: the track's table).  One wavefront per slot b < n, lane 0: hnet_keyframe_map::note on the record's flags, copy[b] and
// the session's new state -> store[b] (the slot the new keyframe goes to, or -1; -1 for an id outside the table)
hipError_t launch_keyframe_map_note(const int32_t* ids, int n, const KeyTrack* out, const int32_t* copy, const KeyState* state, const MapStore& map, int32_t* store,
                                    hipStream_t s);
// img[ids[b]][store[b]] <- curr[b]; the commit's grid, workgroups of slots with store[b] outside 0 .. M-1 return at once
hipError_t launch_keyframe_map_store(const int32_t* ids, int n, const int32_t* store, const uint8_t* curr, const MapStore& map, hipStream_t s);

// ---- a revisit (ids, slot: the call's table {ids [n] | curr ring slot [n]}).  One wavefront per slot: h_origin_curr from the state, relative for each of
// the M entries uniformly, lane i tests grid point i and the count is one ballot; lane 0 keeps the best -> x0[b] (quiet NaNs without a candidate),
// cand[b], and out[b].grid / out[b].h_origin_before for the decide
hipError_t launch_keyframe_map_select(const int32_t* ids, int n, const KeyState* state, const MapStore& map, int min_grid, float* x0, int32_t* cand, MapRevisit* out,
                                      hipStream_t s);
// prev[b] <- img[ids[b]][cand[b]], curr[b] <- ring slot; slots without a candidate return at once (their start is NaN and the alignment returns on it)
hipError_t launch_keyframe_map_gather(const int32_t* ids, const int32_t* slot, int n, const int32_t* cand, const MapStore& map, const uint8_t* ring, int n_slots,
                                      uint8_t* prev, uint8_t* curr, hipStream_t s);
// One wavefront per slot, after the alignment (rec: the level-0 records [n]): the lanes copy the record (zeros without a candidate), lane 0 runs
// hnet_keyframe_map::decide_revisit in place on the session's state and map state -> out[b] (every byte written) and attach[b]
hipError_t launch_keyframe_map_decide(const int32_t* ids, int n, const RobustRec* rec, const float* x0, const int32_t* cand, const MapOpts& opts, KeyState* state,
                                      const MapStore& map, MapRevisit* out, int32_t* attach, hipStream_t s);
// key[ids[b]] <- img[ids[b]][cand[b]] where attach[b] != 0; the gather's grid
hipError_t launch_keyframe_map_attach(const int32_t* ids, int n, const int32_t* cand, const int32_t* attach, const MapStore& map, uint8_t* key, hipStream_t s);

}  // namespace hnet
