// keyframe_recover_dev.h — recovering a lost camera inside the track (include/hnet.h hnet_sessions_keyframe_track_recover): what
// capi_keyframe.hip and kernels_keyframe_recover.hip share.  The device compiles include/hnet_keyframe_recover.h itself (host + device functions):
// decide_deferred, finish and the zero record are the functions tests/test_keyframe_recover_cpu.py pins on the host.
#pragma once
#include "photo_search_oriented_dev.h"

#include <cstddef>      // (ahead of the header below: the C library's declarations must not be forced host + device)
#include <cstring>

#pragma clang force_cuda_host_device begin
#include "../../include/hnet_keyframe_recover.h"
#pragma clang force_cuda_host_device end

namespace hnet {

using RecoverOpts = hnet_keyframe_recovery::Opts;       // = hnet_keyframe_recover_opts
using RecoverRec = hnet_keyframe_recovery::Record;      // = hnet_keyframe_recover
using RecoverStash = hnet_keyframe_recovery::Stash;     // a lost session's T1 while the relocalisation runs
static_assert(sizeof(RecoverOpts) == sizeof(KeyOpts) + sizeof(RelocOpts) && sizeof(hnet_keyframe_recovery::Reloc) == sizeof(OrientedRelocRec) &&
              offsetof(hnet_keyframe_recovery::Reloc, search) == offsetof(OrientedRelocRec, search) &&
              offsetof(hnet_keyframe_recovery::Reloc, target) == offsetof(OrientedRelocRec, target) &&
              sizeof(RecoverRec) == sizeof(KeyTrack) + sizeof(OrientedRelocRec) && offsetof(RecoverRec, reloc) == sizeof(KeyTrack) &&
              sizeof(RecoverStash) == sizeof(KeyState) + 160 && sizeof(RecoverRec) % 8 == 0, "packed layouts");

// ---- a track with recovery (tab: the track's table; rec: the records [levels][n] of the track's alignment).  One wavefront per slot b < n, after the
// alignment: hnet_keyframe_recovery::decide_deferred on the session's state -> out[b] (every byte written), the new state, copy[b], stash[b] and
// active[b] (1: the frame is LOST and the relocalisation is to run on it; 0 for an id outside the table).  recover_on: null, or [n_sessions] - a session
// whose word is 0 gets what launch_keyframe_decide leaves in out[b] and copy[b] instead (active 0, the stash zero).  accepted: null, or [n] -
// accepted[b] = the trials the alignment accepted over its levels (the relocalisation's alignment reuses rec)
hipError_t launch_recover_decide(const KeyTable& tab, int n, int n_sessions, const RobustRec* rec, int levels, const float* x0, const KeyOpts& opts,
                                 const int32_t* recover_on, KeyState* state, KeyTrack* out, int32_t* copy, RecoverStash* stash, int32_t* active, int32_t* accepted,
                                 hipStream_t s);
// One wavefront per slot, after the relocalisation's decision (reloc [n]: its records): hnet_keyframe_recovery::finish on the active slots (the state and
// track[b] in place) -> copy2[b] and redo[b] (1: unrecovered, T1 was restored), and out[b] = {track[b] | reloc[b], or the zero record when inactive}
hipError_t launch_recover_finish(const int32_t* ids, int n, int n_sessions, const int32_t* active, const RecoverStash* stash, const OrientedRelocRec* reloc,
                                 KeyState* state, KeyTrack* track, int32_t* copy2, int32_t* redo, RecoverRec* out, hipStream_t s);
// launch_keyframe_map_note for the slots with redo[b] != 0 only; store[b] = -1 for the others
hipError_t launch_recover_note(const int32_t* ids, int n, const KeyTrack* track, const int32_t* copy2, const int32_t* redo, const KeyState* state,
                               const MapStore& map, int32_t* store, hipStream_t s);

}  // namespace hnet
