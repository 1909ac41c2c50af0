// keyframe_dev.h — tracking against a held keyframe (include/hnet.h hnet_sessions_keyframe_track): what capi_keyframe.hip and
// kernels_keyframe.hip share.  The device compiles include/hnet_keyframe.h itself (host + device functions): compose and decide are the functions
// tests/test_keyframe_cpu.py pins on the host.
#pragma once
#include "geom.h"
#include "photo_robust_dev.h"

#include <cstring>      // (ahead of the header below: the C library's declarations must not be forced host + device)

#pragma clang force_cuda_host_device begin
#include "../../include/hnet_keyframe.h"
#pragma clang force_cuda_host_device end

namespace hnet {

using KeyState = hnet_keyframe::State;       // one session's entry of the state table
using KeyTrack = hnet_keyframe::Track;       // = hnet_keyframe_track
using KeyOpts = hnet_keyframe::Opts;         // = hnet_keyframe_opts
static_assert(sizeof(KeyState) == 120 && sizeof(KeyTrack) == sizeof(RobustRec) + 160 && sizeof(KeyOpts) == sizeof(RobustOpts) + 32, "packed layouts");
constexpr int KEY_THREADS = 64;

// One call's table as it is uploaded, for n slots: {step [n][8] f32 | ids [n] i32 | curr ring slot [n] i32 | gap [n] i32}
struct KeyTable { const float* step; const int32_t *ids, *slot, *gap; };

// One wavefront per slot b < n, before the alignment: x0[b] = compose(step[b], key_px of session ids[b]), or quiet NaNs for a session without a keyframe,
// a failed composition or an id outside the table; on those every level of the alignment reports DEGENERATE and its later workgroups return at once.
hipError_t launch_keyframe_start(const KeyTable& tab, int n, int n_sessions, const KeyState* state, float* x0, hipStream_t s);
// prev[b] <- key[ids[b]], curr[b] <- ring slot tab.slot[b]; 16-byte vectors, grid (vectors, n); a slot or id out of range is skipped
hipError_t launch_keyframe_gather(const KeyTable& tab, int n, int n_sessions, const uint8_t* key, const uint8_t* ring, int n_slots, uint8_t* prev, uint8_t* curr,
                                  hipStream_t s);
// One wavefront per slot, after the alignment (rec: the level-0 records [n]): hnet_keyframe::decide on the session's state -> out[b] (every byte
// written), the new state and copy[b]
hipError_t launch_keyframe_decide(const KeyTable& tab, int n, int n_sessions, const RobustRec* rec, const float* x0, const KeyOpts& opts, KeyState* state,
                                  KeyTrack* out, int32_t* copy, hipStream_t s);
// key[ids[b]] <- curr[b] where copy[b] != 0; the gather's grid, workgroups of the other slots return at once
hipError_t launch_keyframe_commit(const KeyTable& tab, int n, int n_sessions, const int32_t* copy, const uint8_t* curr, uint8_t* key, hipStream_t s);

}  // namespace hnet
