// filters_keyframe_dev.h — the keyframe track as an in-step measurement of hnet_filters (include/hnet.h hnet_filters_set_keyframe_measure): what
// capi_filters.hip, capi_keyframe.hip and kernels_filters_keyframe.hip share.  The device compiles include/hnet_keyframe_measure.h itself (host + device
// functions): the step, the usability tests and z are the functions tests/test_filters_keyframe_cpu.py pins on the host.
#pragma once
#include "filters_refine_dev.h"
#include "keyframe_map_dev.h"

#pragma clang force_cuda_host_device begin
#include "../../include/hnet_keyframe_measure.h"
#pragma clang force_cuda_host_device end

struct hnet_sessions;

namespace hnet {

using KfmRec = hnet_kfm::Record;             // = hnet_keyframe_measure
using KfmOpts = hnet_kfm::Opts;              // = hnet_keyframe_measure_opts
static_assert(sizeof(KfmRec) == sizeof(KeyTrack) + 64 + 64 * sizeof(double) + sizeof(InnovRec) + 8 && offsetof(KfmRec, step_px) == sizeof(KeyTrack) &&
              offsetof(KfmRec, r_px) == sizeof(KeyTrack) + 64 && offsetof(KfmRec, r) == offsetof(KfmRec, r_px) + 64 * sizeof(double) &&
              offsetof(KfmRec, flags) == offsetof(KfmRec, r) + sizeof(InnovRec) && sizeof(KfmOpts) == sizeof(KeyOpts) + 32, "packed layouts");
constexpr int KFM_REC_DOUBLES = (int)(sizeof(KfmRec) / sizeof(double));           // 306
constexpr int KFM_THREADS = 64;

// one session's measurement as the kernels read it: on = 0 is off (hnet_filters_set_keyframe_measure)
struct KfmCfg { double cov_scale, sigma_floor_px, max_mse; int32_t when, on; };

// One wavefront per slot b < n, after the network's iterations.  A session with cfg.on: out[b] = {flags ASKED, step_px, zeros} and step[b] = step_px =
// (float)(159.5 * offset) of work[b], where launch_keyframe_start reads it; every other slot: out[b] = zeros and step[b] = quiet NaNs.
hipError_t launch_filter_kfm_step(const int32_t* ids, int n, int n_sessions, const KfmCfg* cfg, const FilterRec* work, float* step, KfmRec* out, hipStream_t s);
// One wavefront per slot, after the track's decide (track [n]: its records; rec [levels][n]: the alignment's; key_state and prev_ok: the tables as they
// were BEFORE the track).  Asked slots: the track's record goes into out[b], hnet_kfm's measurement with the session's k_net_cov into m72[b] (72
// floats), out[b].z_px and out[b].r_px; gate[b] = 1 and opened[b] = updates[b] for a usable selected slot; an unusable one sets its reason bit, an
// unselected one NOT_SELECTED.  Every other slot: gate[b] = 0, opened[b] = -1.
hipError_t launch_filter_kfm_measure(const int32_t* ids, int n, int n_sessions, const FilterParams* params, const KfmCfg* cfg, const KeyState* key_state,
                                     const int32_t* prev_ok, const KeyTrack* track, const RobustRec* rec, int levels, const int32_t* updates, float* m72,
                                     int32_t* gate, int32_t* opened, KfmRec* out, hipStream_t s);
// After the measurement's innovation and update launches: the innovation record (iteration = iters) and APPLIED / NIS_REJECTED / S_SINGULAR of the slots
// the measure kernel opened, and prev_ok_next[ids[b]] of every asked slot (a copy of the table that the accepted call's tail puts back)
hipError_t launch_filter_kfm_finish(const int32_t* ids, int n, int n_sessions, const InnovRec* innov, const int32_t* updates, const int32_t* opened, int iters,
                                    int32_t* prev_ok_next, KfmRec* out, hipStream_t s);
// (State::reset_4pt_offset of every slot, with or without a measurement, is the measurement's filter_update_kernel launch with last = 1)

}  // namespace hnet

// ---- what capi_filters.hip reaches of the keyframe store through capi_keyframe.hip (the store's type is private to that file)
namespace capi __attribute__((visibility("hidden"))) {

// what an in-step track leaves for the measure kernel: the alignment's records [levels][n], the track's records [n] and the store's state table
struct KeyInstep { const hnet::RobustRec* rec; const hnet::KeyTrack* out; const hnet::KeyState* state; };

bool keyframes_enabled(const hnet_sessions* s);
// the {ids | curr ring slot | gap} sections [3][n] of a track's table for the sessions ids[0 .. n): the id of a session with on[id] == 0 is -1, on which
// every launch of the track skips the slot
void keyframes_instep_table(const hnet_sessions* s, int n, const int32_t* ids, const uint8_t* on, int32_t* tab);
// hnet_sessions_keyframe_track's launches up to decide, enqueued on st for the table `tab` (its step section written on the device): the keyframe and
// the current frame gathered into prev / curr (never the context's staging), and decide on state_work, a copy of the state table made here - the store
// itself is not written, so that a repeated attempt starts from what the call found
int keyframes_instep_track(hnet_sessions* s, const hnet::KeyTable& tab, int n, const hnet::KeyOpts& o, uint8_t* prev, uint8_t* curr, hnet::KeyState* state_work,
                           KeyInstep* v, hipStream_t st);
// the commits of the accepted attempt's track, stream ordered and unsynchronised: the state table, the new keyframes' images and, with a map, its note and store
int keyframes_instep_commit(hnet_sessions* s, const hnet::KeyTable& tab, int n, const uint8_t* curr, const hnet::KeyState* state_work, hipStream_t st);
// the host mirrors after an accepted call: the sessions with on[id] hold a keyframe, and their image count at this track
void keyframes_instep_accepted(hnet_sessions* s, int n, const int32_t* ids, const uint8_t* on);

}  // namespace capi
