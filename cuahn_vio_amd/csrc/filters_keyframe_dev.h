// filters_keyframe_dev.h — the keyframe track as an in-step measurement of hnet_filters (include/hnet.h hnet_filters_set_keyframe_measure) and
// the recovery of a lost camera inside that track (hnet_filters_set_keyframe_recover): what capi_filters.hip, capi_keyframe.hip and
// kernels_filters_keyframe.hip share.  The device compiles include/hnet_keyframe_measure.h and include/hnet_keyframe_measure_recover.h itself (host +
// device functions): the step, the usability tests and their order, z, the source of the measurement and the next prev_ok are the functions
// tests/test_filters_keyframe_cpu.py and tests/test_filters_keyframe_recover_cpu.py pin on the host.
#pragma once
#include "filters_refine_dev.h"
#include "keyframe_map_dev.h"
#include "keyframe_recover_dev.h"

#pragma clang force_cuda_host_device begin
#include "../../include/hnet_keyframe_measure.h"
#include "../../include/hnet_keyframe_measure_recover.h"
#pragma clang force_cuda_host_device end

struct hnet_sessions;
struct hnet_keyframe_relocalise_opts;
struct hnet_photo_search_hyp;

namespace hnet {

using KfmRec = hnet_kfm::Record;             // = hnet_keyframe_measure
using KfmOpts = hnet_kfm::Opts;              // = hnet_keyframe_measure_opts
static_assert(sizeof(KfmRec) == sizeof(KeyTrack) + 64 + 64 * sizeof(double) + sizeof(InnovRec) + 8 && offsetof(KfmRec, step_px) == sizeof(KeyTrack) &&
              offsetof(KfmRec, r_px) == sizeof(KeyTrack) + 64 && offsetof(KfmRec, r) == offsetof(KfmRec, r_px) + 64 * sizeof(double) &&
              offsetof(KfmRec, flags) == offsetof(KfmRec, r) + sizeof(InnovRec) && sizeof(KfmOpts) == sizeof(KeyOpts) + 32, "packed layouts");
constexpr int KFM_REC_DOUBLES = (int)(sizeof(KfmRec) / sizeof(double));           // 306
constexpr int KFM_THREADS = 64;
using KfmrRec = hnet_kfmr::Record;            // = hnet_keyframe_measure_recover
static_assert(sizeof(KfmrRec) == sizeof(KfmRec) + sizeof(OrientedRelocRec) && offsetof(KfmrRec, reloc) == sizeof(KfmRec), "packed layouts");

// one session's measurement as the kernels read it: on = 0 is off (hnet_filters_set_keyframe_measure)
struct KfmCfg { double cov_scale, sigma_floor_px, max_mse; int32_t when, on; };

// One wavefront per slot b < n, after the network's iterations.  A session with cfg.on: out[b] = {flags ASKED, step_px, zeros} and step[b] = step_px =
// (float)(159.5 * offset) of work[b], where launch_keyframe_start reads it; every other slot: out[b] = zeros and step[b] = quiet NaNs.
hipError_t launch_filter_kfm_step(const int32_t* ids, int n, int n_sessions, const KfmCfg* cfg, const FilterRec* work, float* step, KfmRec* out, hipStream_t s);
// One wavefront per slot, after the track (key_state and prev_ok: the tables as they were BEFORE the track).  The track's records are EITHER track [n],
// of a plain track, with rec [levels][n] its alignment's records and accepted null; OR rout [n], launch_recover_finish's of a track with recovery, with
// accepted [n] launch_recover_decide's and rec [levels][n] the records of the relocalisation's alignment.  Asked slots: the track's record goes into
// out[b], the measurement with the session's k_net_cov into m72[b] (72 floats), out[b].z_px and out[b].r_px - hnet_kfmr's rule: the reasons in its
// order, the measurement from the track's record or, for a RETRACKED slot, from the relocalise's with FROM_RELOC; on a plain track's records that is
// hnet_kfm's; gate[b] = 1 and opened[b] = updates[b] for a usable selected slot; an unusable one sets its reason bit, an unselected one NOT_SELECTED.
// Every other slot: gate[b] = 0, opened[b] = -1.
hipError_t launch_filter_kfm_measure(const int32_t* ids, int n, int n_sessions, const FilterParams* params, const KfmCfg* cfg, const KeyState* key_state,
                                     const int32_t* prev_ok, const KeyTrack* track, const RecoverRec* rout, const int32_t* accepted, const RobustRec* rec, int levels,
                                     const int32_t* updates, float* m72, int32_t* gate, int32_t* opened, KfmRec* out, hipStream_t s);
// After the measurement's innovation and update launches: the innovation record (iteration = iters) and APPLIED / NIS_REJECTED / S_SINGULAR of the slots
// the measure kernel opened, and prev_ok_next[ids[b]] of every asked slot (a copy of the table that the accepted call's tail puts back; hnet_kfmr's next
// prev_ok, which without RECOVERED is hnet_kfm's).  rout and reloc_out: both null, or reloc_out[b] = rout[b].reloc for every slot (zero_reloc where no
// relocalisation ran): the {measure | reloc} sections of the step's one download
hipError_t launch_filter_kfm_finish(const int32_t* ids, int n, int n_sessions, const InnovRec* innov, const int32_t* updates, const int32_t* opened, int iters,
                                    const RecoverRec* rout, int32_t* prev_ok_next, KfmRec* out, OrientedRelocRec* reloc_out, hipStream_t s);
// (State::reset_4pt_offset of every slot, with or without a measurement, is the measurement's filter_update_kernel launch with last = 1)

}  // namespace hnet

// ---- what capi_filters.hip reaches of the keyframe store through capi_keyframe.hip (the store itself: keyframes_internal.h)
namespace capi __attribute__((visibility("hidden"))) {

// the recovering part of a track: the reloc options, the device table of the oriented search and, of a track inside a filter step, the per-session
// recover_on words (null: every listed session recovers) and where the trials the track's alignment accepted are kept [n] (null: nowhere)
struct KeyRecovery { hnet::RelocOpts o; const hnet::SearchHyp* d_hyps; int n_hyp; const int32_t* recover_on; int32_t* accepted; };
// what an in-step track leaves for launch_filter_kfm_measure and _finish: the records [levels][n] of the last alignment, the track's records [n] - track
// of a plain track, rout of one with recovery (track after finish | reloc, zero_reloc where none ran), the other null - and the store's state table as
// it was before the call
struct KeyInstep { const hnet::RobustRec* rec; int levels; const hnet::KeyTrack* track; const hnet::RecoverRec* rout; const hnet::KeyState* state; };

bool keyframes_enabled(const hnet_sessions* s);
// the {ids | curr ring slot | gap} sections [3][n] of a track's table for the sessions ids[0 .. n): the id of a session with on[id] == 0 (on null: of
// none) is -1, on which every launch of the track skips the slot
void keyframes_table(const hnet_sessions* s, int n, const int32_t* ids, const uint8_t* on, int32_t* tab);
// o <- *opts checked as hnet_sessions_keyframe_relocalise_oriented checks them, the table (hyps null with n_hyp 0: the identity entry alone) into
// table [<= 64] and *n_table; or the context's error
int keyframes_recover_check(hnet_sessions* s, const hnet_keyframe_relocalise_opts* opts, const hnet_photo_search_hyp* hyps, int n_hyp, const char* who,
                            hnet::RelocOpts& o, hnet::SearchHyp* table, int* n_table);
// the relocalisation's scratch and, with a map, the working copies of its entries and states: allocated here, never inside a step (a map enabled
// later allocates its working copies at its enable)
int keyframes_instep_recover_ensure(hnet_sessions* s, const char* who);
// the launches of hnet_sessions_keyframe_track (rc null) or of hnet_sessions_keyframe_track_recover between the upload and the download, in their
// order, enqueued on the context's stream for the table `tab` (its step section written on the device), without the commits and stores of images and
// without the attach: the keyframe and the current frame gathered into prev / curr (never the context's staging), and every table write on working
// copies made here (state_work and, with recovery, the map's entries and states) - the store itself is not written, so that a repeated attempt starts
// from what the call found and leaves one map serial and not two
int keyframes_instep_track(hnet_sessions* s, const hnet::KeyTable& tab, int n, const hnet::KeyOpts& o, const KeyRecovery* rc, uint8_t* prev, uint8_t* curr,
                           hnet::KeyState* state_work, KeyInstep* v);
// the commits of the accepted attempt's track, stream ordered and unsynchronised: the tables, then the image writes in the order of the sessions call -
// the new keyframes' images and their map store and, recovering: the attach, the second commit and its map store
int keyframes_instep_commit(hnet_sessions* s, const hnet::KeyTable& tab, int n, bool recovering, const uint8_t* curr, const hnet::KeyState* state_work);
// the host mirrors after an accepted call: the sessions with on[id] hold a keyframe, and their image count at this track
void keyframes_instep_accepted(hnet_sessions* s, int n, const int32_t* ids, const uint8_t* on);

}  // namespace capi
