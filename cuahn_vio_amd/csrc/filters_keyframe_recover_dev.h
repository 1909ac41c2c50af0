// filters_keyframe_recover_dev.h — recovering a lost camera inside the in-step keyframe track of hnet_filters (include/hnet.h
// hnet_filters_set_keyframe_recover): what capi_filters.hip, capi_keyframe.hip and kernels_filters_keyframe_recover.hip share.  The device
// compiles include/hnet_keyframe_measure_recover.h itself (host + device functions): the order of the reasons, the source of the measurement and the
// next prev_ok are the functions tests/test_filters_keyframe_recover_cpu.py pins on the host.
#pragma once
#include "filters_keyframe_dev.h"
#include "keyframe_recover_dev.h"

#pragma clang force_cuda_host_device begin
#include "../../include/hnet_keyframe_measure_recover.h"
#pragma clang force_cuda_host_device end

struct hnet_keyframe_relocalise_opts;
struct hnet_photo_search_hyp;

namespace hnet {

using KfmrRec = hnet_kfmr::Record;            // = hnet_keyframe_measure_recover
static_assert(sizeof(KfmrRec) == sizeof(KfmRec) + sizeof(OrientedRelocRec) && offsetof(KfmrRec, reloc) == sizeof(KfmRec), "packed layouts");

// One wavefront per slot b < n, after the track's alignment (rec [levels][n]: its records): the session's decision on `state` (a working copy of the
// table) -> out[b] (every byte written), copy[b], stash[b], active[b] as launch_recover_decide leaves them when recover_on[ids[b]] != 0, and as
// launch_keyframe_decide leaves out[b] and copy[b] otherwise (active 0, the stash zero); accepted[b] = the trials the alignment accepted over its levels
// (the relocalisation's alignment reuses rec)
hipError_t launch_filter_kfmr_decide(const KeyTable& tab, int n, int n_sessions, const RobustRec* rec, int levels, const float* x0, const KeyOpts& opts,
                                     const int32_t* recover_on, KeyState* state, KeyTrack* out, int32_t* copy, RecoverStash* stash, int32_t* active,
                                     int32_t* accepted, hipStream_t s);
// launch_filter_kfm_measure on the records of a track with recovery (rout [n]: launch_recover_finish's; accepted [n]: the decide kernel's; rec2
// [levels2][n]: the records of the relocalisation's alignment): the reasons in hnet_kfmr's order, the measurement from the track's record or, for a
// RETRACKED slot, from the relocalise's with FROM_RELOC
hipError_t launch_filter_kfmr_measure(const int32_t* ids, int n, int n_sessions, const FilterParams* params, const KfmCfg* cfg, const KeyState* key_state,
                                      const int32_t* prev_ok, const RecoverRec* rout, const int32_t* accepted, const RobustRec* rec2, int levels2, const int32_t* updates,
                                      float* m72, int32_t* gate, int32_t* opened, KfmRec* out, hipStream_t s);
// launch_filter_kfm_finish with hnet_kfmr's next prev_ok; reloc_out[b] = rout[b].reloc for every slot (zero_reloc where no relocalisation ran): the
// {measure | reloc} sections of the step's one download
hipError_t launch_filter_kfmr_finish(const int32_t* ids, int n, int n_sessions, const InnovRec* innov, const int32_t* updates, const int32_t* opened, int iters,
                                     const RecoverRec* rout, int32_t* prev_ok_next, KfmRec* out, OrientedRelocRec* reloc_out, hipStream_t s);

}  // namespace hnet

// ---- what capi_filters.hip reaches of the keyframe store's recovery through capi_keyframe.hip
namespace capi __attribute__((visibility("hidden"))) {

// what an in-step track with recovery leaves for the measure kernel: the records of the SECOND alignment [reloc levels][n], the call's records [n]
// (track after finish | reloc, zero_reloc where none ran) and the store's state table as it was before the call
struct KeyInstepRecover { const hnet::RobustRec* rec2; const hnet::RecoverRec* rout; const hnet::KeyState* state; };

// o <- *opts checked as hnet_sessions_keyframe_relocalise_oriented checks them, the table (hyps null with n_hyp 0: the identity entry alone) into
// table [<= 64] and *n_table; or the context's error
int keyframes_recover_check(hnet_sessions* s, const hnet_keyframe_relocalise_opts* opts, const hnet_photo_search_hyp* hyps, int n_hyp, const char* who,
                            hnet::RelocOpts& o, hnet::SearchHyp* table, int* n_table);
// the relocalisation's scratch and, with a map, the working copies of its entries and states: allocated here, never inside a step (a map enabled
// later allocates its working copies at its enable)
int keyframes_instep_recover_ensure(hnet_sessions* s, const char* who);
// hnet_sessions_keyframe_track_recover's launches between its upload and its finish's note, in its order, with every table write on working copies
// (state_work, the map's entries and states) and every image write left out; recover_on [n_sessions] and accepted [n] are the caller's device words
int keyframes_instep_track_recover(hnet_sessions* s, const hnet::KeyTable& tab, int n, const hnet::KeyOpts& o, const hnet::RelocOpts& ro, const hnet::SearchHyp* d_hyps,
                                   int n_hyp, const int32_t* recover_on, uint8_t* prev, uint8_t* curr, hnet::KeyState* state_work, int32_t* accepted,
                                   KeyInstepRecover* v, hipStream_t st);
// the commits of the accepted attempt, stream ordered and unsynchronised: the tables, then the image writes in the order of the sessions call - the
// first commit and its map store, the attach, the second commit and its map store
int keyframes_instep_commit_recover(hnet_sessions* s, const hnet::KeyTable& tab, int n, const uint8_t* curr, const hnet::KeyState* state_work, hipStream_t st);

}  // namespace capi
