// photo_search_oriented_dev.h — the coarse search under a table of orientation hypotheses and the relocalisation on top of it (include/hnet.h
// hnet_op_photo_search_oriented, hnet_sessions_photo_search_oriented, hnet_sessions_keyframe_relocalise_oriented): what
// capi_photo_search_oriented.hip, capi_keyframe.hip and kernels_photo_search_oriented.hip share.  The device compiles
// include/hnet_photo_search_oriented.h itself (host + device functions): warp_pixel, hyp_better, offer_hyp, start_of and finish are the functions
// tests/test_photo_search_oriented_cpu.py pins on the host.
#pragma once
#include "photo_search_dev.h"

#pragma clang force_cuda_host_device begin
#include "../../include/hnet_photo_search_oriented.h"
#pragma clang force_cuda_host_device end

namespace hnet {

using SearchHyp = hnet_search_oriented::Hyp;            // = hnet_photo_search_hyp
using OrientedRec = hnet_search_oriented::Record;       // = hnet_photo_search_oriented
// = hnet_keyframe_relocalise_oriented: 7r's record with the oriented search record in place of the plain one
struct OrientedRelocRec {
    MapRevisit rv;
    OrientedRec search;
    int32_t target, n_searched, n_found, pad;
};
constexpr int SEARCH_MAX_HYP = hnet_search_oriented::MAX_HYP;
static_assert(sizeof(SearchHyp) == 48 && sizeof(OrientedRec) == 160 && sizeof(OrientedRelocRec) == sizeof(RelocRec) + 64 && offsetof(OrientedRelocRec, rv) == 0 &&
              offsetof(OrientedRelocRec, search) == sizeof(MapRevisit) && sizeof(OrientedRelocRec) % sizeof(double) == 0, "packed layouts");

// One workgroup per (entry x < n_hyp, job y < jobs_x, z < n): template thumbs[z ta_stride + y] warped in LDS by hyps[x] against image
// thumbs[z tb_stride + tb_off], the masked sums of every shift divided over the lanes -> hrec[(z jobs_x + y) n_hyp + x], 7r's record of the entry (every
// byte written; start_px as 7r's) and, when scores != nullptr, its score table [.][SEARCH_SHIFTS].  valid != nullptr: a job with valid[z jobs_x + y] == 0
// reads no thumbnail and writes nothing here.
hipError_t launch_photo_search_oriented(const uint8_t* thumbs, int ta_stride, int tb_stride, int tb_off, int jobs_x, int n, const int32_t* valid,
                                        const SearchOpts& opts, const SearchHyp* hyps, int n_hyp, SearchRec* hrec, double* scores, hipStream_t s);
// One wavefront per job (jobs = n jobs_x): lane h holds entry h's best; the winner and the runner-up under hnet_search_oriented::hyp_better by a butterfly,
// lane 0 writes out[job] (every byte; all zero for a job with valid[job] == 0)
hipError_t launch_photo_search_winner(const SearchRec* hrec, const SearchHyp* hyps, int n_hyp, int jobs, const int32_t* valid, OrientedRec* out, hipStream_t s);

// ---- the oriented relocalise: launch_reloc_thumbs, launch_reloc_gather and launch_keyframe_map_attach are 7r's and 7q's; the pick and the decision are
// photo_search_dev.h's on the wider records (srec [n][M + 1], out [n]): the same kernel templates, instantiated in kernels_photo_search.hip
hipError_t launch_reloc_pick(const int32_t* ids, int n, int n_sessions, const KeyState* state, int M, const int32_t* valid, const OrientedRec* srec, float* x0,
                             int32_t* cand, int32_t* mslot, OrientedRelocRec* out, hipStream_t s);
hipError_t launch_reloc_decide(const int32_t* ids, int n, int n_sessions, const RobustRec* rec, const float* x0, const int32_t* cand, const RelocOpts& opts,
                               KeyState* state, const MapStore& map, OrientedRelocRec* out, int32_t* attach, hipStream_t s);

}  // namespace hnet

struct hnet_ctx;
struct hnet_photo_search_hyp;
namespace capi {
// HNET_OK, or the context's error set for a table no call may enqueue (capi_photo_search_oriented.hip)
int photo_search_check_table(hnet_ctx* c, const hnet_photo_search_hyp* hyps, int n_hyp, const char* who);
}  // namespace capi
