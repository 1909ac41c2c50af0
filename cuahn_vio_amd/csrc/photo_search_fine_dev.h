// photo_search_fine_dev.h — the fine stage of the search around the oriented winner and the relocalisation on top of it (include/hnet.h
// hnet_op_photo_search_fine, hnet_sessions_photo_search_fine, hnet_sessions_keyframe_relocalise_fine): what capi_photo_search_fine.hip,
// capi_keyframe.hip and kernels_photo_search_fine.hip share.  The device compiles include/hnet_photo_search_fine.h itself (host + device functions):
// thumb_pixel, warp_pixel, better, offer, start_of and finish are the functions tests/test_photo_search_fine_cpu.py pins on the host.
#pragma once
#include "photo_search_oriented_dev.h"

#pragma clang force_cuda_host_device begin
#include "../../include/hnet_photo_search_fine.h"
#pragma clang force_cuda_host_device end

namespace hnet {

using FineOpts = hnet_search_fine::Opts;          // = hnet_photo_search_fine_opts
using FinePart = hnet_search_fine::Part;          // = hnet_photo_search_fine_part
using FineRec = hnet_search_fine::Record;         // = hnet_photo_search_fine
using FineEntry = hnet_search_fine::Entry;        // one fine entry's best, between the search and the winner
// = hnet_keyframe_relocalise_fine: the oriented relocalise's record, then the fine part of the picked candidate
struct FineRelocRec {
    OrientedRelocRec base;
    FinePart fine;
};
constexpr int FINE_THUMB_BYTES = hnet_search_fine::FPIX, FINE_SHIFTS = hnet_search_fine::NSHIFT, FINE_MAX = hnet_search_fine::MAX_FINE;
static_assert(sizeof(FineOpts) == 24 && sizeof(FinePart) == 128 && sizeof(FineRec) == 288 && sizeof(FineRelocRec) == sizeof(OrientedRelocRec) + 128 &&
                  offsetof(FineRelocRec, fine) == sizeof(OrientedRelocRec) && sizeof(FineEntry) == 40 && FINE_THUMB_BYTES % 16 == 0,
              "packed layouts; level-2 thumbnails stay 16-byte aligned in an array of them");

// thumbs[i] <- the level-2 thumbnail of frames[idx ? idx[i] : i], i < count; frames: device u8 [.][NPIX]; an idx outside 0 .. n_frames-1 is skipped
hipError_t launch_photo_fine_thumbs(const uint8_t* frames, const int32_t* idx, int n_frames, int count, uint8_t* thumbs, hipStream_t s);

// One workgroup per (fine entry x < n_fine, job y < jobs): the job's coarse record is read at coarse + y coarse_stride bytes; unless it is FOUND with its
// winner inside the table (and cand == nullptr or cand[y] >= 0) the workgroup returns at once, after filling its score table with quiet NaNs when asked.
// Else template thumbs[y ta_stride] is warped in LDS by fine[hyp n_fine + x] against image thumbs[y tb_stride + tb_off] over the shifts of the radius ->
// ent[y n_fine + x] and, when scores != nullptr, scores[y n_fine + x][FINE_SHIFTS].
hipError_t launch_photo_search_fine(const uint8_t* thumbs, int ta_stride, int tb_stride, int tb_off, int jobs, const uint8_t* coarse, int coarse_stride,
                                    const int32_t* cand, const SearchOpts& opts, const FineOpts& fopts, const SearchHyp* fine, int n_hyp, FineEntry* ent,
                                    double* scores, hipStream_t s);
// One wavefront per job: lane j holds entry j's best, a butterfly under hnet_search_fine::better, lane 0 writes the fine part (every byte) at
// out + y out_stride + part_off; copy_coarse: the lanes copy the coarse record to out + y out_stride first.  x0 != nullptr: unless SKIPPED the final
// start goes to x0[8 y], the alignment's start table.
hipError_t launch_photo_search_fine_winner(const FineEntry* ent, int jobs, const uint8_t* coarse, int coarse_stride, const int32_t* cand, const FineOpts& fopts,
                                           const SearchHyp* fine, int n_hyp, uint8_t* out, int out_stride, int part_off, bool copy_coarse, float* x0, hipStream_t s);
// out[b].base <- base[b], b < n: the oriented relocalise's records in front of the fine parts the winner wrote
hipError_t launch_reloc_fine_pack(const OrientedRelocRec* base, int n, FineRelocRec* out, hipStream_t s);

}  // namespace hnet

struct hnet_photo_search_fine_opts;
namespace capi {
// HNET_OK and fo <- *fine_opts with its pads zeroed, or the context's error set for options or a fine table no call may enqueue (capi_photo_search_fine.hip)
int photo_search_fine_check(hnet_ctx* c, const hnet_photo_search_fine_opts* fine_opts, const hnet_photo_search_hyp* fine, int n_hyp, const char* who,
                            hnet::FineOpts& fo);
}  // namespace capi
