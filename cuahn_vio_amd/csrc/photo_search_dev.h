// photo_search_dev.h — the coarse search over integer translations and the relocalisation on top of it (include/hnet.h hnet_op_photo_search,
// hnet_sessions_photo_search, hnet_sessions_keyframe_relocalise): what capi_photo_search.hip, capi_keyframe.hip and
// kernels_photo_search.hip share.  The device compiles include/hnet_photo_search.h and include/hnet_keyframe_reloc.h themselves (host + device
// functions): thumb_pixel, shift_score, better, offer, finish and decide_relocalise are the functions tests/test_photo_search_cpu.py pins on the host.
#pragma once
#include "keyframe_map_dev.h"

#include <cstring>      // (ahead of the headers below: the C library's declarations must not be forced host + device)

#pragma clang force_cuda_host_device begin
#include "../../include/hnet_keyframe_reloc.h"
#pragma clang force_cuda_host_device end

namespace hnet {

using SearchOpts = hnet_search::Opts;      // = hnet_photo_search_opts
using SearchRec = hnet_search::Record;     // = hnet_photo_search
using RelocOpts = hnet_keyframe_reloc::Opts;     // = hnet_keyframe_relocalise_opts
using RelocRec = hnet_keyframe_reloc::Reloc;     // = hnet_keyframe_relocalise
constexpr int THUMB_BYTES = hnet_search::TPIX, SEARCH_SHIFTS = hnet_search::NSHIFT;
constexpr int RELOC_MAX_CANDIDATES = hnet_keyframe_reloc::MAX_CANDIDATES;
static_assert(sizeof(SearchOpts) == 32 && sizeof(SearchRec) == 96 && sizeof(RelocOpts) == sizeof(RobustOpts) + 64 && sizeof(RelocRec) == sizeof(MapRevisit) + 112 &&
              THUMB_BYTES % 16 == 0, "packed layouts; thumbnails stay 16-byte aligned in an array of them");

// thumbs[i] <- the thumbnail of frames[idx ? idx[i] : i], i < count; frames: device u8 [.][NPIX], 8-byte aligned; an idx outside 0 .. n_frames-1 is skipped
hipError_t launch_photo_thumbs(const uint8_t* frames, const int32_t* idx, int n_frames, int count, uint8_t* thumbs, hipStream_t s);

// One workgroup per job (x < jobs_x, y < n): template thumbs[y ta_stride + x] against image thumbs[y tb_stride + tb_off]; both thumbnails and the score of
// every shift in LDS, the shifts divided over the lanes, one fixed-order reduction for the best and a second one for `second` -> rec[y jobs_x + x] (every
// byte written) and, when scores != nullptr, the score table [y jobs_x + x][SEARCH_SHIFTS].  valid != nullptr: a job with valid[y jobs_x + x] == 0 reads no
// thumbnail and writes an all-zero record (flags 0: not searched).
hipError_t launch_photo_search(const uint8_t* thumbs, int ta_stride, int tb_stride, int tb_off, int jobs_x, int n, const int32_t* valid, const SearchOpts& opts,
                               SearchRec* rec, double* scores, hipStream_t s);

// ---- a relocalise (ids, slot: the call's table {ids [n] | curr ring slot [n]}); M = map.capacity, or 0 without a map (map.img == nullptr).  Per listed
// session b the candidates are index 0 (the held keyframe) and 1 + slot (a valid entry other than the current keyframe's); thumbs [n][M + 2] holds theirs
// and, last, the current frame's; valid [n][M + 1] whether a candidate exists (0 for all when the id or the ring slot is outside its table).
// active != nullptr (a track with recovery): every candidate of a slot with active[b] == 0 is absent and no thumbnail is made for it; on that input the
// search, the winner, the pick, the gather, the alignment, the decision and the attach do nothing for the slot
hipError_t launch_reloc_thumbs(const int32_t* ids, const int32_t* slot, int n, int n_sessions, const int32_t* active, const KeyState* state, const uint8_t* key,
                               const MapStore& map, const uint8_t* ring, int n_slots, uint8_t* thumbs, int32_t* valid, hipStream_t s);
// One wavefront per slot, lane 0, over the search records srec [n][M + 1]: hnet_keyframe_reloc::offer in the order of the indices -> cand[b] (the index or
// -1), mslot[b] (the map slot or -1), x0[b] (the pick's start, quiet NaNs without one), and out[b]'s search record, target, counts and h_origin_before
hipError_t launch_reloc_pick(const int32_t* ids, int n, int n_sessions, const KeyState* state, int M, const int32_t* valid, const SearchRec* srec, float* x0,
                             int32_t* cand, int32_t* mslot, RelocRec* out, hipStream_t s);
// prev[b] <- the picked candidate's image, curr[b] <- ring slot; slots without a pick return at once (their start is NaN and the alignment returns on it)
hipError_t launch_reloc_gather(const int32_t* ids, const int32_t* slot, int n, int n_sessions, const int32_t* cand, const uint8_t* key, const MapStore& map,
                               const uint8_t* ring, int n_slots, uint8_t* prev, uint8_t* curr, hipStream_t s);
// One wavefront per slot, after the alignment (rec: the level-0 records [n]): the lanes copy the record (zeros without a pick), lane 0 runs
// decide_relocalise (the held keyframe) or hnet_keyframe_map::decide_revisit (a map entry, or no pick) in place -> out[b].rv and attach[b]
hipError_t launch_reloc_decide(const int32_t* ids, int n, int n_sessions, const RobustRec* rec, const float* x0, const int32_t* cand, const RelocOpts& opts,
                               KeyState* state, const MapStore& map, RelocRec* out, int32_t* attach, hipStream_t s);

}  // namespace hnet

struct hnet_ctx;
struct hnet_photo_search_opts;
namespace capi {
// HNET_OK and o <- *opts with its pad zeroed, or the context's error set for options no search may run under (capi_photo_search.hip)
int photo_search_check_opts(hnet_ctx* c, const hnet_photo_search_opts* opts, const char* who, hnet::SearchOpts& o);
}  // namespace capi
