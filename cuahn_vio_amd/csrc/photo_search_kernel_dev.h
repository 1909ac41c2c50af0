// photo_search_kernel_dev.h — device code that kernels_photo_search.hip and kernels_photo_search_oriented.hip share: the layout of a
// thumbnail in LDS between its guards, the reduction of a score table, the tail of a search workgroup once its table is filled, and the test of a map
// store that the relocalisation's kernels (and kernels_keyframe_recover.hip) apply.  Included by .hip kernel files only.
#pragma once
#include "photo_search_dev.h"

namespace hnet {
namespace {

constexpr int PS_GUARD = 32;                                             // guard bytes on either side of the image thumbnail in LDS
constexpr int TWORDS = hnet_search::TPIX / 4, ROW_WORDS = hnet_search::TW / 4, BWORDS = (hnet_search::TPIX + 2 * PS_GUARD) / 4;
static_assert(hnet_search::TW % 4 == 0 && PS_GUARD % 4 == 0 && PS_GUARD >= hnet_search::MAX_RX + 2,
              "rows are whole dwords; the guard holds the farthest column of a shifted group");
// the farthest dword a shift reads: row TH - 1, the last group of the row, shifted right by MAX_RX, and the dword after it
static_assert(((PS_GUARD + (hnet_search::TH - 1) * hnet_search::TW + hnet_search::MAX_RX + (hnet_search::TW - 4)) >> 2) + 1 < BWORDS &&
                  PS_GUARD - hnet_search::MAX_RX >= 0,
              "a shifted group stays inside the guards");

// a store whose images the relocalisation may read (kernels_keyframe_map.hip's map_ok asks for no image array: a different predicate)
__device__ inline bool reloc_map_ok(const MapStore& map) {
    return map.img != nullptr && map.capacity >= hnet_keyframe_map::MIN_CAPACITY && map.capacity <= hnet_keyframe_map::MAX_CAPACITY;
}

// the workgroup's best of the table under the header's order; `around` >= 0: among the shifts outside the 3 x 3 around it.  Every thread returns it.
template <int THREADS>
__device__ __forceinline__ hnet_search::Best table_best(const double* sc, int around, double* red_s, int32_t* red_i) {
    namespace ps = hnet_search;
    const int tid = threadIdx.x;
    ps::Best b;
    ps::best_none(b);
    for (int i = tid; i < ps::NSHIFT; i += THREADS)
        if (around < 0 || ps::outside3(i, around)) ps::offer(b, sc[i], i);
    red_s[tid] = b.score;
    red_i[tid] = b.index;
    __syncthreads();
    for (int st = THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) {
            ps::Best x = {red_s[tid], red_i[tid]};
            ps::offer(x, red_s[tid + st], red_i[tid + st]);
            red_s[tid] = x.score;
            red_i[tid] = x.index;
        }
        __syncthreads();
    }
    b.score = red_s[0];
    b.index = red_i[0];
    __syncthreads();                                                      // (red_* are free again)
    return b;
}

// a search workgroup of THREADS threads once its score table sc [NSHIFT] is filled and synchronised: the best, the second, thread 0's sums of the best
// shift (sums(dx, dy, s): the kernel's own shift_sums on its thumbnails in LDS) and hnet_search::finish -> rec[slot]; the table -> scores[slot] when asked
template <int THREADS, class SumsAt>
__device__ __forceinline__ void search_finish(const double* sc, double* red_s, int32_t* red_i, const SearchOpts& o, SumsAt sums, size_t slot,
                                              SearchRec* __restrict__ rec, double* __restrict__ scores) {
    namespace ps = hnet_search;
    const int tid = threadIdx.x;
    const ps::Best best = table_best<THREADS>(sc, -1, red_s, red_i);
    ps::Best second;
    ps::best_none(second);
    if (best.index >= 0) second = table_best<THREADS>(sc, best.index, red_s, red_i);      // (workgroup-uniform: every thread holds the same best)
    if (tid == 0) {
        ps::Sums s = {0, 0, 0, 0, 0, 0};
        if (best.index >= 0) {
            int dx, dy;
            ps::index_shift(best.index, dx, dy);
            sums(dx, dy, s);
        }
        ps::finish(best, second, s, o, rec[slot]);
    }
    if (scores)
        for (int i = tid; i < ps::NSHIFT; i += THREADS) scores[slot * ps::NSHIFT + i] = sc[i];
}

}  // namespace
}  // namespace hnet
