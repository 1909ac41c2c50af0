/* hnet_photo_masked.h — the robust photometric alignment on the pixels of the template a mask admits (include/hnet.h hnet_op_photo_align_masked;
 * DESIGN 7ae), dependency free: what the device (csrc/kernels_photo_masked.hip) and the host reference (tests/cpp/photo_masked_ref.cpp) both compile, on
 * top of include/hnet_photo_robust.h, whose quantity, sums, step, records, per-level min_valid and start of a level serve unchanged.
 *
 * The mask.  A u8 image [224][320] beside img1; non-zero: the template pixel takes part.  Level L of the mask pyramid is 1 where ALL 4^L level-0 bytes under
 * the pixel are non-zero and 0 otherwise (an AND, not a cascade of means), in the packed layout of hnet_align::level_offset.  A coarse template pixel whose
 * box mean mixes admitted and refused bytes is therefore never used, and the image pyramid needs no mask of its own.
 *
 * One linearisation is hnet_photo_robust.h's with one more condition in front: a template pixel whose mask byte at that level is 0 is skipped (takes_part);
 * it adds nothing to n_valid and nothing to n_outliers.  A mask without a zero byte leaves every sum, in its order, as it was.
 *
 * n_mask [L][slice]: the mask pixels of level L in the whole rows of row slice `slice` of 7 (32, 16, 8 and 4 rows at levels 0 - 3): where it is 0 the
 * slice has nothing to add.
 */
#ifndef HNET_PHOTO_MASKED_H
#define HNET_PHOTO_MASKED_H

#include "hnet_photo_robust.h"

namespace hnet_masked {

namespace pa = hnet_align;

constexpr int SLICES = 7;                                       /* the row slices of an accumulate launch */
constexpr int N_MASK = pa::MAX_LEVELS * SLICES;                 /* counts of one mask: [4][7] */
constexpr int slice_rows(int L) { return pa::level_h(L) / SLICES; }
static_assert(pa::level_h(3) % SLICES == 0, "whole rows per slice at every level");

/* one pixel of the next level of a mask: 1 iff all four are non-zero */
inline uint8_t and4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    HNET_ALIGN_NO_CONTRACT
    return (uint8_t)((a != 0u && b != 0u && c != 0u && d != 0u) ? 1 : 0);
}
/* the level above src (w x h, both even) into dst (w / 2 x h / 2); the AND of ANDs is the AND of all 4^L bytes */
inline void mask_down(const uint8_t* src, int w, int h, uint8_t* dst) {
    HNET_ALIGN_NO_CONTRACT
    for (int v = 0; v < h / 2; v++)
        for (int u = 0; u < w / 2; u++) {
            const uint8_t* p = src + (2 * v) * w + 2 * u;
            dst[v * (w / 2) + u] = and4(p[0], p[1], p[w], p[w + 1]);
        }
}
/* levels 1 .. 3 of mask0 into pyr [PYR_BYTES] */
inline void mask_pyramid(const uint8_t* mask0, uint8_t* pyr) {
    HNET_ALIGN_NO_CONTRACT
    const uint8_t* src = mask0;
    for (int L = 1; L < pa::MAX_LEVELS; L++) {
        uint8_t* dst = pyr + pa::level_offset(L);
        mask_down(src, pa::level_w(L - 1), pa::level_h(L - 1), dst);
        src = dst;
    }
}
/* level L of a mask: mask0 itself or its place in the packed pyramid */
inline const uint8_t* mask_level(const uint8_t* mask0, const uint8_t* pyr, int L) { return L == 0 ? mask0 : pyr + pa::level_offset(L); }
/* whether template pixel (u, v) of level L takes part; m: that level of the mask */
inline bool takes_part(const uint8_t* m, int L, int u, int v) {
    HNET_ALIGN_NO_CONTRACT
    return m[v * pa::level_w(L) + u] != 0;
}
/* n_mask [4][7] of a mask and its pyramid */
inline void mask_counts(const uint8_t* mask0, const uint8_t* pyr, int32_t* n_mask) {
    HNET_ALIGN_NO_CONTRACT
    for (int L = 0; L < pa::MAX_LEVELS; L++) {
        const uint8_t* m = mask_level(mask0, pyr, L);
        const int per = slice_rows(L) * pa::level_w(L);
        for (int s = 0; s < SLICES; s++) {
            int32_t c = 0;
            for (int i = 0; i < per; i++) c += m[s * per + i] != 0 ? 1 : 0;
            n_mask[L * SLICES + s] = c;
        }
    }
}

}  /* namespace hnet_masked */

#endif /* HNET_PHOTO_MASKED_H */
