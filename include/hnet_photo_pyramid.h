/* hnet_photo_pyramid.h — the image pyramid of coarse-to-fine photometric alignment (include/hnet.h hnet_op_photo_align_pyramid), dependency
 * free: what the device (csrc/kernels_photo_pyramid.hip) and the host reference (tests/cpp/photo_align_pyr_ref.cpp) both compile, next to
 * include/hnet_photo_align.h, whose sums, reduction and Levenberg-Marquardt step serve every level unchanged.
 *
 * The pyramid.  Level 0 is the 320 x 224 u8 frame; level L + 1 is the 2 x 2 box mean of level L, rounded to nearest in integers:
 * (a + b + c + d + 2) >> 2, cascaded (level 2 is made from the ROUNDED level 1).  Integer arithmetic: the host and the device agree bit for bit.
 * The centre of level-L pixel (u, v) in level-0 coordinates is (s u + c, s v + c), s = 2^L, c = (s - 1) / 2: an exact half-integer in fp32.
 *
 * One linearisation at level L keeps the offsets x in FULL-RESOLUTION pixels and H = (float) dlt_solve(p4 + x).  Level-L pixel (u, v) sits at
 * (fu, fv) = (s u + c, s v + c); (ix0, iy0, Z) are the warp's own expressions at (fu, fv) (level_coords), the position in the level-L image is
 * ix = (ix0 - c) / s, and the pixel is VALID when 0 <= ix < W_L - 1 and 0 <= iy < H_L - 1.  The taps, w and r are those of level 0 on the level-L images;
 * the gradient is taken per full-resolution pixel (x 1 / s) and the row s[9] is formed as at level 0 with (fu, fv) for (u, v) and (ix0, iy0) in q.
 * At L = 0 every added operation is exact (x 1, - 0): level 0 is, bit for bit, the quantity of include/hnet_photo_align.h.
 */
#ifndef HNET_PHOTO_PYRAMID_H
#define HNET_PHOTO_PYRAMID_H

#include "hnet_photo_align.h"

namespace hnet_align {

constexpr int MAX_LEVELS = 4;
constexpr int PYR_W0 = 320, PYR_H0 = 224;
constexpr int level_w(int L) { return PYR_W0 >> L; }
constexpr int level_h(int L) { return PYR_H0 >> L; }
constexpr int level_pix(int L) { return level_w(L) * level_h(L); }
/* levels 1, 2, 3 of one frame, packed: 17 920 + 4 480 + 1 120 bytes; every level starts at a multiple of 16 */
constexpr int PYR_BYTES = level_pix(1) + level_pix(2) + level_pix(3);
constexpr int level_offset(int L) { return L <= 1 ? 0 : (L == 2 ? level_pix(1) : level_pix(1) + level_pix(2)); }
static_assert(PYR_BYTES == 23520 && level_offset(2) % 16 == 0 && level_offset(3) % 16 == 0 && PYR_BYTES % 16 == 0 && PYR_H0 % 8 == 0 && PYR_W0 % 8 == 0,
              "three whole levels, 16-byte aligned");

/* one pixel of the next level; at most (4 * 255 + 2) >> 2 = 255 */
inline uint8_t down4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    HNET_ALIGN_NO_CONTRACT
    return (uint8_t)((a + b + c + d + 2u) >> 2);
}
/* the level above src (w x h, both even) into dst (w / 2 x h / 2) */
inline void downsample(const uint8_t* src, int w, int h, uint8_t* dst) {
    HNET_ALIGN_NO_CONTRACT
    for (int v = 0; v < h / 2; v++)
        for (int u = 0; u < w / 2; u++) {
            const uint8_t* p = src + (2 * v) * w + 2 * u;
            dst[v * (w / 2) + u] = down4(p[0], p[1], p[w], p[w + 1]);
        }
}

/* s, c and 1 / s of a level: powers of two and half-integers, exact */
inline float level_scale(int L) { HNET_ALIGN_NO_CONTRACT return (float)(1 << L); }
inline float level_shift(int L) { HNET_ALIGN_NO_CONTRACT return (float)((1 << L) - 1) * 0.5f; }
inline float level_inv_scale(int L) { HNET_ALIGN_NO_CONTRACT return 1.0f / (float)(1 << L); }
/* the centre of level-L pixel index u in level-0 coordinates */
inline float level_centre(int L, int u) { HNET_ALIGN_NO_CONTRACT return fmaf((float)u, level_scale(L), level_shift(L)); }
/* min_valid of a call at level L: a level has 4^-L of the pixels (step() still floors it at 9) */
inline int32_t level_min_valid(int32_t min_valid, int L) { HNET_ALIGN_NO_CONTRACT return min_valid >> (2 * L); }

/* warp_coords' (csrc/warp_dev.h) expressions at the float position (fu, fv): the same FMA chain, the division the caller supplies (div(X, Y, Z, qx, qy):
 * IEEE quotients; the device's reciprocal form is bit-identical to them), the same normalise / un-normalise with 319 and 223 */
template <typename DIV>
inline void level_coords(const float* h, float fu, float fv, DIV div, float& ix0, float& iy0, float& Z) {
    HNET_ALIGN_NO_CONTRACT
    const float X = fmaf(h[0], fu, fmaf(h[1], fv, h[2]));
    const float Y = fmaf(h[3], fu, fmaf(h[4], fv, h[5]));
    Z = fmaf(h[6], fu, fmaf(h[7], fv, h[8]));
    float qx, qy;
    div(X, Y, Z, qx, qy);
    const float gx = fmaf(qx, (float)(2.0 / (PYR_W0 - 1)), -1.0f);
    const float gy = fmaf(qy, (float)(2.0 / (PYR_H0 - 1)), -1.0f);
    ix0 = ((gx + 1.0f) * 0.5f) * (float)(PYR_W0 - 1);
    iy0 = ((gy + 1.0f) * 0.5f) * (float)(PYR_H0 - 1);
}

/* the position in the level-L image and whether all four taps are pixels of it (false for NaN) */
inline bool level_position(int L, float ix0, float iy0, float& ix, float& iy) {
    HNET_ALIGN_NO_CONTRACT
    const float c = level_shift(L), is = level_inv_scale(L);
    ix = (ix0 - c) * is;
    iy = (iy0 - c) * is;
    return ix >= 0.0f && ix < (float)(level_w(L) - 1) && iy >= 0.0f && iy < (float)(level_h(L) - 1);
}

/* residual r (grey levels of the level's images) and the row s of dr / dvec(H) of a VALID pixel: a b / c d the four taps at (floor ix, floor iy) and i1 the
 * level-L img1 pixel, all as u8 / 255; every operation is written out, one rounding each */
inline void level_row(int L, float a, float b, float c, float d, float i1, float ix, float iy, float ix0, float iy0, float Z, float fu, float fv, float& r,
                      float s[NH]) {
    HNET_ALIGN_NO_CONTRACT
    const float is = level_inv_scale(L);
    const float x0f = floorf(ix), y0f = floorf(iy);
    const float wx1 = ix - x0f, wx0 = 1.0f - wx1, wy1 = iy - y0f, wy0 = 1.0f - wy1;
    float w = fmaf(a, wx0 * wy0, 0.0f);
    w = fmaf(b, wx1 * wy0, w);
    w = fmaf(c, wx0 * wy1, w);
    w = fmaf(d, wx1 * wy1, w);
    r = (w - i1) * 255.0f;
    const float gx = fmaf(d - c, wy1, (b - a) * wy0) * 255.0f * is;
    const float gy = fmaf(d - b, wx1, (c - a) * wx0) * 255.0f * is;
    const float q = fmaf(gx, ix0, gy * iy0);
    const float rz = 1.0f / Z, au = fu * rz, av = fv * rz;
    s[0] = gx * au; s[1] = gx * av; s[2] = gx * rz;
    s[3] = gy * au; s[4] = gy * av; s[5] = gy * rz;
    s[6] = -q * au; s[7] = -q * av; s[8] = -q * rz;
}

}  /* namespace hnet_align */

#endif /* HNET_PHOTO_PYRAMID_H */
