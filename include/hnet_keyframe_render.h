/* hnet_keyframe_render.h — a session's keyframe map RENDERED into one view (include/hnet.h hnet_op_keyframe_render, hnet_sessions_keyframe_render;
 * DESIGN 7ab): where a pixel of the view samples each stored keyframe, the bilinear tap, the blend of the samples that cover a pixel and the integer
 * seam statistics of the overlaps.  What the device (csrc/kernels_keyframe_render.hip) and the host reference (tests/cpp/keyframe_render_ref.cpp) both
 * compile, on top of include/hnet_keyframe_map.h (Entry, the conventions: H_a->b maps a pixel of a to its position in b).
 *
 * A view is a width x height u8 image with h_origin_view (origin -> view, h[8] = 1).
 *
 * render_setup(h_origin_view, entry, S) -> bool: S = entry.h_origin_key . inverse(h_origin_view), renormalised to S[8] = 1 (hnet_keyframe::chain): S maps
 *   a pixel of the view to its sampling position in the stored keyframe.  The inverse is hnet_keyframe_map::inverse, the one relative calls: false when
 *   |det| is below ORIGIN_TINY times the cube of the largest entry in frame units.  False too when the entry is not valid, when h_origin_key fails the
 *   same test (its S would map the view onto a line), when the product is degenerate or anything is not finite.
 * render_sample(S, img, u, v, val) -> bool: (X, Y, Z) = S (u, v, 1) in double, each as (S0 u + S1 v) + S2; x = X / Z, y = Y / Z.  Invalid unless Z > 0,
 *   x and y are finite, 0 <= x <= 319 and 0 <= y <= 223.  x0 = floor(x), x1 = min(x0 + 1, 319), fx = (float)(x - x0), the same in y.  The blend, in float
 *   and in THIS order (nothing contracted):
 *       top = a00 + fx * (a01 - a00)      a00 = img[y0][x0], a01 = img[y0][x1]
 *       bot = a10 + fx * (a11 - a10)      a10 = img[y1][x0], a11 = img[y1][x1]
 *       b   = top + fy * (bot - top)
 *   val = (uint8) floor(b + 0.5f).  Every partial result lies between two bytes, so val needs no clamp.  At x = 319 the second tap is the first with
 *   weight 0.
 * render_pixel(vals, mask, links, serial, mode, cover) -> the output byte.  vals packs the samples v_j of the M entries (byte j), mask their validity;
 *   cover = popcount(mask).  FEWEST_LINKS: the covering entry with the fewest links, then the lower slot (select's preference: the least-drifted ground).
 *   NEWEST: the covering entry with the largest serial, then the lower slot.  MEAN: (sum + cover / 2) / cover in integers.  Uncovered: 0.
 * seam_add(vals, mask, out, n, sse): for a pixel with cover >= 2, every covering entry j adds 1 to n[j] and (v_j - out)^2 to sse[j].  Integers only: any
 *   order of reduction gives the same bits (7g's rule).  A Counters block also keeps n_covered (cover >= 1) and n_overlap (cover >= 2).
 * render_fit_view(entries, capacity, width, height, margin_px, h_origin_view) -> bool, host side, in double: the corners p4 of every valid entry taken
 *   back to the origin frame through inverse(h_origin_key), their bounding box, and the uniform scale and translation that centre the box in
 *   [margin, width - 1 - margin] x [margin, height - 1 - margin].  False without a usable entry, for a box or a drawing area without extent, for a
 *   corner with z <= 0 or anything not finite.
 * Choices the rule left open.  skipped_mask holds EVERY slot below the capacity whose setup failed, the invalid ones included: a map without a valid
 *   entry renders zeros and a record that is zero but for the view and skipped_mask.  used_mask holds the slots whose setup succeeded, whether or not
 *   they cover a pixel.  S is renormalised like every composed homography of the tree, so a product whose [8] is negative flips the sign of Z: such a
 *   view looks at the keyframe from behind and the rule does not promise it.  render_fit_view leaves out a valid entry whose h_origin_key has no inverse
 *   (the render skips it too).  Equal serials cannot occur in a session's map; hnet_op_keyframe_render takes what it is given and the lower slot wins.
 * Every body is non-contracting, nothing depends on the batch or the slot of the call.
 */
#ifndef HNET_KEYFRAME_RENDER_H
#define HNET_KEYFRAME_RENDER_H

#include "hnet_keyframe_map.h"

namespace hnet_keyframe_render {

namespace kf = hnet_keyframe;
namespace km = hnet_keyframe_map;

constexpr int KEY_W = 320, KEY_H = 224, KEY_PIXELS = KEY_W * KEY_H;
constexpr int MAX_ENTRIES = km::MAX_CAPACITY;          /* a render takes 1 .. 8 entries */
constexpr int MAX_DIM = 8192;                          /* the largest width or height of a view */

/* = HNET_RENDER_* */
enum { FEWEST_LINKS = 0, NEWEST = 1, MEAN = 2, N_MODES = 3 };

/* = hnet_keyframe_render_opts */
struct Opts { int32_t width, height, mode, pad; };
inline bool opts_valid(const Opts& o) {
    return o.width >= 1 && o.width <= MAX_DIM && o.height >= 1 && o.height <= MAX_DIM && o.mode >= 0 && o.mode < N_MODES;
}

/* = hnet_keyframe_render_rec: the view that was rendered, the counters (the layout of Counters) and the masks */
struct Counters { uint64_t n_covered, n_overlap, n[MAX_ENTRIES], sse[MAX_ENTRIES]; };
struct Record { double h_origin_view[9]; Counters c; int32_t used_mask, skipped_mask; };

/* false: S holds nothing to be used */
inline bool render_setup(const double h_origin_view[9], const km::Entry& e, double S[9]) {
    HNET_ALIGN_NO_CONTRACT
    double inv[9];
    if (e.valid == 0 || !km::inverse(e.h_origin_key, inv)) return false;    /* (a singular h_origin_key: S would map the view onto a line) */
    if (!km::inverse(h_origin_view, inv)) return false;
    for (int k = 0; k < 9; k++)
        if (!std::isfinite(inv[k])) return false;
    return kf::chain(e.h_origin_key, inv, S);
}

/* img: one stored keyframe [224][320]; false: the view pixel (u, v) does not fall inside it (val untouched) */
inline bool render_sample(const double S[9], const uint8_t* img, int u, int v, uint8_t& val) {
    HNET_ALIGN_NO_CONTRACT
    const double du = (double)u, dv = (double)v;
    const double X = (S[0] * du + S[1] * dv) + S[2], Y = (S[3] * du + S[4] * dv) + S[5], Z = (S[6] * du + S[7] * dv) + S[8];
    const double x = X / Z, y = Y / Z;
    if (!(Z > 0.0 && std::isfinite(x) && std::isfinite(y) && x >= 0.0 && x <= (double)(KEY_W - 1) && y >= 0.0 && y <= (double)(KEY_H - 1))) return false;
    const double xf = std::floor(x), yf = std::floor(y);
    const int x0 = (int)xf, y0 = (int)yf;
    const int x1 = x0 + 1 < KEY_W - 1 ? x0 + 1 : KEY_W - 1, y1 = y0 + 1 < KEY_H - 1 ? y0 + 1 : KEY_H - 1;
    const float fx = (float)(x - xf), fy = (float)(y - yf);
    const float a00 = (float)img[y0 * KEY_W + x0], a01 = (float)img[y0 * KEY_W + x1], a10 = (float)img[y1 * KEY_W + x0], a11 = (float)img[y1 * KEY_W + x1];
    const float top = a00 + fx * (a01 - a00);
    const float bot = a10 + fx * (a11 - a10);
    const float b = top + fy * (bot - top);
    val = (uint8_t)(int)std::floor(b + 0.5f);
    return true;
}

/* byte j of vals */
inline int sample_of(uint64_t vals, int j) { return (int)((vals >> (8 * j)) & 0xffu); }

/* the output byte of one pixel and its cover; links / serial: the entries', by slot (read for the bits of mask only) */
inline uint8_t render_pixel(uint64_t vals, int mask, const int32_t* links, const int32_t* serial, int mode, int& cover) {
    int n = 0, sum = 0, best = -1;
    for (int j = 0; j < MAX_ENTRIES; j++) {
        if (!((mask >> j) & 1)) continue;
        n++;
        sum += sample_of(vals, j);
        if (best < 0 || (mode == NEWEST ? serial[j] > serial[best] : links[j] < links[best])) best = j;
    }
    cover = n;
    if (n == 0) return 0;
    if (mode == MEAN) return (uint8_t)((sum + n / 2) / n);
    return (uint8_t)sample_of(vals, best);
}

/* the seam statistics of one pixel with cover >= 2 (the caller tests the cover); C: any unsigned integer wide enough for what the caller sums */
template <typename C>
inline void seam_add(uint64_t vals, int mask, int out, C* n, C* sse) {
    for (int j = 0; j < MAX_ENTRIES; j++) {
        if (!((mask >> j) & 1)) continue;
        const int d = sample_of(vals, j) - out;
        n[j] += (C)1;
        sse[j] += (C)(d * d);
    }
}

/* one pixel of a view of M entries with the setups S [M][9] (ok_mask: those that succeeded) and images [M][71 680]: the output byte, the cover, and
 * the counters advanced.  The host reference's whole pixel; the device runs the same three functions with the table in LDS. */
inline uint8_t render_one(const double* S, int ok_mask, const uint8_t* images, const int32_t* links, const int32_t* serial, int M, int mode, int u, int v,
                          uint8_t& cover_out, Counters& c) {
    uint64_t vals = 0;
    int mask = 0, cover = 0;
    for (int j = 0; j < M; j++) {
        uint8_t val = 0;
        if (!((ok_mask >> j) & 1) || !render_sample(S + 9 * j, images + (size_t)j * KEY_PIXELS, u, v, val)) continue;
        vals |= (uint64_t)val << (8 * j);
        mask |= 1 << j;
    }
    const uint8_t out = render_pixel(vals, mask, links, serial, mode, cover);
    cover_out = (uint8_t)cover;
    if (cover >= 1) c.n_covered++;
    if (cover >= 2) {
        c.n_overlap++;
        seam_add(vals, mask, (int)out, c.n, c.sse);
    }
    return out;
}

/* host side */
inline bool render_fit_view(const km::Entry* e, int capacity, int width, int height, double margin_px, double h_origin_view[9]) {
    HNET_ALIGN_NO_CONTRACT
    const double aw = ((double)(width - 1) - margin_px) - margin_px, ah = ((double)(height - 1) - margin_px) - margin_px;
    if (!e || capacity < 1 || !std::isfinite(margin_px) || margin_px < 0.0 || !(aw > 0.0) || !(ah > 0.0)) return false;
    double lo[2] = {0.0, 0.0}, hi[2] = {0.0, 0.0};
    int used = 0;
    for (int j = 0; j < capacity; j++) {
        double inv[9];
        if (!e[j].valid || !km::inverse(e[j].h_origin_key, inv)) continue;
        for (int c = 0; c < 4; c++) {
            const double u = hnet::p4(2 * c), v = hnet::p4(2 * c + 1);
            const double X = (inv[0] * u + inv[1] * v) + inv[2], Y = (inv[3] * u + inv[4] * v) + inv[5], Z = (inv[6] * u + inv[7] * v) + inv[8];
            const double p[2] = {X / Z, Y / Z};
            if (!(Z > 0.0) || !std::isfinite(p[0]) || !std::isfinite(p[1])) return false;
            for (int a = 0; a < 2; a++) {
                if (!used || p[a] < lo[a]) lo[a] = p[a];
                if (!used || p[a] > hi[a]) hi[a] = p[a];
            }
            used++;
        }
    }
    const double bw = hi[0] - lo[0], bh = hi[1] - lo[1];
    if (!used || !(bw > 0.0) || !(bh > 0.0) || !std::isfinite(bw) || !std::isfinite(bh)) return false;
    const double sx = aw / bw, sy = ah / bh, s = sx < sy ? sx : sy;
    const double tx = (margin_px + (aw - s * bw) / 2.0) - s * lo[0], ty = (margin_px + (ah - s * bh) / 2.0) - s * lo[1];
    if (!(s > 0.0) || !std::isfinite(s) || !std::isfinite(tx) || !std::isfinite(ty)) return false;
    const double h[9] = {s, 0.0, tx, 0.0, s, ty, 0.0, 0.0, 1.0};
    for (int k = 0; k < 9; k++) h_origin_view[k] = h[k];
    return true;
}

}  /* namespace hnet_keyframe_render */

#endif /* HNET_KEYFRAME_RENDER_H */
