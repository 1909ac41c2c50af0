/* hnet_photo_search.h — a start for the photometric alignment that needs no prediction (include/hnet.h hnet_op_photo_search,
 * hnet_sessions_photo_search, hnet_sessions_keyframe_relocalise): an exhaustive search over integer translations between two level-3
 * thumbnails, every shift scored by the zero-mean normalised cross-correlation on integer sums.  What the device (csrc/kernels_photo_search.hip) and the
 * host reference (tests/cpp/photo_search_ref.cpp) both compile, on top of include/hnet_photo_pyramid.h (down4).
 *
 * The thumbnail of a 320 x 224 u8 frame is level 3 of 7m's pyramid bit for bit, 40 x 28 u8: pixel (u, v) is the cascade (a + b + c + d + 2) >> 2 over the
 * 8 x 8 block at (8 u, 8 v): sixteen level-1 pixels, four of level 2, one of level 3 (thumb_pixel).
 * A shift (dx, dy) in level-3 pixels compares template pixel (u, v) of img1 with img2 at (u + dx, v + dy): the sense of H(x) everywhere in the tree, a
 * template pixel maps to its sampling position in img2.  The overlap is the set of (u, v) with both pixels inside; n its count; Sa, Sb, Sab, Saa, Sbb the
 * integer sums over it (at most 1120 * 255^2 < 2^27).  With every product and difference exact in int64:
 *   num = n Sab - Sa Sb, va = n Saa - Sa^2, vb = n Sbb - Sb^2; the shift is SCORED only when n >= min_overlap, va > 0 and vb > 0, and then
 *   score = (double) num / sqrt((double) va * (double) vb): three correctly rounded operations, so every implementation gives the same bits.
 * The best over the scored shifts with |dx| <= radius_x and |dy| <= radius_y: the highest score, then the smaller dx^2 + dy^2, then the smaller dy, then
 * the smaller dx: a total order, so the result does not depend on the order of a reduction.  `second` is the best by the same order among the scored
 * shifts with max(|dx - bx|, |dy - by|) > 1, -1 when there is none.
 * Flags, exactly one, tested in this order: NO_TEXTURE (no shift was scored: a constant thumbnail, or a min_overlap nothing meets), LOW_SCORE
 * (score < min_score), AMBIGUOUS (score - second < min_margin), else FOUND.  start_px is (8 dx, 8 dy) on all four corners when FOUND and quiet NaNs
 * otherwise: the value on which the alignment's kernels return at once.
 * Choices the rule left open.  Without a scored shift dx = dy = 0, score = -1 and the sums are zero; without a second dx2 = dy2 = 0.  The scores of a
 * search are kept as [41][61] doubles, index (dy + 20) * 61 + (dx + 30), quiet NaN where a shift is not scored or lies outside the radii.
 * Every body is non-contracting; sums are integers, scores are doubles, nothing depends on the batch.
 */
#ifndef HNET_PHOTO_SEARCH_H
#define HNET_PHOTO_SEARCH_H

#include <cstring>

#include "hnet_photo_pyramid.h"

namespace hnet_search {

namespace pa = hnet_align;

constexpr int TW = pa::level_w(3), TH = pa::level_h(3), TPIX = TW * TH;        /* 40 x 28 = 1120 */
constexpr int STEP = 8;                                                        /* full-resolution pixels per level-3 pixel */
constexpr int MAX_RX = 30, MAX_RY = 20, NSX = 2 * MAX_RX + 1, NSY = 2 * MAX_RY + 1, NSHIFT = NSX * NSY;    /* 61 x 41 = 2501 */
constexpr int MIN_MIN_OVERLAP = 16;
static_assert(TW == 40 && TH == 28 && MAX_RX < TW && MAX_RY < TH && NSHIFT == 2501, "every shift of the range leaves an overlap");

/* the flags of a search record (= HNET_PS_*) */
enum { FOUND = 1, NO_TEXTURE = 2, LOW_SCORE = 4, AMBIGUOUS = 8 };

/* = hnet_photo_search_opts */
struct Opts { int32_t radius_x, radius_y, min_overlap, pad; double min_score, min_margin; };
/* the defaults lie between the figures of a prototype on synthetic views; they are not calibrated on footage */
inline void default_opts(Opts& o) { o.radius_x = MAX_RX; o.radius_y = MAX_RY; o.min_overlap = 140; o.pad = 0; o.min_score = 0.75; o.min_margin = 0.1; }
inline bool opts_valid(const Opts& o) {
    return o.radius_x >= 0 && o.radius_x <= MAX_RX && o.radius_y >= 0 && o.radius_y <= MAX_RY && o.min_overlap >= MIN_MIN_OVERLAP && o.min_overlap <= TPIX &&
           o.min_score >= -1.0 && o.min_score <= 1.0 && o.min_margin >= 0.0 && o.min_margin <= 2.0;      /* (false for NaN) */
}

/* the integer sums of one shift */
struct Sums { int32_t n, sa, sb, sab, saa, sbb; };

/* = hnet_photo_search */
struct Record {
    float start_px[pa::NX];
    int32_t dx, dy, dx2, dy2, n_overlap, flags;
    double score, second;
    int32_t sa, sb, sab, saa, sbb, pad;
};

inline float quiet_nan_f() {
    const uint32_t u = 0x7fc00000u;
    float f;
    std::memcpy(&f, &u, sizeof f);
    return f;
}
inline double quiet_nan_d() {
    const uint64_t u = 0x7ff8000000000000ull;
    double d;
    std::memcpy(&d, &u, sizeof d);
    return d;
}

/* thumbnail pixel (u, v) of a frame of PYR_W0 x PYR_H0 bytes: the cascade over its 8 x 8 block */
inline uint8_t thumb_pixel(const uint8_t* img, int u, int v) {
    HNET_ALIGN_NO_CONTRACT
    const uint8_t* p = img + (size_t)(STEP * v) * pa::PYR_W0 + STEP * u;
    uint32_t l2[4];
    for (int j = 0; j < 2; j++)
        for (int i = 0; i < 2; i++) {
            uint32_t l1[4];
            for (int b = 0; b < 2; b++)
                for (int a = 0; a < 2; a++) {
                    const uint8_t* q = p + (4 * j + 2 * b) * pa::PYR_W0 + 4 * i + 2 * a;
                    l1[2 * b + a] = pa::down4(q[0], q[1], q[pa::PYR_W0], q[pa::PYR_W0 + 1]);
                }
            l2[2 * j + i] = pa::down4(l1[0], l1[1], l1[2], l1[3]);
        }
    return pa::down4(l2[0], l2[1], l2[2], l2[3]);
}

inline void thumbnail(const uint8_t* img, uint8_t* out) {
    for (int v = 0; v < TH; v++)
        for (int u = 0; u < TW; u++) out[v * TW + u] = thumb_pixel(img, u, v);
}

/* the index of a shift of the full range in a score table, and back */
inline int shift_index(int dx, int dy) { return (dy + MAX_RY) * NSX + (dx + MAX_RX); }
inline void index_shift(int i, int& dx, int& dy) { dy = i / NSX - MAX_RY; dx = i % NSX - MAX_RX; }

/* the overlap of a shift: template columns u0 .. u1 - 1, rows v0 .. v1 - 1 (non-empty for every shift of the range) */
inline void overlap(int dx, int dy, int& u0, int& u1, int& v0, int& v1) {
    u0 = dx < 0 ? -dx : 0; u1 = dx > 0 ? TW - dx : TW;
    v0 = dy < 0 ? -dy : 0; v1 = dy > 0 ? TH - dy : TH;
}

/* the sums of one shift with |dx| <= MAX_RX, |dy| <= MAX_RY, pixels in ascending order */
inline void shift_sums(const uint8_t* a, const uint8_t* b, int dx, int dy, Sums& s) {
    HNET_ALIGN_NO_CONTRACT
    int u0, u1, v0, v1;
    overlap(dx, dy, u0, u1, v0, v1);
    int32_t sa = 0, sb = 0, sab = 0, saa = 0, sbb = 0;
    for (int v = v0; v < v1; v++)
        for (int u = u0; u < u1; u++) {
            const int32_t p = a[v * TW + u], q = b[(v + dy) * TW + (u + dx)];
            sa += p; sb += q; sab += p * q; saa += p * p; sbb += q * q;
        }
    s.n = (u1 - u0) * (v1 - v0); s.sa = sa; s.sb = sb; s.sab = sab; s.saa = saa; s.sbb = sbb;
}

/* whether the shift is scored, and its score */
inline bool shift_score(const Sums& s, int min_overlap, double& score) {
    HNET_ALIGN_NO_CONTRACT
    const int64_t n = s.n, sa = s.sa, sb = s.sb;
    const int64_t num = n * (int64_t)s.sab - sa * sb, va = n * (int64_t)s.saa - sa * sa, vb = n * (int64_t)s.sbb - sb * sb;
    if (s.n < min_overlap || va <= 0 || vb <= 0) return false;
    const double den = std::sqrt((double)va * (double)vb);
    score = (double)num / den;
    return true;
}

/* the total order: whether scored shift i (score si) is better than scored shift j */
inline bool better(double si, int i, double sj, int j) {
    HNET_ALIGN_NO_CONTRACT
    if (si != sj) return si > sj;
    int xi, yi, xj, yj;
    index_shift(i, xi, yi);
    index_shift(j, xj, yj);
    const int ri = xi * xi + yi * yi, rj = xj * xj + yj * yj;
    if (ri != rj) return ri < rj;
    if (yi != yj) return yi < yj;
    return xi < xj;
}

/* a candidate of a reduction: index -1 = none.  offer keeps the better of two; it is associative and commutative. */
struct Best { double score; int32_t index; };
inline void best_none(Best& b) { b.score = -1.0; b.index = -1; }
inline void offer(Best& b, double score, int index) {
    if (index < 0 || score != score) return;                 /* (a NaN in the table: not scored) */
    if (b.index < 0 || better(score, index, b.score, b.index)) { b.score = score; b.index = index; }
}
/* whether shift i lies outside the 3 x 3 around shift `around` */
inline bool outside3(int i, int around) {
    int xi, yi, xa, ya;
    index_shift(i, xi, yi);
    index_shift(around, xa, ya);
    const int ex = xi > xa ? xi - xa : xa - xi, ey = yi > ya ? yi - ya : ya - yi;
    return ex > 1 || ey > 1;
}

/* the record of a search from its best, its second and the best's sums (zeros without a best): every byte is written */
inline void finish(const Best& best, const Best& second, const Sums& s, const Opts& o, Record& r) {
    HNET_ALIGN_NO_CONTRACT
    r.dx = r.dy = r.dx2 = r.dy2 = 0;
    r.n_overlap = 0;
    r.score = -1.0;
    r.second = -1.0;
    r.sa = r.sb = r.sab = r.saa = r.sbb = 0;
    r.pad = 0;
    if (best.index < 0) {
        r.flags = NO_TEXTURE;
    } else {
        index_shift(best.index, r.dx, r.dy);
        r.score = best.score;
        r.n_overlap = s.n; r.sa = s.sa; r.sb = s.sb; r.sab = s.sab; r.saa = s.saa; r.sbb = s.sbb;
        if (second.index >= 0) {
            index_shift(second.index, r.dx2, r.dy2);
            r.second = second.score;
        }
        if (r.score < o.min_score) r.flags = LOW_SCORE;
        else if (r.score - r.second < o.min_margin) r.flags = AMBIGUOUS;
        else r.flags = FOUND;
    }
    for (int c = 0; c < 4; c++) {
        r.start_px[2 * c] = r.flags == FOUND ? (float)(STEP * r.dx) : quiet_nan_f();
        r.start_px[2 * c + 1] = r.flags == FOUND ? (float)(STEP * r.dy) : quiet_nan_f();
    }
}

/* the score table [NSHIFT] of two thumbnails: quiet NaN where a shift is not scored or lies outside the radii */
inline void score_table(const uint8_t* a, const uint8_t* b, const Opts& o, double* scores) {
    for (int i = 0; i < NSHIFT; i++) {
        int dx, dy;
        index_shift(i, dx, dy);
        Sums s;
        double sc;
        const bool in = dx >= -o.radius_x && dx <= o.radius_x && dy >= -o.radius_y && dy <= o.radius_y;
        if (in) shift_sums(a, b, dx, dy, s);
        scores[i] = in && shift_score(s, o.min_overlap, sc) ? sc : quiet_nan_d();
    }
}

/* the whole search of two thumbnails on the host: scores [NSHIFT] is written */
inline void search(const uint8_t* a, const uint8_t* b, const Opts& o, Record& r, double* scores) {
    score_table(a, b, o, scores);
    Best best, second;
    Sums s = {0, 0, 0, 0, 0, 0};
    best_none(best);
    best_none(second);
    for (int i = 0; i < NSHIFT; i++) offer(best, scores[i], i);
    if (best.index >= 0) {
        int dx, dy;
        index_shift(best.index, dx, dy);
        shift_sums(a, b, dx, dy, s);
        for (int i = 0; i < NSHIFT; i++)
            if (outside3(i, best.index)) offer(second, scores[i], i);
    }
    finish(best, second, s, o, r);
}

}  /* namespace hnet_search */

#endif /* HNET_PHOTO_SEARCH_H */
