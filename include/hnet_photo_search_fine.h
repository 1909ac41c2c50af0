/* hnet_photo_search_fine.h — a second, fine stage of the search around the winner of include/hnet_photo_search_oriented.h (include/hnet.h
 * hnet_op_photo_search_fine, hnet_sessions_photo_search_fine, hnet_sessions_keyframe_relocalise_fine): a handful of sub-step orientation
 * entries around the winning entry, on LEVEL-2 thumbnails, over the shifts of +-r level-2 pixels around twice the winning shift.  What the device
 * (csrc/kernels_photo_search_fine.hip) and the host reference (tests/cpp/photo_search_fine_ref.cpp) both compile, on top of the unedited coarse headers.
 *
 * The level-2 thumbnail of a 320 x 224 u8 frame is level 2 of 7m's pyramid bit for bit, 80 x 56 u8: pixel (u, v) is the down4 cascade over the 4 x 4 block
 * at (4u, 4v).  Its grid centre (39.5, 27.5) times 4 plus 1.5 is the frame centre c = (159.5, 111.5), 7s's c.
 * The fine table is fine[n_hyp][n_fine] entries of 7s's Hyp, 1 <= n_fine <= 9; row h belongs to coarse entry h and only the winner's row is read.  Every
 * entry must pass hyp_valid.  fine_yaw_table (host only) fills [h][j] with make_hyp at (first_deg + h step_deg) + ((double) j - (n_fine - 1) / 2.0) *
 * (step_deg / n_fine) degrees, scale 1: for odd n_fine the middle entry has the coarse entry's bits.
 * The warp is 7s's integer warp with the level-2 constants: q = (2u - 79, 2v - 55), sx = b00 qx + b01 qy + (79 << 16), sy = b10 qx + b11 qy + (55 << 16)
 * (|.| <= 2^17 (79 + 55) + 79 2^16 < 2^25), ix, fx, the validity test, the bilinear value and the mask as there with 79 / 55 in place of 39 / 27.
 * For the coarse shift (dx, dy) and |ex|, |ey| <= r, 0 <= r <= 4, the level-2 shift is (2 dx + ex, 2 dy + ey): |.| <= 64 < 80 and 44 < 56, so every shift
 * leaves an overlap.  The masked sums are 7s's six, each at most 4480 * 255^2 < 2^31; a shift is scored by hnet_search::shift_score with 4 * min_overlap of
 * the coarse options: the same share of the area.
 * The best over (entry j, ex, ey): the highest score, then the smaller ex^2 + ey^2, then the smaller ey, then the smaller ex, then the lower j: a total
 * order, so the result does not depend on the order of a reduction.  A candidate is the index j * 81 + (ey + 4) * 9 + (ex + 4).
 * Flags, exactly one, tested in this order: FINE_SKIPPED (the coarse record is not FOUND), FINE_NOTHING_SCORED, FINE_LOW_SCORE (the best fine score is
 * below min_score), else FINE_REFINED.  The final start: REFINED, at corner x_i, ((c + A_f (x_i - c)) + 4 (sx, sy)) - x_i in double in start_of's order,
 * rounded to float once; NOTHING_SCORED or LOW_SCORE, the coarse start_px unchanged; SKIPPED, quiet NaNs.  Scores of the two levels are never compared.
 * Choices the rule left open: the "none" values.  SKIPPED and NOTHING_SCORED: j = -1, ex = ey = 0, sx = sy = 0, n_overlap = 0, score = -1, a and the sums
 * zero.  LOW_SCORE reports the rejected best in full.  min_score defaults to the coarse default 0.75 and is NOT calibrated for level 2.
 * The scores of a call are [n_fine][9][9] doubles per pair, index (ey + 4) * 9 + (ex + 4), quiet NaN where a shift is not scored or lies outside r, and
 * all quiet NaN for a SKIPPED pair.  Every body is non-contracting; sums are integers, scores are doubles.
 */
#ifndef HNET_PHOTO_SEARCH_FINE_H
#define HNET_PHOTO_SEARCH_FINE_H

#include "hnet_photo_search_oriented.h"

namespace hnet_search_fine {

namespace pa = hnet_align;
namespace ps = hnet_search;
namespace po = hnet_search_oriented;

constexpr int FW = pa::level_w(2), FH = pa::level_h(2), FPIX = FW * FH;        /* 80 x 56 = 4480 */
constexpr int FSTEP = 4;                                                       /* full-resolution pixels per level-2 pixel */
constexpr int MAX_FINE = 9, MAX_R = 4, NE = 2 * MAX_R + 1, NSHIFT = NE * NE;   /* 9 x 9 = 81 shifts per entry */
constexpr int MAX_SX = 2 * ps::MAX_RX + MAX_R, MAX_SY = 2 * ps::MAX_RY + MAX_R;
static_assert(FW == 80 && FH == 56 && FPIX == 4480 && FW == 2 * ps::TW && FH == 2 * ps::TH && MAX_SX == 64 && MAX_SY == 44 && MAX_SX < FW && MAX_SY < FH,
              "every level-2 shift leaves an overlap");
static_assert((int64_t)po::MAX_B * ((FW - 1) + (FH - 1)) + (int64_t)(FW - 1) * po::ONE < ((int64_t)1 << 25), "sx and sy stay below 2^25 in magnitude");
static_assert((int64_t)FPIX * 255 * 255 < ((int64_t)1 << 31), "the sums are int32");

/* the flags of the fine part (= HNET_PSF_*) */
enum { FINE_REFINED = 1, FINE_SKIPPED = 2, FINE_NOTHING_SCORED = 4, FINE_LOW_SCORE = 8 };

/* = hnet_photo_search_fine_opts */
struct Opts { int32_t radius, n_fine; double min_score; int32_t pad[2]; };
/* min_score is the coarse default: it is not calibrated for level 2 */
inline void default_opts(Opts& o) { o.radius = 3; o.n_fine = 5; o.min_score = 0.75; o.pad[0] = o.pad[1] = 0; }
inline bool opts_valid(const Opts& o) {
    return o.radius >= 0 && o.radius <= MAX_R && o.n_fine >= 1 && o.n_fine <= MAX_FINE && o.min_score >= -1.0 && o.min_score <= 1.0;       /* (false for NaN) */
}

/* the fine part of a record (= hnet_photo_search_fine_part) */
struct Part {
    float start_px[pa::NX];    /* the FINAL start */
    int32_t flags;             /* FINE_* */
    int32_t j, ex, ey;         /* the best fine entry and its offsets from twice the coarse shift */
    int32_t sx, sy;            /* the level-2 shift (2 dx + ex, 2 dy + ey) */
    int32_t n_overlap, pad0;
    double score;
    double a[4];               /* the fine entry's matrix */
    int32_t sa, sb, sab, saa, sbb, pad1;
};
/* = hnet_photo_search_fine */
struct Record { po::Record coarse; Part fine; };
static_assert(sizeof(Opts) == 24 && sizeof(Part) == 128 && sizeof(Record) == 288 && offsetof(Record, fine) == 160 && offsetof(Part, flags) == 32 &&
                  offsetof(Part, j) == 36 && offsetof(Part, ex) == 40 && offsetof(Part, ey) == 44 && offsetof(Part, sx) == 48 && offsetof(Part, sy) == 52 &&
                  offsetof(Part, n_overlap) == 56 && offsetof(Part, pad0) == 60 && offsetof(Part, score) == 64 && offsetof(Part, a) == 72 &&
                  offsetof(Part, sa) == 104 && offsetof(Part, pad1) == 124,
              "the layout of hnet_photo_search_fine");

/* what one fine entry hands to the winner: its best candidate (index -1: none) and that shift's sums */
struct Entry { double score; int32_t index, pad; ps::Sums s; };
static_assert(sizeof(Entry) == 40, "packed");

/* [count][n_fine] entries around the count entries of po::yaw_table(first_deg, step_deg, count): host only */
inline bool fine_yaw_table(double first_deg, double step_deg, int count, int n_fine, po::Hyp* out) {
    HNET_ALIGN_NO_CONTRACT
    if (count < 1 || count > po::MAX_HYP || n_fine < 1 || n_fine > MAX_FINE || !std::isfinite(first_deg) || !std::isfinite(step_deg)) return false;
    for (int h = 0; h < count; h++)
        for (int j = 0; j < n_fine; j++) {
            const double deg = (first_deg + (double)h * step_deg) + ((double)j - (double)(n_fine - 1) / 2.0) * (step_deg / (double)n_fine);
            if (!po::make_hyp(deg * (3.14159265358979323846 / 180.0), 1.0, out[h * n_fine + j])) return false;
        }
    return true;
}
inline bool fine_table_valid(const po::Hyp* f, int n_hyp, int n_fine) {
    if (!f || n_hyp < 1 || n_hyp > po::MAX_HYP || n_fine < 1 || n_fine > MAX_FINE) return false;
    for (int k = 0; k < n_hyp * n_fine; k++)
        if (!po::hyp_valid(f[k])) return false;
    return true;
}

/* level-2 thumbnail pixel (u, v) of a frame of PYR_W0 x PYR_H0 bytes: the cascade over its 4 x 4 block */
inline uint8_t thumb_pixel(const uint8_t* img, int u, int v) {
    HNET_ALIGN_NO_CONTRACT
    const uint8_t* p = img + (size_t)(FSTEP * v) * pa::PYR_W0 + FSTEP * u;
    uint32_t l1[4];
    for (int b = 0; b < 2; b++)
        for (int a = 0; a < 2; a++) {
            const uint8_t* q = p + (2 * b) * pa::PYR_W0 + 2 * a;
            l1[2 * b + a] = pa::down4(q[0], q[1], q[pa::PYR_W0], q[pa::PYR_W0 + 1]);
        }
    return pa::down4(l1[0], l1[1], l1[2], l1[3]);
}
inline void thumbnail(const uint8_t* img, uint8_t* out) {
    for (int v = 0; v < FH; v++)
        for (int u = 0; u < FW; u++) out[v * FW + u] = thumb_pixel(img, u, v);
}

/* warped template pixel (u, v) of level-2 thumbnail t under b: the value (0 when invalid); returns the mask, 1 or 0 */
inline int warp_pixel(const uint8_t* t, const int32_t* b, int u, int v, uint8_t& value) {
    const int32_t qx = 2 * u - (FW - 1), qy = 2 * v - (FH - 1);
    const int32_t sx = b[0] * qx + b[1] * qy + ((FW - 1) * po::ONE), sy = b[2] * qx + b[3] * qy + ((FH - 1) * po::ONE);
    const int32_t bias = 1 << 26;                  /* floor for either sign: |sx|, |sy| < 2^25 */
    const int32_t ix = ((sx + bias) >> 17) - (bias >> 17), iy = ((sy + bias) >> 17) - (bias >> 17);
    const int32_t fx = ((sx + bias) >> 9) & 255, fy = ((sy + bias) >> 9) & 255;
    value = 0;
    if (ix < 0 || ix > FW - 1 || iy < 0 || iy > FH - 1 || (fx != 0 && ix + 1 > FW - 1) || (fy != 0 && iy + 1 > FH - 1)) return 0;
    const int32_t ix1 = ix + 1 > FW - 1 ? FW - 1 : ix + 1, iy1 = iy + 1 > FH - 1 ? FH - 1 : iy + 1;
    const int32_t p00 = t[iy * FW + ix], p10 = t[iy * FW + ix1], p01 = t[iy1 * FW + ix], p11 = t[iy1 * FW + ix1];
    value = (uint8_t)(((256 - fx) * (256 - fy) * p00 + fx * (256 - fy) * p10 + (256 - fx) * fy * p01 + fx * fy * p11 + 32768) >> 16);
    return 1;
}
inline void warp_template(const uint8_t* t, const int32_t* b, uint8_t* w, uint8_t* m) {
    for (int v = 0; v < FH; v++)
        for (int u = 0; u < FW; u++) m[v * FW + u] = (uint8_t)warp_pixel(t, b, u, v, w[v * FW + u]);
}

/* whether a level-2 shift is one the rule can form */
inline bool shift_ok(int sx, int sy) { return sx >= -MAX_SX && sx <= MAX_SX && sy >= -MAX_SY && sy <= MAX_SY; }
inline void overlap(int sx, int sy, int& u0, int& u1, int& v0, int& v1) {
    u0 = sx < 0 ? -sx : 0; u1 = sx > 0 ? FW - sx : FW;
    v0 = sy < 0 ? -sy : 0; v1 = sy > 0 ? FH - sy : FH;
}
/* the masked sums of one level-2 shift: a the warped template (0 where m is 0), m its mask, b the image */
inline void shift_sums(const uint8_t* a, const uint8_t* m, const uint8_t* b, int sx, int sy, ps::Sums& s) {
    HNET_ALIGN_NO_CONTRACT
    int u0, u1, v0, v1;
    overlap(sx, sy, u0, u1, v0, v1);
    int32_t n = 0, sa = 0, sb = 0, sab = 0, saa = 0, sbb = 0;
    for (int v = v0; v < v1; v++)
        for (int u = u0; u < u1; u++) {
            const int32_t p = a[v * FW + u], k = m[v * FW + u], q = k * b[(v + sy) * FW + (u + sx)];
            n += k; sa += p; sb += q; sab += p * q; saa += p * p; sbb += q * q;
        }
    s.n = n; s.sa = sa; s.sb = sb; s.sab = sab; s.saa = saa; s.sbb = sbb;
}

/* a candidate index and its parts */
inline int cand_index(int j, int ex, int ey) { return j * NSHIFT + (ey + MAX_R) * NE + (ex + MAX_R); }
inline void index_cand(int i, int& j, int& ex, int& ey) { j = i / NSHIFT; const int k = i % NSHIFT; ey = k / NE - MAX_R; ex = k % NE - MAX_R; }

/* the total order: whether scored candidate i (score si) is better than scored candidate k */
inline bool better(double si, int i, double sk, int k) {
    HNET_ALIGN_NO_CONTRACT
    if (si != sk) return si > sk;
    int ji, xi, yi, jk, xk, yk;
    index_cand(i, ji, xi, yi);
    index_cand(k, jk, xk, yk);
    const int ri = xi * xi + yi * yi, rk = xk * xk + yk * yk;
    if (ri != rk) return ri < rk;
    if (yi != yk) return yi < yk;
    if (xi != xk) return xi < xk;
    return ji < jk;
}
/* a candidate of a reduction: index -1 = none.  offer keeps the better of two; it is associative and commutative. */
struct Best { double score; int32_t index; };
inline void best_none(Best& b) { b.score = -1.0; b.index = -1; }
inline void offer(Best& b, double score, int index) {
    if (index < 0 || score != score) return;
    if (b.index < 0 || better(score, index, b.score, b.index)) { b.score = score; b.index = index; }
}

/* the final start of fine entry a and level-2 shift (sx, sy), the corners in the tree's order */
inline void start_of(const double* a, int sx, int sy, float* start_px) {
    HNET_ALIGN_NO_CONTRACT
    const double xs[4] = {0.0, 0.0, 2.0 * po::CX, 2.0 * po::CX}, ys[4] = {0.0, 2.0 * po::CY, 2.0 * po::CY, 0.0};
    for (int c = 0; c < 4; c++) {
        const double ex = xs[c] - po::CX, ey = ys[c] - po::CY;
        const double px = a[0] * ex + a[1] * ey, py = a[2] * ex + a[3] * ey;
        start_px[2 * c] = (float)(((po::CX + px) + (double)(FSTEP * sx)) - xs[c]);
        start_px[2 * c + 1] = (float)(((po::CY + py) + (double)(FSTEP * sy)) - ys[c]);
    }
}

/* whether the fine stage runs on a coarse record under a table of n_hyp rows */
inline bool coarse_usable(const po::Record& c, int n_hyp) {
    return c.base.flags == ps::FOUND && c.hyp >= 0 && c.hyp < n_hyp && c.base.dx >= -ps::MAX_RX && c.base.dx <= ps::MAX_RX && c.base.dy >= -ps::MAX_RY &&
           c.base.dy <= ps::MAX_RY;
}

/* the fine part from the coarse record, the winner's row of the fine table (null when the stage did not run), the best over the row and its sums: every
 * byte is written */
inline void finish(const po::Record& c, const po::Hyp* row, int n_fine, bool ran, const Best& best, const ps::Sums& s, const Opts& o, Part& r) {
    HNET_ALIGN_NO_CONTRACT
    r.j = -1;
    r.ex = r.ey = r.sx = r.sy = 0;
    r.n_overlap = 0;
    r.pad0 = 0;
    r.score = -1.0;
    for (int k = 0; k < 4; k++) r.a[k] = 0.0;
    r.sa = r.sb = r.sab = r.saa = r.sbb = 0;
    r.pad1 = 0;
    int j = -1, ex = 0, ey = 0;
    if (ran && best.index >= 0) index_cand(best.index, j, ex, ey);
    if (!ran || !row) {
        r.flags = FINE_SKIPPED;
    } else if (j < 0 || j >= n_fine) {
        r.flags = FINE_NOTHING_SCORED;
    } else {
        r.j = j; r.ex = ex; r.ey = ey;
        r.sx = 2 * c.base.dx + ex; r.sy = 2 * c.base.dy + ey;
        r.score = best.score;
        r.n_overlap = s.n; r.sa = s.sa; r.sb = s.sb; r.sab = s.sab; r.saa = s.saa; r.sbb = s.sbb;
        for (int k = 0; k < 4; k++) r.a[k] = row[j].a[k];
        r.flags = r.score < o.min_score ? FINE_LOW_SCORE : FINE_REFINED;
    }
    if (r.flags == FINE_REFINED) start_of(r.a, r.sx, r.sy, r.start_px);
    else
        for (int k = 0; k < pa::NX; k++) r.start_px[k] = r.flags == FINE_SKIPPED ? ps::quiet_nan_f() : c.base.start_px[k];
}

/* one fine entry on the host: level-2 thumbnails t (template) and b (image), coarse shift (dx, dy); its best and the sums of it, scores [81] written */
inline void search_entry(const uint8_t* t, const uint8_t* b, const po::Hyp& h, int j, int dx, int dy, int min_overlap, int radius, Entry& e, double* scores) {
    uint8_t w[FPIX], m[FPIX];
    warp_template(t, h.b, w, m);
    Best best;
    best_none(best);
    for (int i = 0; i < NSHIFT; i++) {
        const int ey = i / NE - MAX_R, ex = i % NE - MAX_R;
        ps::Sums s;
        double sc;
        const bool in = ex >= -radius && ex <= radius && ey >= -radius && ey <= radius;
        if (in) shift_sums(w, m, b, 2 * dx + ex, 2 * dy + ey, s);
        scores[i] = in && ps::shift_score(s, 4 * min_overlap, sc) ? sc : ps::quiet_nan_d();
        offer(best, scores[i], cand_index(j, ex, ey));
    }
    e.score = best.score; e.index = best.index; e.pad = 0;
    e.s = ps::Sums{0, 0, 0, 0, 0, 0};
    if (best.index >= 0) {
        int jj, ex, ey;
        index_cand(best.index, jj, ex, ey);
        shift_sums(w, m, b, 2 * dx + ex, 2 * dy + ey, e.s);
    }
}

/* the fine stage of one pair on the host, after the coarse record c: level-2 thumbnails t and b, the coarse options' min_overlap, the whole fine table
 * [n_hyp][n_fine]; scores [n_fine][81] (may be null) */
inline void refine(const uint8_t* t, const uint8_t* b, const po::Record& c, int min_overlap, int n_hyp, const Opts& o, const po::Hyp* fine, Part& r, double* scores) {
    double sc[NSHIFT];
    if (scores)
        for (int i = 0; i < o.n_fine * NSHIFT; i++) scores[i] = ps::quiet_nan_d();
    Best best;
    best_none(best);
    ps::Sums s = {0, 0, 0, 0, 0, 0};
    const bool ran = coarse_usable(c, n_hyp);
    const po::Hyp* row = ran ? fine + (size_t)c.hyp * o.n_fine : nullptr;
    if (ran)
        for (int j = 0; j < o.n_fine; j++) {
            Entry e;
            search_entry(t, b, row[j], j, c.base.dx, c.base.dy, min_overlap, o.radius, e, scores ? scores + (size_t)j * NSHIFT : sc);
            const Best before = best;
            offer(best, e.score, e.index);
            if (best.index != before.index) s = e.s;
        }
    finish(c, row, o.n_fine, ran, best, s, o, r);
}

}  /* namespace hnet_search_fine */

#endif /* HNET_PHOTO_SEARCH_FINE_H */
