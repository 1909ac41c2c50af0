/* hnet_photo_search_oriented.h — the coarse search of include/hnet_photo_search.h under a table of ORIENTATION hypotheses (include/hnet.h
 * hnet_op_photo_search_oriented, hnet_sessions_photo_search_oriented, hnet_sessions_keyframe_relocalise_oriented): a camera that is lost AND has
 * turned.  What the device (csrc/kernels_photo_search_oriented.hip) and the host reference (tests/cpp/photo_search_oriented_ref.cpp) both compile.
 *
 * A hypothesis is a linear map A about the frame centre c = (159.5, 111.5): x' = c + A (x - c) + t, in the sense of H(x) everywhere in the tree.  A table
 * entry holds A as doubles (a[4], row major) and b[4] = round(65536 A^-1) as int32; make_hyp fills one with std::cos / std::sin on the HOST, the device only
 * ever receives the table.  1 .. 64 entries, the scale in [0.5, 2]; an entry with a non-finite a or |b[i]| > 2 * 65536 is refused (hyp_valid).
 * The warped template of an entry, integers only, so that host and device agree bit for bit: for thumbnail pixel (u, v), with q = (2u - 39, 2v - 27) (twice
 * the offset from the thumbnail's centre (19.5, 13.5)), sx = b00 qx + b01 qy + (39 << 16), sy = b10 qx + b11 qy + (27 << 16) (|.| < 2^25), the source
 * position in 1/2^17 pixels: ix = floor(sx / 2^17), fx = floor(sx / 2^9) mod 256 and the same in y.  The pixel is VALID when 0 <= ix <= 39, 0 <= iy <= 27,
 * (fx == 0 or ix + 1 <= 39) and (fy == 0 or iy + 1 <= 27); its value is then
 *   ((256 - fx)(256 - fy) p00 + fx (256 - fy) p10 + (256 - fx) fy p01 + fx fy p11 + 32768) >> 16, taps of weight zero read at a clamped index,
 * and an invalid pixel is 0 with mask 0.  The identity reproduces the thumbnail under a full mask; quarter turns are exact permutations of pixels.
 * Per entry the search is 7r's with the sums restricted to the valid template pixels of the overlap: n = sum m, Sa = sum a, Saa = sum a^2, Sab = sum a b,
 * Sb = sum m b, Sbb = sum m b^2, then hnet_search::shift_score, better, offer and outside3 exactly as they are: the entry's best and its second.
 * The winner over the table is the entry with a scored shift whose best has the highest score, ties to the lower table index: a total order.  The flags are
 * 7r's four, judged by hnet_search::finish on the winner's best and the winner's OWN second; nothing scored under any entry: NO_TEXTURE.  The runner-up is
 * the winner of the table without the winning entry: reported, never gated (neighbouring entries are near-peaks by construction).
 * start_px at corner x_i of the order (0, 0), (0, 223), (319, 223), (319, 0) is c + A (x_i - c) + 8 (dx, dy) - x_i, formed in double in the order of
 * start_of and rounded to float once; quiet NaNs unless FOUND.  A table of only the identity gives hnet_search::search's record in the first 96 bytes.
 * Choices the rule left open.  Without a winner hyp = -1, n_scored = 0 and a is zero; without a runner-up hyp2 = -1 and score2 = -1.  The scores of a call are
 * [n_hyp][41][61] doubles per pair, each table as 7r's.  Every body is non-contracting.
 */
#ifndef HNET_PHOTO_SEARCH_ORIENTED_H
#define HNET_PHOTO_SEARCH_ORIENTED_H

#include "hnet_photo_search.h"

namespace hnet_search_oriented {

namespace ps = hnet_search;

constexpr int MAX_HYP = 64;
constexpr int ONE = 65536, MAX_B = 2 * ONE;                    /* b is 16.16 fixed point; a scale of 0.5 is |b| = 2 */
constexpr double MIN_SCALE = 0.5, MAX_SCALE = 2.0;
constexpr double CX = 159.5, CY = 111.5;                       /* the frame centre = the centre of the thumbnail's pixel grid, times 8, plus 3.5 */
constexpr int DEFAULT_COUNT = 60;                              /* the documented default table: 60 entries of 6 degrees from -180 */
constexpr double DEFAULT_FIRST_DEG = -180.0, DEFAULT_STEP_DEG = 6.0;
static_assert(ps::TW == 40 && ps::TH == 28, "q = (2u - 39, 2v - 27)");

/* = hnet_photo_search_hyp */
struct Hyp { double a[4]; int32_t b[4]; };

/* = hnet_photo_search_oriented */
struct Record {
    ps::Record base;           /* of the winning entry: 7r's record, start_px under the entry */
    int32_t hyp;               /* the winner's table index, -1 without one */
    int32_t n_scored;          /* entries with a scored shift */
    int32_t hyp2, pad0;        /* the runner-up's table index, -1 without one */
    double score2;             /* its best score, -1 without one */
    double a[4];               /* the winner's matrix, zeros without one */
    int32_t pad[2];
};
static_assert(sizeof(Hyp) == 48 && sizeof(Record) == 160 && offsetof(Record, hyp) == 96 && offsetof(Record, n_scored) == 100 && offsetof(Record, hyp2) == 104 &&
              offsetof(Record, score2) == 112 && offsetof(Record, a) == 120 && offsetof(Record, pad) == 152, "the layout of hnet_photo_search_oriented");

/* the entry of a rotation by angle_rad and a scale: false (nothing written) for a non-finite angle or a scale outside [0.5, 2].  Called on the host
 * only: no kernel evaluates a trigonometric function. */
inline bool make_hyp(double angle_rad, double scale, Hyp& h) {
    HNET_ALIGN_NO_CONTRACT
    if (!std::isfinite(angle_rad) || !(scale >= MIN_SCALE && scale <= MAX_SCALE)) return false;
    const double c = std::cos(angle_rad), s = std::sin(angle_rad);
    h.a[0] = scale * c; h.a[1] = -(scale * s); h.a[2] = scale * s; h.a[3] = scale * c;
    const double inv[4] = {c / scale, s / scale, -(s / scale), c / scale};          /* A^-1 = R(-angle) / scale */
    for (int k = 0; k < 4; k++) h.b[k] = (int32_t)std::floor(inv[k] * (double)ONE + 0.5);
    return true;
}
/* count entries of scale 1 at first_deg + k step_deg degrees; false for a count outside 1 .. 64 or non-finite angles */
inline bool yaw_table(double first_deg, double step_deg, int count, Hyp* out) {
    HNET_ALIGN_NO_CONTRACT
    if (count < 1 || count > MAX_HYP || !std::isfinite(first_deg) || !std::isfinite(step_deg)) return false;
    for (int k = 0; k < count; k++) {
        const double deg = first_deg + (double)k * step_deg;
        if (!make_hyp(deg * (3.14159265358979323846 / 180.0), 1.0, out[k])) return false;
    }
    return true;
}

inline bool hyp_valid(const Hyp& h) {
    bool ok = true;
    for (int k = 0; k < 4; k++) ok = ok && std::isfinite(h.a[k]) && h.b[k] >= -MAX_B && h.b[k] <= MAX_B;
    return ok;
}
inline bool table_valid(const Hyp* h, int n_hyp) {
    if (!h || n_hyp < 1 || n_hyp > MAX_HYP) return false;
    for (int k = 0; k < n_hyp; k++)
        if (!hyp_valid(h[k])) return false;
    return true;
}

/* warped template pixel (u, v) of thumbnail t under b: the value (0 when invalid); returns the mask, 1 or 0 */
inline int warp_pixel(const uint8_t* t, const int32_t* b, int u, int v, uint8_t& value) {
    const int32_t qx = 2 * u - (ps::TW - 1), qy = 2 * v - (ps::TH - 1);
    const int32_t sx = b[0] * qx + b[1] * qy + ((ps::TW - 1) * ONE), sy = b[2] * qx + b[3] * qy + ((ps::TH - 1) * ONE);
    /* floor for either sign: the shifts below are of x + 2^26 >= 0 (|b q| sums below 2^25) */
    const int32_t bias = 1 << 26;
    const int32_t ix = ((sx + bias) >> 17) - (bias >> 17), iy = ((sy + bias) >> 17) - (bias >> 17);
    const int32_t fx = ((sx + bias) >> 9) & 255, fy = ((sy + bias) >> 9) & 255;
    value = 0;
    if (ix < 0 || ix > ps::TW - 1 || iy < 0 || iy > ps::TH - 1 || (fx != 0 && ix + 1 > ps::TW - 1) || (fy != 0 && iy + 1 > ps::TH - 1)) return 0;
    const int32_t ix1 = ix + 1 > ps::TW - 1 ? ps::TW - 1 : ix + 1, iy1 = iy + 1 > ps::TH - 1 ? ps::TH - 1 : iy + 1;
    const int32_t p00 = t[iy * ps::TW + ix], p10 = t[iy * ps::TW + ix1], p01 = t[iy1 * ps::TW + ix], p11 = t[iy1 * ps::TW + ix1];
    value = (uint8_t)(((256 - fx) * (256 - fy) * p00 + fx * (256 - fy) * p10 + (256 - fx) * fy * p01 + fx * fy * p11 + 32768) >> 16);
    return 1;
}

/* the warped template and its mask (bytes 1 / 0), [TPIX] each */
inline void warp_template(const uint8_t* t, const int32_t* b, uint8_t* w, uint8_t* m) {
    for (int v = 0; v < ps::TH; v++)
        for (int u = 0; u < ps::TW; u++) m[v * ps::TW + u] = (uint8_t)warp_pixel(t, b, u, v, w[v * ps::TW + u]);
}

/* the masked sums of one shift with |dx| <= MAX_RX, |dy| <= MAX_RY: a the warped template (0 where m is 0), m its mask, b the image */
inline void shift_sums(const uint8_t* a, const uint8_t* m, const uint8_t* b, int dx, int dy, ps::Sums& s) {
    HNET_ALIGN_NO_CONTRACT
    int u0, u1, v0, v1;
    ps::overlap(dx, dy, u0, u1, v0, v1);
    int32_t n = 0, sa = 0, sb = 0, sab = 0, saa = 0, sbb = 0;
    for (int v = v0; v < v1; v++)
        for (int u = u0; u < u1; u++) {
            const int32_t p = a[v * ps::TW + u], k = m[v * ps::TW + u], q = k * b[(v + dy) * ps::TW + (u + dx)];
            n += k; sa += p; sb += q; sab += p * q; saa += p * p; sbb += q * q;
        }
    s.n = n; s.sa = sa; s.sb = sb; s.sab = sab; s.saa = saa; s.sbb = sbb;
}

/* the score table [NSHIFT] of a warped template: quiet NaN where a shift is not scored or lies outside the radii */
inline void score_table(const uint8_t* a, const uint8_t* m, const uint8_t* b, const ps::Opts& o, double* scores) {
    for (int i = 0; i < ps::NSHIFT; i++) {
        int dx, dy;
        ps::index_shift(i, dx, dy);
        ps::Sums s;
        double sc;
        const bool in = dx >= -o.radius_x && dx <= o.radius_x && dy >= -o.radius_y && dy <= o.radius_y;
        if (in) shift_sums(a, m, b, dx, dy, s);
        scores[i] = in && ps::shift_score(s, o.min_overlap, sc) ? sc : ps::quiet_nan_d();
    }
}

/* the search of one entry on the host: thumbnails t (template) and b (image); 7r's record of the entry (start_px as 7r's), scores [NSHIFT] written */
inline void search_hyp(const uint8_t* t, const uint8_t* b, const Hyp& h, const ps::Opts& o, ps::Record& r, double* scores) {
    uint8_t w[ps::TPIX], m[ps::TPIX];
    warp_template(t, h.b, w, m);
    score_table(w, m, b, o, scores);
    ps::Best best, second;
    ps::Sums s = {0, 0, 0, 0, 0, 0};
    ps::best_none(best);
    ps::best_none(second);
    for (int i = 0; i < ps::NSHIFT; i++) ps::offer(best, scores[i], i);
    if (best.index >= 0) {
        int dx, dy;
        ps::index_shift(best.index, dx, dy);
        shift_sums(w, m, b, dx, dy, s);
        for (int i = 0; i < ps::NSHIFT; i++)
            if (ps::outside3(i, best.index)) ps::offer(second, scores[i], i);
    }
    ps::finish(best, second, s, o, r);
}

/* the order over the table: whether entry i (a scored best of score si) is better than entry j */
inline bool hyp_better(double si, int i, double sj, int j) {
    if (si != sj) return si > sj;
    return i < j;
}
/* a candidate of the reduction over the table: index -1 = none.  offer_hyp keeps the better of two; it is associative and commutative. */
struct BestHyp { double score; int32_t index; };
inline void hyp_none(BestHyp& b) { b.score = -1.0; b.index = -1; }
inline void offer_hyp(BestHyp& b, double score, int index) {
    if (index < 0) return;
    if (b.index < 0 || hyp_better(score, index, b.score, b.index)) { b.score = score; b.index = index; }
}
/* whether an entry's record holds a scored best */
inline bool hyp_scored(const ps::Record& r) { return r.flags != ps::NO_TEXTURE && r.flags != 0; }

/* start_px [8] of entry a and shift (dx, dy), the corners in the tree's order */
inline void start_of(const double* a, int dx, int dy, float* start_px) {
    HNET_ALIGN_NO_CONTRACT
    const double xs[4] = {0.0, 0.0, 2.0 * CX, 2.0 * CX}, ys[4] = {0.0, 2.0 * CY, 2.0 * CY, 0.0};
    for (int c = 0; c < 4; c++) {
        const double ex = xs[c] - CX, ey = ys[c] - CY;
        const double px = a[0] * ex + a[1] * ey, py = a[2] * ex + a[3] * ey;
        start_px[2 * c] = (float)(((CX + px) + (double)(ps::STEP * dx)) - xs[c]);
        start_px[2 * c + 1] = (float)(((CY + py) + (double)(ps::STEP * dy)) - ys[c]);
    }
}

/* the record of a call from the entries' records [n_hyp] (winner and runner-up already reduced, or -1): every byte is written */
inline void finish(const ps::Record* per_hyp, const Hyp* hyps, int n_hyp, const BestHyp& win, const BestHyp& second, int n_scored, Record& r) {
    HNET_ALIGN_NO_CONTRACT
    if (win.index >= 0 && win.index < n_hyp) {
        r.base = per_hyp[win.index];
        if (r.base.flags == ps::FOUND) start_of(hyps[win.index].a, r.base.dx, r.base.dy, r.base.start_px);
        for (int k = 0; k < 4; k++) r.a[k] = hyps[win.index].a[k];
        r.hyp = win.index;
    } else {
        r.base = per_hyp[0];                       /* nothing is scored anywhere: every entry's record is the same NO_TEXTURE record */
        for (int k = 0; k < 4; k++) r.a[k] = 0.0;
        r.hyp = -1;
    }
    r.n_scored = n_scored;
    r.hyp2 = second.index >= 0 ? second.index : -1;
    r.pad0 = 0;
    r.score2 = second.index >= 0 ? second.score : -1.0;
    r.pad[0] = r.pad[1] = 0;
}

/* the winner and the runner-up over the entries' records, in any order of the offers */
inline void reduce(const ps::Record* per_hyp, int n_hyp, BestHyp& win, BestHyp& second, int& n_scored) {
    hyp_none(win);
    hyp_none(second);
    n_scored = 0;
    for (int h = 0; h < n_hyp; h++)
        if (hyp_scored(per_hyp[h])) { offer_hyp(win, per_hyp[h].score, h); n_scored++; }
    for (int h = 0; h < n_hyp; h++)
        if (h != win.index && hyp_scored(per_hyp[h])) offer_hyp(second, per_hyp[h].score, h);
}

/* the whole oriented search of two thumbnails on the host; scores [n_hyp][NSHIFT] (may be null); per_hyp [n_hyp] (may be null) receives the entries' records */
inline void search(const uint8_t* t, const uint8_t* b, const ps::Opts& o, const Hyp* hyps, int n_hyp, Record& r, double* scores, ps::Record* per_hyp) {
    ps::Record tmp[MAX_HYP];
    double sc[ps::NSHIFT];
    ps::Record* ph = per_hyp ? per_hyp : tmp;
    for (int h = 0; h < n_hyp; h++) search_hyp(t, b, hyps[h], o, ph[h], scores ? scores + (size_t)h * ps::NSHIFT : sc);
    BestHyp win, second;
    int n_scored;
    reduce(ph, n_hyp, win, second, n_scored);
    finish(ph, hyps, n_hyp, win, second, n_scored, r);
}

}  /* namespace hnet_search_oriented */

#endif /* HNET_PHOTO_SEARCH_ORIENTED_H */
