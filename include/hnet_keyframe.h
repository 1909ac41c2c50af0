/* hnet_keyframe.h — tracking a camera against a HELD keyframe (include/hnet.h hnet_sessions_keyframe_track): the rule that turns the level-0
 * record of one alignment "keyframe -> current frame" into the session's next state, what the device (csrc/kernels_keyframe.hip) and the host reference
 * (tests/cpp/keyframe_ref.cpp) both compile, next to include/hnet_photo_robust.h (the alignment's record).  csrc/geom.h (p4, dlt_solve) is included
 * before this header by both.
 *
 * Conventions.  Offsets x are ul, bl, br, ur in pixels; H(x) = dlt_solve(p4 + (double) x) in double, h[8] = 1, NOT rounded to fp32 (the alignment rounds
 * its own H; here an fp32 H would not give x back from the corners of H(x)).  H(x) maps a template pixel to its sampling position in the other image, as
 * in the records of DESIGN 7g, hence H_key->curr = H_prev->curr . H_key->prev.
 *
 * compose(step, key, out): the corners of H(step) . H(key) applied to p4, minus p4, rounded to fp32.  False, nothing written, when an entry of either
 * homography or a projected corner is not finite or a corner's z is not positive.
 *
 * decide(state, start, record, opts, gap) -> new state, output record, copy flag.  The state of a session is {has_key, key_px, h_origin_key, age,
 * keyframes}: the offsets keyframe -> previous tracked frame, the homography origin -> keyframe (the origin is the first keyframe since the last reset),
 * the frames tracked since the keyframe was taken and the keyframes taken.
 *   no keyframe: FIRST | REKEYED.  curr becomes the keyframe (copy = 1), key_px = 0, h_origin_key = I, keyframes = 1, age = 0; nothing of start or record
 *     is read, and the output is zeros but for h_origin_curr = I, keyframes and flags.
 *   LOST, one reason bit, tested in this order: NO_START (an entry of start is not finite: compose failed and the alignment ran from quiet NaNs);
 *     STOPPED (the record's flags hold SINGULAR, DEGENERATE or FEW_PIXELS); MSE_ABOVE_MAX (max_mse > 0 and not mse <= max_mse); NON_FINITE (an entry of
 *     the record's offsets is not finite).  A start that accepted no trial is NOT lost (a camera that stands still has mse0 = 0 and accepts nothing).
 *     The BRIDGE of a lost frame is start when start is finite and H(start) is, else the previous key_px.  With auto_rekey the session re-keys
 *     (REKEYED | BRIDGED, copy = 1) and the origin chain is extended by H(bridge): dead reckoning.  Without it the keyframe stays and key_px = bridge;
 *     BRIDGED is then set only when the bridge is the start (otherwise nothing changed but the age).
 *   TRACKED (everything else): key_px = the record's offsets.
 *   In both: age + 1, overlap = n_valid / 71 680 of the record, h_origin_curr = H(key_px) . h_origin_key renormalised to h[8] = 1.  With auto_rekey a
 *   TRACKED session re-keys after this frame when overlap < rekey_overlap (LOW_OVERLAP) or max_age > 0 and the new age >= max_age (MAX_AGE); both bits
 *   may be set.  A re-key: h_origin_key <- h_origin_curr, key_px = 0, age = 0, keyframes + 1, copy = 1.
 *   The origin chain going degenerate: when a product has a non-finite entry or |h[8]| below 1e-12 of its largest entry, the chain restarts at the
 *   current keyframe: h_origin_key = I (ORIGIN_RESTARTED) and h_origin_curr = H(key_px), or I when that is not finite either.
 *   gap (the session's image count is not its count at the previous track + 1: frames no track saw, or the same frame tracked again) only sets GAP:
 *   the alignment's basin decides whether the start served.
 * Choices the rule left open.  The output's key_px is the measurement keyframe -> curr (the bridge for a lost frame) and its age the frame's age against
 * the keyframe it was measured on, also when the state re-keys after it; keyframes counts the new keyframe.  A lost frame ages the keyframe like a
 * tracked one, and max_age is not judged on it (it re-keys anyway with auto_rekey, and never without).  decide does not touch out.rec: the caller copies
 * the record there, or zeros for FIRST.
 * Every body is non-contracting, everything is in double, nothing depends on the batch.
 */
#ifndef HNET_KEYFRAME_H
#define HNET_KEYFRAME_H

#include <cstring>

#include "hnet_photo_robust.h"

namespace hnet_keyframe {

namespace pa = hnet_align;
namespace pr = hnet_robust;

constexpr double FRAME_PIXELS = 71680.0;       /* 224 x 320 */
constexpr double ORIGIN_TINY = 1e-12;

/* the flags of a track record (= HNET_KF_*) */
enum { FIRST = 1,                  /* the session had no keyframe: curr became it, no alignment result was read */
       REKEYED = 2,                /* curr is the session's keyframe from the next call on */
       BRIDGED = 4,                /* LOST, and the composed start stands in for the measurement */
       GAP = 8,                    /* frames were pushed since the previous track that no track saw */
       LOW_OVERLAP = 16,           /* re-key reason: overlap < rekey_overlap */
       MAX_AGE = 32,               /* re-key reason: max_age > 0 and age >= max_age */
       NO_START = 64,              /* LOST: compose failed, the start has no homography */
       STOPPED = 128,              /* LOST: the record stopped SINGULAR, DEGENERATE or FEW_PIXELS */
       MSE_ABOVE_MAX = 256,        /* LOST: max_mse > 0 and not mse <= max_mse */
       NON_FINITE = 512,           /* LOST: an entry of the record's offsets is not finite */
       ORIGIN_RESTARTED = 1024,    /* the origin chain went degenerate and restarts at the current keyframe */
       LOST = NO_START | STOPPED | MSE_ABOVE_MAX | NON_FINITE };

/* = hnet_keyframe_opts */
struct Opts { pr::Opts align; int32_t levels, auto_rekey, max_age, pad; double rekey_overlap, max_mse; };
inline void default_opts(Opts& o) {
    pr::default_opts(o.align);
    o.levels = 3; o.auto_rekey = 1; o.max_age = 0; o.pad = 0; o.rekey_overlap = 0.6; o.max_mse = 0.0;
}
inline bool opts_valid(const Opts& o) {
    return pr::opts_valid(o.align) && o.levels >= 1 && o.levels <= pa::MAX_LEVELS && (o.auto_rekey == 0 || o.auto_rekey == 1) && o.max_age >= 0 &&
           o.rekey_overlap >= 0.0 && o.rekey_overlap <= 1.0 && o.max_mse >= 0.0 && std::isfinite(o.max_mse);
}

/* a session's state: one entry of the device table */
struct State { int32_t has_key, age, keyframes, pad; float key_px[pa::NX]; double h_origin_key[9]; };

/* = hnet_keyframe_track */
struct Track {
    pr::Record rec;
    float start_px[pa::NX], key_px[pa::NX];
    double h_origin_curr[9], overlap;
    int32_t age, keyframes, flags, pad;
};

/* the start the alignment gets when there is none to compose: on it every level reports DEGENERATE */
inline float quiet_nan() {
    const uint32_t u = 0x7fc00000u;
    float f;
    std::memcpy(&f, &u, sizeof f);
    return f;
}

/* H(x); false when an offset or an entry of H is not finite */
inline bool homography(const float* x, double h[9]) {
    HNET_ALIGN_NO_CONTRACT
    double dst[8];
    bool ok = true;
    for (int k = 0; k < 8; k++) {
        dst[k] = hnet::p4(k) + (double)x[k];
        ok = ok && std::isfinite(dst[k]);
    }
    hnet::dlt_solve(dst, h);
    for (int k = 0; k < 9; k++) ok = ok && std::isfinite(h[k]);
    return ok;
}

/* c = a b (a, b and c distinct) */
inline void mul3(const double a[9], const double b[9], double c[9]) {
    HNET_ALIGN_NO_CONTRACT
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}

inline bool compose(const float* step_px, const float* key_px, float* out_px) {
    HNET_ALIGN_NO_CONTRACT
    double hs[9], hk[9], m[9];
    float o[8];
    if (!homography(step_px, hs) || !homography(key_px, hk)) return false;
    mul3(hs, hk, m);
    bool ok = true;
    for (int c = 0; c < 4; c++) {
        const double u = hnet::p4(2 * c), v = hnet::p4(2 * c + 1);
        const double X = (m[0] * u + m[1] * v) + m[2], Y = (m[3] * u + m[4] * v) + m[5], Z = (m[6] * u + m[7] * v) + m[8];
        const double px = X / Z, py = Y / Z;
        ok = ok && Z > 0.0 && std::isfinite(px) && std::isfinite(py);
        o[2 * c] = (float)(px - u);
        o[2 * c + 1] = (float)(py - v);
    }
    if (!ok) return false;
    for (int k = 0; k < 8; k++) out_px[k] = o[k];
    return true;
}

/* out = hx . h_origin renormalised to out[8] = 1; false (out untouched) when the product is degenerate */
inline bool chain(const double hx[9], const double h_origin[9], double out[9]) {
    HNET_ALIGN_NO_CONTRACT
    double m[9];
    mul3(hx, h_origin, m);
    double top = 0.0;
    bool ok = true;
    for (int k = 0; k < 9; k++) {
        const double a = std::fabs(m[k]);
        top = a > top ? a : top;
        ok = ok && std::isfinite(m[k]);
    }
    if (!ok || std::fabs(m[8]) < ORIGIN_TINY * top) return false;
    for (int k = 0; k < 9; k++) out[k] = m[k] / m[8];
    return true;
}

/* s and ns may be the same object, as may start_px and out.start_px; returns the copy flag.  out.rec is the caller's (see above). */
inline int decide(const State& s, const float* start_px, const pr::Record& rec, const Opts& o, bool gap, State& ns, Track& out) {
    HNET_ALIGN_NO_CONTRACT
    double ho[9], hc[9], hx[9];
    float start[8], key[8];
    for (int k = 0; k < 9; k++) ho[k] = hc[k] = (k & 3) == 0 ? 1.0 : 0.0;
    if (!s.has_key) {
        for (int k = 0; k < 8; k++) { ns.key_px[k] = 0.0f; out.start_px[k] = 0.0f; out.key_px[k] = 0.0f; }
        for (int k = 0; k < 9; k++) { ns.h_origin_key[k] = ho[k]; out.h_origin_curr[k] = ho[k]; }
        ns.has_key = 1; ns.age = 0; ns.keyframes = 1; ns.pad = 0;
        out.overlap = 0.0;
        out.age = 0; out.keyframes = 1; out.flags = FIRST | REKEYED; out.pad = 0;
        return 1;
    }
    int flags = gap ? (int)GAP : 0;
    const int age = s.age + 1;
    int keyframes = s.keyframes;
    bool start_finite = true, rec_finite = true;
    for (int k = 0; k < 8; k++) {
        start[k] = start_px[k];
        key[k] = s.key_px[k];
        start_finite = start_finite && std::isfinite(start[k]);
        rec_finite = rec_finite && std::isfinite(rec.px.offsets_px[k]);
    }
    for (int k = 0; k < 9; k++) ho[k] = s.h_origin_key[k];
    int why = 0;
    if (!start_finite) why = NO_START;
    else if (rec.px.flags & (pa::SINGULAR | pa::DEGENERATE | pa::FEW_PIXELS)) why = STOPPED;
    else if (o.max_mse > 0.0 && !(rec.px.mse <= o.max_mse)) why = MSE_ABOVE_MAX;
    else if (!rec_finite) why = NON_FINITE;
    flags |= why;
    const double overlap = (double)rec.px.n_valid / FRAME_PIXELS;
    bool have_h;
    if (why) {
        const bool by_start = start_finite && homography(start, hx);
        have_h = by_start;
        if (by_start) {
            for (int k = 0; k < 8; k++) key[k] = start[k];
        } else {
            have_h = homography(key, hx);
        }
        if (by_start || (o.auto_rekey && have_h)) flags |= BRIDGED;
    } else {
        for (int k = 0; k < 8; k++) key[k] = rec.px.offsets_px[k];
        have_h = homography(key, hx);
    }
    /* h_origin_curr; a degenerate chain restarts at the keyframe */
    if (!have_h || !chain(hx, ho, hc)) {
        flags |= ORIGIN_RESTARTED;
        for (int k = 0; k < 9; k++) ho[k] = (k & 3) == 0 ? 1.0 : 0.0;
        if (!have_h || !chain(hx, ho, hc))
            for (int k = 0; k < 9; k++) hc[k] = ho[k];
    }
    bool rekey = false;
    if (o.auto_rekey) {
        if (why) {
            rekey = true;
        } else {
            if (overlap < o.rekey_overlap) { flags |= LOW_OVERLAP; rekey = true; }
            if (o.max_age > 0 && age >= o.max_age) { flags |= MAX_AGE; rekey = true; }
        }
    }
    if (rekey) {
        flags |= REKEYED;
        keyframes++;
    }
    for (int k = 0; k < 8; k++) {
        out.start_px[k] = start[k];
        out.key_px[k] = key[k];
        ns.key_px[k] = rekey ? 0.0f : key[k];
    }
    for (int k = 0; k < 9; k++) {
        out.h_origin_curr[k] = hc[k];
        ns.h_origin_key[k] = rekey ? hc[k] : ho[k];
    }
    ns.has_key = 1; ns.age = rekey ? 0 : age; ns.keyframes = keyframes; ns.pad = 0;
    out.overlap = overlap;
    out.age = age; out.keyframes = keyframes; out.flags = flags; out.pad = 0;
    return rekey ? 1 : 0;
}

}  /* namespace hnet_keyframe */

#endif /* HNET_KEYFRAME_H */
