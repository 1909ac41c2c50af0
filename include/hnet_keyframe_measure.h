/* hnet_keyframe_measure.h — a session's keyframe track as a filter measurement INSIDE the step (include/hnet.h hnet_filters_set_keyframe_measure; DESIGN
 * 7v), dependency free: what the device (csrc/kernels_filters_keyframe.hip) and the host reference (tests/cpp/filters_keyframe_ref.cpp) both compile, on
 * top of the unedited include/hnet_keyframe.h (compose, decide, homography, chain), include/hnet_keyframe_map.h (relative: the adjugate inverse, corners)
 * and include/hnet_photo_refine.h (refine_measurement and its pieces; hnet_ekf's innovation and update).  csrc/geom.h (p4, dlt_solve) is included before
 * this header by both, as for include/hnet_keyframe.h.
 *
 * Why inside the step.  State::reset_4pt_offset zeroes the offset rows and their covariance after every update, so a measurement of the offsets handed
 * over after the step meets H P H^T = 0.  The keyframe measurement therefore enters after the network's iterations and before the reset, as one more
 * sequential update, linearised at the network's posterior: the last iteration's update runs with update_offset = 1 (rows 0 .. 14 of dx do not depend on
 * it, and the offsets are reset afterwards, so a session without the feature keeps its bytes).
 *
 * The rule, per measuring session:
 *   1 step_px[k] = (float)(159.5 * offset) of the state after the network's iterations.
 *   2 the track: start = compose(step_px, key_px), the robust alignment key -> curr from it, decide with the call's keyframe options and gap: exactly
 *     hnet_sessions_keyframe_track with the filter's own step.
 *   3 UNUSABLE, one reason bit, tested in this order: the state before the call held no keyframe (FIRST); the track's record has a LOST bit (TRACK_LOST);
 *     it has GAP (TRACK_GAP); the session's previous in-step track left no measured key_px (PREV_NOT_MEASURED: prev_ok is 1 after TRACKED or FIRST, 0
 *     after LOST and for a session never measured); H(key_px_prev) has no inverse by relative's test or a corner of the product fails corners
 *     (NO_INVERSE); then refine_measurement's reasons on the level-0 record, in its order.
 *   4 z_px = the corners of H(rec offsets) . inverse(H(key_px_prev)) minus p4, rounded to fp32: the consecutive-frame offsets the network measures and
 *     the offset states predict.  R_px = cov_scale * mse * inverse(info8) + sigma_floor_px^2 I, symmetrised (refine_measurement's).
 *     Two approximations are deliberate: the Jacobian of z with respect to key_px_curr is taken as I, and the noise of key_px_prev is ignored - which
 *     is what lets the errors telescope: the composition of the H(z) over a stay on one keyframe equals the last key_px.
 *   5 the session is SELECTED under when = ALWAYS, or under IF_NONE when the network's iterations applied nothing; never after a singular S of the
 *     network's own.  For a selected usable session: the prior of the current state, innovation (with the NIS gate when max_nis > 0), update with
 *     update_offset = false.  The reset follows for every session.
 * Every body is non-contracting and in double; nothing depends on the batch.
 */
#ifndef HNET_KEYFRAME_MEASURE_H
#define HNET_KEYFRAME_MEASURE_H

#include "hnet_keyframe_map.h"
#include "hnet_photo_refine.h"

namespace hnet_kfm {

namespace pa = hnet_align;
namespace pr = hnet_robust;
namespace kf = hnet_keyframe;
namespace km = hnet_keyframe_map;
namespace rf = hnet_refine;

/* `when` (= HNET_KFM_ALWAYS, HNET_KFM_IF_NONE) */
enum { ALWAYS = 0, IF_NONE = 1 };

/* the flags of a measure record (= HNET_KFM_*); bits 1 .. 512 are hnet_refine's */
enum { ASKED = 1,                      /* the session measures: `track` is its in-step track's record */
       APPLIED = 2,                    /* the keyframe update was applied */
       NIS_REJECTED = 4,               /* the session's NIS gate refused the measurement */
       S_SINGULAR = 8,                 /* update() found the measurement's S singular */
       BAD_K_NET_COV = 16, STOPPED = 32, NO_STEP = 64, MSE_ABOVE_MAX = 128, NO_FACTOR = 256, NON_FINITE = 512,      /* UNUSABLE: refine_measurement's */
       FIRST = 1024,                   /* UNUSABLE: the state before the call held no keyframe */
       TRACK_LOST = 2048,              /* UNUSABLE: the track's record has a LOST bit */
       TRACK_GAP = 4096,               /* UNUSABLE: the track's record has GAP */
       PREV_NOT_MEASURED = 8192,       /* UNUSABLE: the previous in-step track left no measured key_px */
       NO_INVERSE = 16384,             /* UNUSABLE: H(key_px_prev) has no inverse, or a corner of the product fails */
       NOT_SELECTED = 32768,           /* `when` (or a singular S of the network's own) kept the measurement from the filter; not an UNUSABLE reason */
       UNUSABLE = BAD_K_NET_COV | STOPPED | NO_STEP | MSE_ABOVE_MAX | NO_FACTOR | NON_FINITE | FIRST | TRACK_LOST | TRACK_GAP | PREV_NOT_MEASURED | NO_INVERSE };
static_assert((int)ASKED == rf::ASKED && (int)APPLIED == rf::APPLIED && (int)NIS_REJECTED == rf::NIS_REJECTED && (int)S_SINGULAR == rf::S_SINGULAR &&
              (int)BAD_K_NET_COV == rf::BAD_K_NET_COV && (int)STOPPED == rf::STOPPED && (int)NO_STEP == rf::NO_STEP && (int)MSE_ABOVE_MAX == rf::MSE_ABOVE_MAX &&
              (int)NO_FACTOR == rf::NO_FACTOR && (int)NON_FINITE == rf::NON_FINITE, "the low bits are hnet_refine's");

/* = hnet_keyframe_measure_opts: the track's options (shared by the measuring sessions of a call), and per session the measurement's */
struct Opts { kf::Opts track; double cov_scale, sigma_floor_px, max_mse; int32_t when, pad; };
inline void default_opts(Opts& o) {
    kf::default_opts(o.track);
    o.cov_scale = 0.0; o.sigma_floor_px = 0.05; o.max_mse = 0.0; o.when = ALWAYS; o.pad = 0;
}
inline bool opts_valid(const Opts& o) {
    return kf::opts_valid(o.track) && o.cov_scale > 0.0 && std::isfinite(o.cov_scale) && o.sigma_floor_px >= 0.0 && std::isfinite(o.sigma_floor_px) &&
           o.max_mse >= 0.0 && std::isfinite(o.max_mse) && (o.when == ALWAYS || o.when == IF_NONE);
}
/* what refine_measurement reads of them */
inline void refine_opts(const Opts& o, rf::Opts& r) {
    r.align = o.track.align; r.levels = o.track.levels; r.pad = 0;
    r.cov_scale = o.cov_scale; r.sigma_floor_px = o.sigma_floor_px; r.max_mse = o.max_mse;
}

/* = hnet_keyframe_measure: the track's record, the step it was composed from, z_px, R_px, the measurement's innovation (hnet_innovation: r, s_diag, nis,
 * iteration = max_iekf_iteration, flag) */
struct Record {
    kf::Track track;
    float step_px[pa::NX], z_px[pa::NX];
    double r_px[pa::NX * pa::NX];
    double r[8], s_diag[8], nis;
    int32_t iteration, flag;
    int32_t flags, pad;
};

/* a session as the host twin carries it: the keyframe state and the prev_ok word */
struct Session { kf::State key; int32_t prev_ok, pad; };

/* entry k of step_px */
inline float step_entry(const hnet_ekf::State& s, int k) { HNET_ALIGN_NO_CONTRACT return (float)(hnet_ekf::F_PIX * s.offset[k >> 1][k & 1]); }

/* what can be judged before any matrix is formed: 0, or the reason bit.  had_key: the state BEFORE the track; track_flags: the track's record */
inline int usable(bool had_key, int track_flags, int prev_ok) {
    if (!had_key) return FIRST;
    if (track_flags & kf::LOST) return TRACK_LOST;
    if (track_flags & kf::GAP) return TRACK_GAP;
    if (!prev_ok) return PREV_NOT_MEASURED;
    return 0;
}
/* prev_ok after a track */
inline int next_prev_ok(int track_flags) { return (track_flags & kf::LOST) ? 0 : 1; }
/* whether `when` lets the measurement reach the filter.  updates: the slot's update counter after the network's iterations (< 0: a singular S) */
inline bool selected(int when, int updates) { return updates >= 0 && (when == ALWAYS || updates == 0); }

/* z_px = corners(H(key_px_curr) . inverse(H(key_px_prev))) - p4, rounded to fp32; false: nothing usable was written */
inline bool relative_z(const float* key_px_prev, const float* key_px_curr, float z_px[8]) {
    HNET_ALIGN_NO_CONTRACT
    km::Entry e;
    double hc[9], G[9];
    e.valid = 1; e.links = 0; e.serial = 0; e.pad = 0;
    if (!kf::homography(key_px_prev, e.h_origin_key) || !kf::homography(key_px_curr, hc)) return false;
    return km::relative(hc, e, G, z_px);
}

/* Steps 3 and 4 on a track's record.  had_key and key_px_prev: the keyframe state before the track; track: decide's record with `rec` copied in;
 * accepted_total: the trials accepted over all levels.  -> true: z_px, r_px and out72 = {z_px | (float)(R_px / k_net_cov)} written, flags untouched;
 * false: UNUSABLE, the reason bit set in flags and nothing else written */
inline bool measure(bool had_key, const float* key_px_prev, int prev_ok, const kf::Track& track, int accepted_total, const Opts& o, double k_net_cov,
                    float* z_px, double* r_px, float* out72, int32_t& flags) {
    if (const int why = usable(had_key, track.flags, prev_ok)) { flags |= why; return false; }
    float z[8];
    if (!relative_z(key_px_prev, track.rec.px.offsets_px, z)) { flags |= NO_INVERSE; return false; }
    rf::Opts ro;
    refine_opts(o, ro);
    if (!rf::refine_measurement(track.rec, accepted_total, ro, k_net_cov, out72, r_px, flags)) return false;
    for (int k = 0; k < 8; k++) out72[k] = z_px[k] = z[k];
    return true;
}

}  /* namespace hnet_kfm */

namespace hnet_ekf {

/* The host twin of a measuring session's whole step.  m: null = the feature is off for this filter, and everything is iterated_update_photo_gated's, bit
 * for bit (out: zeros).  Otherwise the network's iterations run as there but with update_offset = true on the last one as well and no reset; then the
 * rule of hnet_kfm on the session `ks` (its keyframe state and prev_ok, both advanced as the device advances them): align(start_px [8] float, rec,
 * accepted_total) is the caller's robust alignment keyframe -> current frame (it is not called for a session without a keyframe; a start of quiet NaNs
 * must give the DEGENERATE record the device's alignment gives).  *copy: decide's copy flag (the current frame becomes the keyframe).  The reset follows.
 * Returns the updates applied, the keyframe update included. */
template <class Net, class Vec8, class Photo, class Align>
inline int iterated_update_keyframe_measured(State& s, Net& net, int max_iekf_iteration, double k_net_cov, Vec8& prior_px_vec, double time_stamp, double max_nis,
                                             Innovation* rec, Photo& photo, double max_ratio, int min_inside, PhotoRecord* prec, const hnet_kfm::Opts* m, bool gap,
                                             hnet_kfm::Session& ks, Align& align, hnet_kfm::Record& out, int* copy) {
    namespace kfm = hnet_kfm;
    std::memset(&out, 0, sizeof out);
    if (copy) *copy = 0;
    if (!m) return iterated_update_photo_gated(s, net, max_iekf_iteration, k_net_cov, prior_px_vec, time_stamp, max_nis, rec, photo, max_ratio, min_inside, prec);
    /* iterated_update_photo_gated's loop with update_offset = true throughout and the reset left to the end */
    int done = 0;
    bool skip = false, singular = false;
    const bool gated = max_ratio > 0.0;
    for (int it = 0; it < max_iekf_iteration; it++) {
        std::memset(&rec[it], 0, sizeof rec[it]);
        rec[it].flag = INNOV_NONE;
    }
    std::memset(prec, 0, sizeof(PhotoRecord) * (size_t)(1 + max_iekf_iteration));
    for (int it = 0; it < max_iekf_iteration; it++) {
        double prior_px[8], prior_cam[8];
        prior_pixels(s, prior_px, prior_cam);
        for (int i = 0; i < 8; i++) prior_px_vec[i] = prior_px[i];
        if (gated && it == 0) {
            double p32[8];
            for (int i = 0; i < 8; i++) p32[i] = (double)(float)prior_px[i];
            prec[0] = photo(p32);
        }
        net.network_inference(prior_px_vec, it);
        if (net.get_latest_inference_time() == time_stamp && net.img_counter > 10) {
            if (skip) { rec[it].flag = INNOV_SKIPPED; continue; }
            const auto mm = net.get_pred_mean();
            const auto C = net.get_pred_Cov();
            double mean[8], cov[64];
            for (int i = 0; i < 8; i++) {
                mean[i] = mm(i, 0);
                for (int j = 0; j < 8; j++) cov[i * 8 + j] = C(i, j);
            }
            if (gated) {
                prec[1 + it] = photo(mean);
                if (photo_reject(prec[0], prec[1 + it], max_ratio, min_inside)) {
                    prec[1 + it].flags |= PHOTO_REJECTED;
                    rec[it].flag = INNOV_SKIPPED;
                    skip = true;
                    continue;
                }
            }
            innovation(s, mean, cov, prior_cam, k_net_cov, rec[it]);
            if (max_nis > 0.0 && rec[it].nis > max_nis) {
                rec[it].flag = INNOV_REJECTED;
                skip = true;
                continue;
            }
            if (!update(s, mean, cov, prior_cam, k_net_cov, true)) {
                for (int k = it + 1; k < max_iekf_iteration; k++) rec[k].flag = INNOV_SKIPPED;
                singular = true;
                break;
            }
            done++;
        }
    }
    /* 1, 2: the step and the track */
    const bool had_key = ks.key.has_key != 0;
    float key_prev[8], start[8];
    for (int k = 0; k < 8; k++) {
        out.step_px[k] = kfm::step_entry(s, k);
        key_prev[k] = ks.key.key_px[k];
        start[k] = hnet_keyframe::quiet_nan();
    }
    int accepted_total = 0;
    hnet_robust::Record arec;
    std::memset(&arec, 0, sizeof arec);
    if (had_key) {
        hnet_keyframe::compose(out.step_px, key_prev, start);
        align(start, arec, accepted_total);
        out.track.rec = arec;
    }
    const int cp = hnet_keyframe::decide(ks.key, start, arec, m->track, gap, ks.key, out.track);
    if (copy) *copy = cp;
    /* 3 .. 5 */
    out.flags = kfm::ASKED;
    out.iteration = max_iekf_iteration;
    out.flag = INNOV_NONE;
    float m72[72];
    const bool ok = kfm::measure(had_key, key_prev, ks.prev_ok, out.track, accepted_total, *m, k_net_cov, out.z_px, out.r_px, m72, out.flags);
    const bool sel = kfm::selected(m->when, singular ? -1 - done : done);
    if (!sel) out.flags |= kfm::NOT_SELECTED;
    if (ok && sel) {
        double prior_px[8], prior_cam[8], mean[8], cov[64];
        prior_pixels(s, prior_px, prior_cam);
        for (int i = 0; i < 8; i++) mean[i] = (double)m72[i];
        for (int e = 0; e < 64; e++) cov[e] = (double)m72[8 + e];
        Innovation inn;
        innovation(s, mean, cov, prior_cam, k_net_cov, inn);
        std::memcpy(out.r, inn.r, sizeof out.r);
        std::memcpy(out.s_diag, inn.s_diag, sizeof out.s_diag);
        out.nis = inn.nis;
        out.flag = inn.flag;
        if (max_nis > 0.0 && inn.nis > max_nis) {
            out.flag = INNOV_REJECTED;
            out.flags |= kfm::NIS_REJECTED;
        } else if (!update(s, mean, cov, prior_cam, k_net_cov, false)) {
            out.flags |= kfm::S_SINGULAR;
        } else {
            out.flags |= kfm::APPLIED;
            done++;
        }
    }
    ks.prev_ok = kfm::next_prev_ok(out.track.flags);
    reset_4pt_offset(s);
    return done;
}

}  /* namespace hnet_ekf */

#endif /* HNET_KEYFRAME_MEASURE_H */
