/* hnet_keyframe_measure_recover.h — recovering a lost camera INSIDE the in-step keyframe track of hnet_filters (include/hnet.h
 * hnet_filters_set_keyframe_recover), dependency free: what the device (csrc/kernels_filters_keyframe_recover.hip) and the host reference
 * (tests/cpp/filters_keyframe_recover_ref.cpp) both compile, on top of the unedited include/hnet_keyframe_measure.h (7v: the step, z, the measurement, the
 * selection) and include/hnet_keyframe_recover.h (7u: decide_deferred, finish, the zero relocalise record).
 *
 * The rule, per stepping session with measure AND recover on.  Steps 1 and 5 are 7v's.
 *   2 the track is hnet_sessions_keyframe_track_recover with the filter's own step_px, the session's gap, the measure options' `track` block and the
 *     recover options' reloc block and table: decide_deferred, the oriented relocalisation of a LOST session on T0's state, finish.  A measuring session
 *     without recovery in the same call gets the plain decide (recover_on = 0: active = 0, the stash is zero, its relocalise record is zero_reloc).
 *   3 UNUSABLE, one reason bit, tested in this order: FIRST; TRACK_LOST: the record has a LOST bit and not RECOVERED; REATTACHED: RECOVERED and the
 *     relocalise record has RL_ATTACHED - the keyframe changed under the session, the frame has no consecutive-frame meaning and is FIRST-like;
 *     TRACK_GAP; PREV_NOT_MEASURED; NO_INVERSE; then refine_measurement's reasons in their order.
 *   4 the source of the measurement: not recovered: track.rec, as in 7v.  RECOVERED with RL_RETRACKED: the relocalise's level-0 record reloc.rv.rec: z_px =
 *     relative_z(key_px before the call, its offsets), R_px is refine_measurement's on it with the trials accepted over the levels of the SECOND
 *     alignment, and the informational bit FROM_RELOC is set (not an UNUSABLE reason).
 *   next prev_ok: 0 only for LOST without RECOVERED; 1 after RETRACKED and after REATTACHED (the next frame measures against the relocalise's key_px).
 * Choices the rule fixes: no fine stage (7x) inside the step; no re-key is judged on a recovered frame (7u's choice); a recovered frame's z_px may lie far
 *   from the prior - a kidnapped camera really did move - and whether it is applied is the session's NIS gate's business; `when` applies unchanged.
 * Every body is non-contracting and in double; nothing depends on the batch.
 */
#ifndef HNET_KEYFRAME_MEASURE_RECOVER_H
#define HNET_KEYFRAME_MEASURE_RECOVER_H

#include "hnet_keyframe_measure.h"
#include "hnet_keyframe_recover.h"

namespace hnet_kfmr {

namespace kfm = hnet_kfm;
namespace kr = hnet_keyframe_recovery;
namespace kf = hnet_keyframe;
namespace rl = hnet_keyframe_reloc;
namespace rf = hnet_refine;
namespace pr = hnet_robust;

/* the flags this layer adds to a measure record (= HNET_KFM_FROM_RELOC, HNET_KFM_REATTACHED) and the wider mask (= HNET_KFMR_UNUSABLE) */
enum { FROM_RELOC = 65536,             /* the measurement was taken from the relocalise's record; informational */
       REATTACHED = 131072,            /* UNUSABLE: the frame was re-attached to a map keyframe */
       UNUSABLE = kfm::UNUSABLE | REATTACHED };
static_assert(((FROM_RELOC | REATTACHED) & (kfm::UNUSABLE | kfm::NOT_SELECTED | 15)) == 0, "the new bits are bits of their own");

/* = hnet_keyframe_measure_recover: 7v's record, then the relocalise's (zero_reloc for a session that needed none or has the feature off) */
struct Record { kfm::Record m; kr::Reloc reloc; };
static_assert(sizeof(Record) == sizeof(kfm::Record) + sizeof(kr::Reloc) && offsetof(Record, reloc) == sizeof(kfm::Record), "packed");

/* what can be judged before any matrix is formed: 0, or the reason bit.  track_flags: the record after finish; reloc_flags: reloc.rv.flags */
inline int usable_recover(bool had_key, int track_flags, int reloc_flags, int prev_ok) {
    if (!had_key) return kfm::FIRST;
    const bool recovered = (track_flags & kr::RECOVERED) != 0;
    if ((track_flags & kf::LOST) && !recovered) return kfm::TRACK_LOST;
    if (recovered && (reloc_flags & rl::RL_ATTACHED)) return REATTACHED;
    if (track_flags & kf::GAP) return kfm::TRACK_GAP;
    if (!prev_ok) return kfm::PREV_NOT_MEASURED;
    return 0;
}
/* prev_ok after a track with recovery */
inline int next_prev_ok_recover(int track_flags) { return ((track_flags & kf::LOST) && !(track_flags & kr::RECOVERED)) ? 0 : 1; }
/* whether the measurement comes from the relocalise's record (a usable session: ATTACHED was refused before) */
inline bool from_reloc(int track_flags) { return (track_flags & kr::RECOVERED) != 0; }

/* Steps 3 and 4.  As hnet_kfm::measure, with the relocalise's record and the trials accepted over the levels of its alignment.  A record without
 * RECOVERED (recovery off, not lost, unrecovered) gives what hnet_kfm::measure gives, bit for bit. */
inline bool measure_recover(bool had_key, const float* key_px_prev, int prev_ok, const kf::Track& track, int accepted_total, const kr::Reloc& reloc,
                            int accepted_reloc, const kfm::Opts& o, double k_net_cov, float* z_px, double* r_px, float* out72, int32_t& flags) {
    if (const int why = usable_recover(had_key, track.flags, reloc.rv.flags, prev_ok)) { flags |= why; return false; }
    const bool from = from_reloc(track.flags);
    const pr::Record& src = from ? reloc.rv.rec : track.rec;
    float z[8];
    if (!kfm::relative_z(key_px_prev, src.px.offsets_px, z)) { flags |= kfm::NO_INVERSE; return false; }
    rf::Opts ro;
    kfm::refine_opts(o, ro);
    if (!rf::refine_measurement(src, from ? accepted_reloc : accepted_total, ro, k_net_cov, out72, r_px, flags)) return false;
    for (int k = 0; k < 8; k++) out72[k] = z_px[k] = z[k];
    if (from) flags |= FROM_RELOC;
    return true;
}

}  /* namespace hnet_kfmr */

namespace hnet_ekf {

/* The host twin of a measuring AND recovering session's whole step: iterated_update_keyframe_measured around two caller-supplied callables.  r: null =
 * recovery is off, and everything IS iterated_update_keyframe_measured, byte for byte (out.reloc: zero_reloc when m is set, zeros with the feature off).
 * align: as there.  reloc(state, track, copy, rec, accepted_total): called for a LOST session only, between decide_deferred and finish: the caller's
 * first commit for (track.flags, copy) - the map's note; copy is always 0 for a lost session - then its oriented relocalisation on `state` (T0's), which
 * it advances; rec: the relocalise record, accepted_total: the trials accepted over the levels of its alignment.  *copy: the copy flag of the FIRST
 * commit (for a session that was not lost: decide's; the caller commits it), *copy2: the second commit's (an unrecovered session: T1's). */
template <class Net, class Vec8, class Photo, class Align, class Relocalise>
inline int iterated_update_keyframe_recovered(State& s, Net& net, int max_iekf_iteration, double k_net_cov, Vec8& prior_px_vec, double time_stamp, double max_nis,
                                              Innovation* rec, Photo& photo, double max_ratio, int min_inside, PhotoRecord* prec, const hnet_kfm::Opts* m,
                                              const hnet_keyframe_reloc::Opts* r, bool gap, hnet_kfm::Session& ks, Align& align, Relocalise& reloc,
                                              hnet_kfmr::Record& out, int* copy, int* copy2) {
    namespace kfm = hnet_kfm;
    namespace kfmr = hnet_kfmr;
    namespace kr = hnet_keyframe_recovery;
    if (copy2) *copy2 = 0;
    if (!m || !r) {
        const int done = iterated_update_keyframe_measured(s, net, max_iekf_iteration, k_net_cov, prior_px_vec, time_stamp, max_nis, rec, photo, max_ratio, min_inside,
                                                           prec, m, gap, ks, align, out.m, copy);
        if (m) kr::zero_reloc(out.reloc);
        else std::memset(&out.reloc, 0, sizeof out.reloc);
        return done;
    }
    std::memset(&out, 0, sizeof out);
    if (copy) *copy = 0;
    /* iterated_update_keyframe_measured's loop */
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
    /* 1, 2: the step and the track with recovery */
    const bool had_key = ks.key.has_key != 0;
    float key_prev[8], start[8];
    for (int k = 0; k < 8; k++) {
        out.m.step_px[k] = kfm::step_entry(s, k);
        key_prev[k] = ks.key.key_px[k];
        start[k] = hnet_keyframe::quiet_nan();
    }
    int accepted_total = 0, accepted_reloc = 0, active = 0;
    hnet_robust::Record arec;
    std::memset(&arec, 0, sizeof arec);
    if (had_key) {
        hnet_keyframe::compose(out.m.step_px, key_prev, start);
        align(start, arec, accepted_total);
        out.m.track.rec = arec;
    }
    kr::Stash stash;
    const int cp = kr::decide_deferred(ks.key, start, arec, m->track, gap, ks.key, out.m.track, stash, active);
    if (copy) *copy = cp;
    kr::zero_reloc(out.reloc);
    if (active) {
        reloc(ks.key, out.m.track, cp, out.reloc, accepted_reloc);
        const int cp2 = kr::finish(out.reloc.rv.flags, stash, ks.key, out.m.track);
        if (copy2) *copy2 = cp2;
    }
    /* 3 .. 5 */
    out.m.flags = kfm::ASKED;
    out.m.iteration = max_iekf_iteration;
    out.m.flag = INNOV_NONE;
    float m72[72];
    const bool ok = kfmr::measure_recover(had_key, key_prev, ks.prev_ok, out.m.track, accepted_total, out.reloc, accepted_reloc, *m, k_net_cov, out.m.z_px, out.m.r_px,
                                          m72, out.m.flags);
    const bool sel = kfm::selected(m->when, singular ? -1 - done : done);
    if (!sel) out.m.flags |= kfm::NOT_SELECTED;
    if (ok && sel) {
        double prior_px[8], prior_cam[8], mean[8], cov[64];
        prior_pixels(s, prior_px, prior_cam);
        for (int i = 0; i < 8; i++) mean[i] = (double)m72[i];
        for (int e = 0; e < 64; e++) cov[e] = (double)m72[8 + e];
        Innovation inn;
        innovation(s, mean, cov, prior_cam, k_net_cov, inn);
        std::memcpy(out.m.r, inn.r, sizeof out.m.r);
        std::memcpy(out.m.s_diag, inn.s_diag, sizeof out.m.s_diag);
        out.m.nis = inn.nis;
        out.m.flag = inn.flag;
        if (max_nis > 0.0 && inn.nis > max_nis) {
            out.m.flag = INNOV_REJECTED;
            out.m.flags |= kfm::NIS_REJECTED;
        } else if (!update(s, mean, cov, prior_cam, k_net_cov, false)) {
            out.m.flags |= kfm::S_SINGULAR;
        } else {
            out.m.flags |= kfm::APPLIED;
            done++;
        }
    }
    ks.prev_ok = kfmr::next_prev_ok_recover(out.m.track.flags);
    reset_4pt_offset(s);
    return done;
}

}  /* namespace hnet_ekf */

#endif /* HNET_KEYFRAME_MEASURE_RECOVER_H */
