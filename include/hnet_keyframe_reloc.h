/* hnet_keyframe_reloc.h — finding a lost camera among its keyframes (include/hnet.h hnet_sessions_keyframe_relocalise): the choice among the
 * searched candidates and the rule that re-tracks the session on its HELD keyframe.  What the device (csrc/kernels_photo_search.hip) and the host
 * reference (tests/cpp/photo_search_ref.cpp) both compile, on top of include/hnet_keyframe_map.h (a map entry is decided by its decide_revisit exactly as
 * it is) and include/hnet_photo_search.h (the search that gives every candidate its start).
 *
 * The candidates of a session, in this order: index 0 is the held keyframe (target -1); with a map, index 1 + slot is every valid entry with
 * slot != cur_slot.  There is no condition on links and no chain prediction.  Each is searched against the session's current frame.  The pick is the FOUND
 * candidate of the highest score; ties go to the held keyframe, then the lower slot (offer, in the order of the indices).  None: RL_NO_CANDIDATE.
 * decide_relocalise, for the held keyframe, on the level-0 record of the alignment keyframe -> curr from the searched start: one REJECTED reason, tested
 *   in decide_revisit's order and with its meaning, without RV_CHAIN: RL_STOPPED, RL_MSE_ABOVE_MAX, RL_NON_FINITE, RL_LOW_OVERLAP, RL_CLOSURE_ABOVE_MAX
 *   (the worst |offset - searched start|).  Else RL_RETRACKED: key_px = the record's offsets, everything else of the state and the map state unchanged.
 * Choices the rule left open.  The record's first part has the layout of hnet_keyframe_map::Revisit, which decide_revisit writes for a map entry and
 *   decide_relocalise for the held keyframe (slot -1, links 0); grid is 0 in both: nothing is predicted.  For the held keyframe h_origin_curr =
 *   chain(H(offsets), h_origin_key) when RETRACKED, and h_origin_before when that product is degenerate (the next track restarts the origin, as it
 *   would have) or when rejected; closure_px as 7q defines it.  The RL_* flags share the values of RV_* and add RL_RETRACKED.  The search record of a
 *   call without a pick is all zero; target is then -2.
 * Every body is non-contracting, everything is in double, nothing depends on the batch.
 */
#ifndef HNET_KEYFRAME_RELOC_H
#define HNET_KEYFRAME_RELOC_H

#include "hnet_keyframe_map.h"
#include "hnet_photo_search.h"

namespace hnet_keyframe_reloc {

namespace kf = hnet_keyframe;
namespace km = hnet_keyframe_map;
namespace ps = hnet_search;
namespace pa = hnet_align;
namespace pr = hnet_robust;

constexpr int MAX_CANDIDATES = km::MAX_CAPACITY + 1;
constexpr int TARGET_NONE = -2, TARGET_HELD = -1;

/* the flags of a relocalise record (= HNET_RL_*): RV_*'s values, and RETRACKED */
enum { RL_NO_CANDIDATE = km::RV_NO_CANDIDATE, RL_ATTACHED = km::RV_ATTACHED, RL_STOPPED = km::RV_STOPPED, RL_MSE_ABOVE_MAX = km::RV_MSE_ABOVE_MAX,
       RL_NON_FINITE = km::RV_NON_FINITE, RL_LOW_OVERLAP = km::RV_LOW_OVERLAP, RL_CLOSURE_ABOVE_MAX = km::RV_CLOSURE_ABOVE_MAX, RL_CHAIN = km::RV_CHAIN,
       RL_RETRACKED = 256, RL_REJECTED = km::RV_REJECTED };

/* = hnet_keyframe_relocalise_opts */
struct Opts { pr::Opts align; int32_t levels, pad; ps::Opts search; double min_overlap, max_mse, max_closure_px; };
inline void default_opts(Opts& o) {
    pr::default_opts(o.align);
    ps::default_opts(o.search);
    o.levels = 4; o.pad = 0; o.min_overlap = 0.5; o.max_mse = 0.0; o.max_closure_px = 0.0;
}
/* the options decide_revisit reads of a relocalise's (min_grid is not read by it) */
inline void revisit_opts(const Opts& o, km::Opts& m) {
    m.align = o.align; m.levels = o.levels; m.min_grid = 1; m.min_overlap = o.min_overlap; m.max_mse = o.max_mse; m.max_closure_px = o.max_closure_px;
}
inline bool opts_valid(const Opts& o) {
    km::Opts m;
    revisit_opts(o, m);
    return km::opts_valid(m) && ps::opts_valid(o.search);
}

/* = hnet_keyframe_relocalise */
struct Reloc {
    km::Revisit rv;
    ps::Record search;
    int32_t target, n_searched, n_found, pad;
};

/* what the pick keeps: the candidate index (-1: none) and its score */
struct Pick { int32_t index; double score; };
inline void pick_none(Pick& p) { p.index = -1; p.score = -1.0; }
/* one searched candidate, offered in the order of the indices: kept when FOUND and strictly better than what p holds */
inline void offer(Pick& p, int index, const ps::Record& r) {
    if (r.flags != ps::FOUND) return;
    if (p.index >= 0 && !(r.score > p.score)) return;
    p.index = index; p.score = r.score;
}
inline int target_of(int index) { return index < 0 ? TARGET_NONE : index - 1; }

/* s and ns may be the same object, as may start_px / h_before and the fields of out.  out.rec is the caller's, as in decide_revisit. */
inline void decide_relocalise(const kf::State& s, const float* start_px, const double* h_before, const pr::Record& rec, const Opts& o, kf::State& ns,
                              km::Revisit& out) {
    HNET_ALIGN_NO_CONTRACT
    double hb[9], hc[9], hx[9], cb[8], ca[8];
    float start[8], key[8];
    for (int k = 0; k < 9; k++) hb[k] = hc[k] = h_before[k];
    for (int k = 0; k < 8; k++) { start[k] = start_px[k]; key[k] = s.key_px[k]; }
    const kf::State keep = s;
    const double overlap = (double)rec.px.n_valid / kf::FRAME_PIXELS;
    bool rec_finite = true;
    double worst = 0.0;
    for (int k = 0; k < 8; k++) {
        rec_finite = rec_finite && std::isfinite(rec.px.offsets_px[k]);
        const double d = std::fabs((double)rec.px.offsets_px[k] - (double)start[k]);
        worst = d > worst ? d : worst;
    }
    int flags;
    if (rec.px.flags & (pa::SINGULAR | pa::DEGENERATE | pa::FEW_PIXELS)) flags = RL_STOPPED;
    else if (o.max_mse > 0.0 && !(rec.px.mse <= o.max_mse)) flags = RL_MSE_ABOVE_MAX;
    else if (!rec_finite) flags = RL_NON_FINITE;
    else if (overlap < o.min_overlap) flags = RL_LOW_OVERLAP;
    else if (o.max_closure_px > 0.0 && !(worst <= o.max_closure_px)) flags = RL_CLOSURE_ABOVE_MAX;
    else flags = RL_RETRACKED;
    ns = keep;
    for (int k = 0; k < 8; k++) out.closure_px[k] = 0.0;
    if (flags == RL_RETRACKED) {
        for (int k = 0; k < 8; k++) key[k] = rec.px.offsets_px[k];
        for (int k = 0; k < 8; k++) ns.key_px[k] = key[k];
        if (kf::homography(key, hx) && kf::chain(hx, keep.h_origin_key, hc)) {
            km::corners(hb, cb);
            km::corners(hc, ca);
            for (int k = 0; k < 8; k++) out.closure_px[k] = ca[k] - cb[k];
        }
    }
    for (int k = 0; k < 8; k++) { out.start_px[k] = start[k]; out.key_px[k] = key[k]; }
    for (int k = 0; k < 9; k++) { out.h_origin_before[k] = hb[k]; out.h_origin_curr[k] = hc[k]; }
    out.overlap = overlap;
    out.slot = TARGET_HELD; out.links = 0; out.grid = 0; out.flags = flags; out.pad[0] = 0; out.pad[1] = 0;
}

}  /* namespace hnet_keyframe_reloc */

#endif /* HNET_KEYFRAME_RELOC_H */
