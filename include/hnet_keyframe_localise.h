/* hnet_keyframe_localise.h — a camera localised against its RENDERED keyframe map (include/hnet.h hnet_op_keyframe_localise): which entries take
 * part, where the masked alignment starts, the verdict on its record and the correction of the chain.  What the device
 * (csrc/kernels_keyframe_localise.hip) and the host reference (tests/cpp/keyframe_localise_ref.cpp) both compile, on top of include/hnet_keyframe_map.h
 * and include/hnet_keyframe_render.h.  Everything is in double, every body is non-contracting, nothing depends on the batch.
 *
 * Eligible: select's preference carried over - a valid entry with slot != cur_slot and links < cur_links.  Without a map state (the operator-level call)
 *   every valid entry is eligible.
 * Template: the eligible entries rendered into the view h_origin_before (the current frame as the chain predicts it) at 320 x 224 by the unchanged
 *   render; used_mask = eligible AND set-up; the cover image is the alignment's mask and n_covered the render record's.
 * Start: zeros; quiet NaNs when no entry took part or n_covered / 71 680 < min_cover (the alignment stops DEGENERATE at once, as in 7q).
 * Verdict, one flag, in this order: LOC_NO_MAP (used_mask == 0), LOC_LOW_COVER, LOC_STOPPED (the record stopped SINGULAR, DEGENERATE or FEW_PIXELS),
 *   LOC_MSE_ABOVE_MAX (max_mse > 0 and not mse <= max_mse), LOC_NON_FINITE (an offset), LOC_LOW_OVERLAP (n_valid / 71 680 < min_overlap),
 *   LOC_SHIFT_ABOVE_MAX (max_shift_px > 0 and the worst |offset| above it), LOC_CHAIN, otherwise LOC_LOCALISED.  On LOCALISED
 *   h_origin_curr = chain(H(offsets), h_origin_before): the template is the predicted view and the alignment maps it to the current frame.
 *   correction_px = corners(h_origin_curr) - corners(h_origin_before), zeros unless localised.  links = 1 + the largest links in used_mask when localised,
 *   links_before otherwise.
 * Apply (opts.apply = 1, a state given, LOCALISED only): key_px stays; h_origin_key' = chain(inverse(H(key_px)), h_origin_curr), the held keyframe's
 *   place as the less-drifted ground sees it - LOC_CHAIN if that fails; the entry of cur_slot follows when cur_slot >= 0; cur_links and that entry's links
 *   become the record's links.  Age, keyframes, images, cursor and serial stay.  A rejected call or apply = 0 changes no byte of any state.
 * The defaults (robust defaults, 3 levels, FEWEST_LINKS, min_cover 0.5, min_overlap 0.4, no max_mse, no max_shift_px, apply 0) are CHOICES, not
 *   measurements.
 */
#ifndef HNET_KEYFRAME_LOCALISE_H
#define HNET_KEYFRAME_LOCALISE_H

#include "hnet_keyframe_render.h"

namespace hnet_localise {

namespace kf = hnet_keyframe;
namespace km = hnet_keyframe_map;
namespace kr = hnet_keyframe_render;
namespace pa = hnet_align;
namespace pr = hnet_robust;

/* the flags of a localise record (= HNET_LOC_*) */
enum { LOC_NO_MAP = 1, LOC_LOW_COVER = 2, LOC_STOPPED = 4, LOC_MSE_ABOVE_MAX = 8, LOC_NON_FINITE = 16, LOC_LOW_OVERLAP = 32, LOC_SHIFT_ABOVE_MAX = 64,
       LOC_CHAIN = 128, LOC_LOCALISED = 256 };

/* = hnet_keyframe_localise_opts */
struct Opts { pr::Opts align; int32_t levels, mode; double min_cover, min_overlap, max_mse, max_shift_px; int32_t apply, pad; };
inline void default_opts(Opts& o) {
    pr::default_opts(o.align);
    o.levels = 3; o.mode = kr::FEWEST_LINKS; o.min_cover = 0.5; o.min_overlap = 0.4; o.max_mse = 0.0; o.max_shift_px = 0.0; o.apply = 0; o.pad = 0;
}
inline bool opts_valid(const Opts& o) {
    return pr::opts_valid(o.align) && o.levels >= 1 && o.levels <= pa::MAX_LEVELS && o.mode >= 0 && o.mode < kr::N_MODES && o.min_cover >= 0.0 && o.min_cover <= 1.0 &&
           o.min_overlap >= 0.0 && o.min_overlap <= 1.0 && o.max_mse >= 0.0 && std::isfinite(o.max_mse) && o.max_shift_px >= 0.0 && std::isfinite(o.max_shift_px) &&
           (o.apply == 0 || o.apply == 1);
}

/* = hnet_keyframe_localise */
struct Localise {
    pr::Record rec;                 /* the level-0 record of the masked alignment (zeros when nothing was aligned: NO_MAP, LOW_COVER) */
    double h_origin_before[9], h_origin_curr[9], correction_px[pa::NX], cover, overlap;
    int32_t used_mask, links_before, links, flags, pad[2];
};

/* the slots that may take part, before any geometry; m == nullptr: every valid entry */
inline int eligible_mask(const km::MapState* m, const km::Entry* e, int capacity) {
    int mask = 0;
    for (int j = 0; j < capacity; j++)
        if (m ? km::eligible(*m, e[j], j) : e[j].valid != 0) mask |= 1 << j;
    return mask;
}

inline bool covered(int used_mask, uint64_t n_covered, const Opts& o) {
    HNET_ALIGN_NO_CONTRACT
    return used_mask != 0 && !((double)n_covered / kf::FRAME_PIXELS < o.min_cover);
}

/* where the alignment starts */
inline void start(int used_mask, uint64_t n_covered, const Opts& o, float x0[pa::NX]) {
    const bool go = covered(used_mask, n_covered, o);
    for (int k = 0; k < pa::NX; k++) x0[k] = go ? 0.0f : kf::quiet_nan();
}

/* 1 + the largest links of the entries in used_mask (0 for an empty mask; only slots below the capacity are read) */
inline int links_after(const km::Entry* e, int capacity, int used_mask) {
    int top = -1;
    for (int j = 0; j < capacity; j++)
        if (((used_mask >> j) & 1) && e[j].links > top) top = e[j].links;
    return top < 0x7fffffff ? top + 1 : top;      /* (links from outside the rule: no overflow) */
}

/* The verdict and the record but for out.rec, which is the caller's (the level-0 record, or zeros when nothing was aligned).  s / m: the session's state
 * and map state, or both nullptr (the operator-level call: links_before = 0, nothing to apply).  With opts.apply = 1, states given and LOCALISED, ns / nm
 * / ne [capacity] receive the applied states; otherwise they receive copies of s / m / e (when given).  s and ns, m and nm, e and ne may be the same
 * objects.  Returns 1 when localised. */
inline int decide_localise(const kf::State* s, const km::MapState* m, const km::Entry* e, int capacity, int used_mask, uint64_t n_covered,
                           const double h_before[9], const pr::Record& rec, const Opts& o, kf::State* ns, km::MapState* nm, km::Entry* ne, Localise& out) {
    HNET_ALIGN_NO_CONTRACT
    double hb[9], hc[9], hx[9], hk[9], inv[9], cb[8], ca[8];
    for (int k = 0; k < 9; k++) hb[k] = hc[k] = hk[k] = h_before[k];
    const int links_before = m ? m->cur_links : 0;
    const double cover = (double)n_covered / kf::FRAME_PIXELS;
    const bool aligned = covered(used_mask, n_covered, o);
    const double overlap = aligned ? (double)rec.px.n_valid / kf::FRAME_PIXELS : 0.0;
    int flags;
    if (used_mask == 0) flags = LOC_NO_MAP;
    else if (!aligned) flags = LOC_LOW_COVER;
    else {
        bool finite = true;
        double worst = 0.0;
        for (int k = 0; k < 8; k++) {
            finite = finite && std::isfinite(rec.px.offsets_px[k]);
            const double d = std::fabs((double)rec.px.offsets_px[k]);
            worst = d > worst ? d : worst;
        }
        if (rec.px.flags & (pa::SINGULAR | pa::DEGENERATE | pa::FEW_PIXELS)) flags = LOC_STOPPED;
        else if (o.max_mse > 0.0 && !(rec.px.mse <= o.max_mse)) flags = LOC_MSE_ABOVE_MAX;
        else if (!finite) flags = LOC_NON_FINITE;
        else if (overlap < o.min_overlap) flags = LOC_LOW_OVERLAP;
        else if (o.max_shift_px > 0.0 && !(worst <= o.max_shift_px)) flags = LOC_SHIFT_ABOVE_MAX;
        else if (!kf::homography(rec.px.offsets_px, hx) || !kf::chain(hx, hb, hc)) flags = LOC_CHAIN;
        else flags = LOC_LOCALISED;
    }
    const bool apply = flags == LOC_LOCALISED && o.apply == 1 && s && m;
    if (apply && !(kf::homography(s->key_px, hx) && km::inverse(hx, inv) && kf::chain(inv, hc, hk))) flags = LOC_CHAIN;
    const bool localised = flags == LOC_LOCALISED;
    const int links = localised ? links_after(e, capacity, used_mask) : links_before;
    if (s && ns) {
        const kf::State keep = *s;
        *ns = keep;
    }
    if (m && nm) {
        const km::MapState keep = *m;
        *nm = keep;
    }
    if (e && ne && ne != e)
        for (int j = 0; j < capacity; j++) ne[j] = e[j];
    if (apply && localised) {
        const int slot = m->cur_slot;
        if (ns)
            for (int k = 0; k < 9; k++) ns->h_origin_key[k] = hk[k];
        if (nm) nm->cur_links = links;
        if (ne && slot >= 0 && slot < capacity) {
            for (int k = 0; k < 9; k++) ne[slot].h_origin_key[k] = hk[k];
            ne[slot].links = links;
        }
    }
    for (int k = 0; k < 8; k++) out.correction_px[k] = 0.0;
    if (localised) {
        km::corners(hb, cb);
        km::corners(hc, ca);
        for (int k = 0; k < 8; k++) out.correction_px[k] = ca[k] - cb[k];
    } else {
        for (int k = 0; k < 9; k++) hc[k] = hb[k];
    }
    for (int k = 0; k < 9; k++) { out.h_origin_before[k] = hb[k]; out.h_origin_curr[k] = hc[k]; }
    out.cover = cover;
    out.overlap = overlap;
    out.used_mask = used_mask; out.links_before = links_before; out.links = links; out.flags = flags; out.pad[0] = 0; out.pad[1] = 0;
    return localised ? 1 : 0;
}

}  /* namespace hnet_localise */

#endif /* HNET_KEYFRAME_LOCALISE_H */
