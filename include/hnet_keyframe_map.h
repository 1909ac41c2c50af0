/* hnet_keyframe_map.h — a MAP of keyframes per session and the closing of loops against it (include/hnet.h hnet_sessions_enable_keyframe_map,
 * hnet_sessions_keyframe_revisit): the bookkeeping that stores every keyframe a track takes, the composition that predicts where a stored
 * keyframe lies in the current frame, the choice of a candidate and the rule that re-attaches the session to it.  What the device
 * (csrc/kernels_keyframe_map.hip) and the host reference (tests/cpp/keyframe_map_ref.cpp) both compile, on top of include/hnet_keyframe.h (State, chain,
 * homography; the conventions are that header's).
 *
 * Per session: `capacity` entries (M, 2 .. 8) {valid, links, serial, h_origin_key} and one map state {cur_slot, cur_links, cursor, serial}.  links is the
 * number of chain links between the origin and that keyframe (fewer links = less accumulated drift), serial numbers the stored keyframes of a session
 * from 1 in the order they were stored.  Slot 0 is never evicted: it holds the oldest keyframe the chain knows.  Slots 1 .. M-1 are a ring.
 *
 * note(track_flags, copy, new State, map state, entries) -> store slot or -1: the bookkeeping after one track's decide.  ORIGIN_RESTARTED invalidates
 *   all entries (their h_origin_key refer to an origin that no longer exists) and sets cur_links = 0, cur_slot = -1.  With copy, the new keyframe is
 *   stored with the new state's h_origin_key: links = 0 for FIRST, else cur_links + 1; into slot 0 when that is invalid, else into slot 1 + cursor, and
 *   the cursor advances modulo M - 1; cur_slot and cur_links become the new entry's.  Otherwise nothing changes.
 * origin_curr(state, h): h_origin_curr = chain(H(key_px), h_origin_key), the chain's value for the frame the state's key_px describes.
 * inverse(a, inv) -> bool: adjugate / determinant, the one inverse of this header and of hnet_keyframe_render.h; false when |det| is below ORIGIN_TINY
 *   times the cube of the largest entry IN FRAME UNITS (a conjugated by diag(1 / 320, 1 / 320, 1), see the function) or anything is not finite.
 * relative(h_origin_curr, entry, G, start_px) -> bool: G = h_origin_curr . inverse(entry.h_origin_key); false when the inverse fails or anything is not
 *   finite.  G is renormalised to G[8] = 1 and maps a pixel of the stored keyframe to its position in the current frame.  start_px = the corners of G applied to p4, minus p4, rounded to fp32; false when a corner's z
 *   is not positive or a corner is not finite.
 * grid_inside(G, i), i in 0 .. 63: the template point (20 + 40 (i & 7), 14 + 28 (i >> 3)) is inside when z > 0, 0 <= x <= 319, 0 <= y <= 223.  The grid
 *   count is the number of points inside, of 64.  The grid is inset on purpose: a coarse test of visibility that a pixel of drift cannot flip at the
 *   frame's border.
 * select: over the valid entries with slot != cur_slot, links < cur_links, a successful relative and a grid count >= min_grid, the smallest links; on a
 *   tie the larger grid count; on a tie the lower slot.  Few links before much overlap: the oldest visible keyframe removes the most drift.  No such
 *   entry: slot -1 and a start of quiet NaNs.  The device offers the entries one by one (offer), counting the grid with a ballot.
 * decide_revisit -> the new State, the new map state, the output record and the attach flag.  Without a candidate RV_NO_CANDIDATE.  Otherwise one
 *   REJECTED reason, tested in this order: RV_STOPPED (the record stopped SINGULAR, DEGENERATE or FEW_PIXELS); RV_MSE_ABOVE_MAX (max_mse > 0 and not
 *   mse <= max_mse); RV_NON_FINITE (an offset of the record); RV_LOW_OVERLAP (n_valid / 71 680 < min_overlap); RV_CLOSURE_ABOVE_MAX (max_closure_px > 0
 *   and the worst |offset - start| exceeds it: the guard against a false match inside the basin); RV_CHAIN (chain(H(offsets), entry.h_origin_key)
 *   fails).  Else RV_ATTACHED: key_px = the record's offsets, h_origin_key = the entry's, age = 0, keyframes unchanged, cur_slot and cur_links the
 *   entry's.  A rejected or candidate-less revisit changes nothing in either state.
 * Choices the rule left open.  FIRST invalidates the entries like ORIGIN_RESTARTED does (a first keyframe is a new origin; after a reset the entries are
 *   already invalid, so this only matters to a caller of note by hand).  An ORIGIN_RESTARTED without copy leaves the map empty and the held keyframe
 *   outside it (cur_slot = -1) until the next re-key stores one with links 1.  serial goes on counting over a restart.  An attach does not touch cursor or
 *   serial, and the entry stays in the map.  The candidate must have STRICTLY fewer links than the current keyframe: re-attaching to an equal one gains
 *   nothing.  When origin_curr fails there is no candidate and h_origin_before is the state's h_origin_key.  The output's key_px is the new state's
 *   (the record's offsets when attached, else the session's unchanged key_px); overlap is the record's n_valid / 71 680 (0 without a candidate); slot,
 *   links and grid are the candidate's (-1, 0, 0 without one); closure_px is in double and is not judged.  decide_revisit does not touch out.rec: the
 *   caller copies the level-0 record there, or zeros without a candidate (no alignment result was read).
 * Every body is non-contracting, everything is in double, nothing depends on the batch.
 */
#ifndef HNET_KEYFRAME_MAP_H
#define HNET_KEYFRAME_MAP_H

#include "hnet_keyframe.h"

namespace hnet_keyframe_map {

namespace kf = hnet_keyframe;
namespace pa = hnet_align;
namespace pr = hnet_robust;

constexpr int MIN_CAPACITY = 2, MAX_CAPACITY = 8, GRID_POINTS = 64;

/* the flags of a revisit record (= HNET_RV_*) */
enum { RV_NO_CANDIDATE = 1,          /* no stored keyframe qualified: nothing was aligned */
       RV_ATTACHED = 2,              /* the session now tracks against the candidate */
       RV_STOPPED = 4,               /* REJECTED: the record stopped SINGULAR, DEGENERATE or FEW_PIXELS */
       RV_MSE_ABOVE_MAX = 8,         /* REJECTED: max_mse > 0 and not mse <= max_mse */
       RV_NON_FINITE = 16,           /* REJECTED: an entry of the record's offsets is not finite */
       RV_LOW_OVERLAP = 32,          /* REJECTED: n_valid / 71 680 < min_overlap */
       RV_CLOSURE_ABOVE_MAX = 64,    /* REJECTED: max_closure_px > 0 and the worst |offset - start| exceeds it */
       RV_CHAIN = 128,               /* REJECTED: H(offsets) . entry.h_origin_key is degenerate */
       RV_REJECTED = RV_STOPPED | RV_MSE_ABOVE_MAX | RV_NON_FINITE | RV_LOW_OVERLAP | RV_CLOSURE_ABOVE_MAX | RV_CHAIN };

/* = hnet_keyframe_revisit_opts */
struct Opts { pr::Opts align; int32_t levels, min_grid; double min_overlap, max_mse, max_closure_px; };
inline void default_opts(Opts& o) {
    pr::default_opts(o.align);
    o.levels = 3; o.min_grid = 32; o.min_overlap = 0.5; o.max_mse = 0.0; o.max_closure_px = 0.0;
}
inline bool opts_valid(const Opts& o) {
    return pr::opts_valid(o.align) && o.levels >= 1 && o.levels <= pa::MAX_LEVELS && o.min_grid >= 1 && o.min_grid <= GRID_POINTS && o.min_overlap >= 0.0 &&
           o.min_overlap <= 1.0 && o.max_mse >= 0.0 && std::isfinite(o.max_mse) && o.max_closure_px >= 0.0 && std::isfinite(o.max_closure_px);
}

/* = hnet_keyframe_map_entry: one stored keyframe of a session */
struct Entry { int32_t valid, links, serial, pad; double h_origin_key[9]; };
/* = hnet_keyframe_map_state: a session's map; all zero = empty (no entry is valid, so cur_slot is not read) */
struct MapState { int32_t cur_slot, cur_links, cursor, serial; };

/* = hnet_keyframe_revisit */
struct Revisit {
    pr::Record rec;
    float start_px[pa::NX], key_px[pa::NX];
    double h_origin_before[9], h_origin_curr[9], closure_px[pa::NX], overlap;
    int32_t slot, links, grid, flags, pad[2];
};

/* what select keeps */
struct Pick { int32_t slot, links, grid; float start_px[pa::NX]; };

inline int note(int track_flags, int copy, const kf::State& ns, MapState& m, Entry* e, int capacity) {
    if (track_flags & (kf::ORIGIN_RESTARTED | kf::FIRST)) {
        for (int i = 0; i < capacity; i++) e[i].valid = 0;
        m.cur_links = 0;
        m.cur_slot = -1;
    }
    if (!copy) return -1;
    int slot = 0;
    if (m.cursor < 0 || m.cursor >= capacity - 1) m.cursor = 0;      /* (a cursor from outside the rule never indexes past the ring) */
    if (e[0].valid) {
        slot = 1 + m.cursor;
        m.cursor = (m.cursor + 1) % (capacity - 1);
    }
    Entry& n = e[slot];
    n.valid = 1;
    n.links = (track_flags & kf::FIRST) ? 0 : m.cur_links + 1;
    n.serial = ++m.serial;
    n.pad = 0;
    for (int k = 0; k < 9; k++) n.h_origin_key[k] = ns.h_origin_key[k];
    m.cur_slot = slot;
    m.cur_links = n.links;
    return slot;
}

/* h_origin_curr of the frame the state's key_px describes; false (h = the state's h_origin_key) when H(key_px) or the product is degenerate */
inline bool origin_curr(const kf::State& s, double h[9]) {
    HNET_ALIGN_NO_CONTRACT
    double hx[9];
    for (int k = 0; k < 9; k++) h[k] = s.h_origin_key[k];
    return kf::homography(s.key_px, hx) && kf::chain(hx, s.h_origin_key, h);
}

/* the corners of m applied to p4, minus p4, in double; false when a corner's z is not positive or a corner is not finite (o is written either way) */
inline bool corners(const double m[9], double o[8]) {
    HNET_ALIGN_NO_CONTRACT
    bool ok = true;
    for (int c = 0; c < 4; c++) {
        const double u = hnet::p4(2 * c), v = hnet::p4(2 * c + 1);
        const double X = (m[0] * u + m[1] * v) + m[2], Y = (m[3] * u + m[4] * v) + m[5], Z = (m[6] * u + m[7] * v) + m[8];
        const double px = X / Z, py = Y / Z;
        ok = ok && Z > 0.0 && std::isfinite(px) && std::isfinite(py);
        o[2 * c] = px - u;
        o[2 * c + 1] = py - v;
    }
    return ok;
}

/* inv = adjugate(a) / det(a); false (inv untouched) when a is not finite or degenerate: |det| below ORIGIN_TINY times the cube of the largest entry of
 * a IN FRAME UNITS.  The entries of a homography mix units (pixels in [2] and [5], 1 / pixels in [6] and [7]), so the largest is taken over a conjugated by
 * diag(1 / 320, 1 / 320, 1): [2] and [5] divided by FRAME_UNIT, [6] and [7] multiplied by it, the rest as they are.  The determinant is the same either
 * way.  A translation by t px then counts as t / 320 frame widths and is refused beyond 320 x 10^4 = 3.2 x 10^6 px, not beyond 10^4 px. */
constexpr double FRAME_UNIT = 320.0;
inline bool inverse(const double a[9], double inv[9]) {
    HNET_ALIGN_NO_CONTRACT
    double adj[9];
    adj[0] = a[4] * a[8] - a[5] * a[7]; adj[1] = a[2] * a[7] - a[1] * a[8]; adj[2] = a[1] * a[5] - a[2] * a[4];
    adj[3] = a[5] * a[6] - a[3] * a[8]; adj[4] = a[0] * a[8] - a[2] * a[6]; adj[5] = a[2] * a[3] - a[0] * a[5];
    adj[6] = a[3] * a[7] - a[4] * a[6]; adj[7] = a[1] * a[6] - a[0] * a[7]; adj[8] = a[0] * a[4] - a[1] * a[3];
    const double det = (a[0] * adj[0] + a[1] * adj[3]) + a[2] * adj[6];
    double top = 0.0;
    bool ok = std::isfinite(det);
    for (int k = 0; k < 9; k++) {
        const double v = std::fabs(a[k]), f = (k == 2 || k == 5) ? v / FRAME_UNIT : (k == 6 || k == 7) ? v * FRAME_UNIT : v;
        top = f > top ? f : top;
        ok = ok && std::isfinite(a[k]);
    }
    if (!ok || !(std::fabs(det) >= kf::ORIGIN_TINY * ((top * top) * top)) || det == 0.0) return false;
    for (int k = 0; k < 9; k++) inv[k] = adj[k] / det;
    return true;
}

/* false: G and start_px hold nothing to be used */
inline bool relative(const double h_origin_curr[9], const Entry& e, double G[9], float start_px[8]) {
    HNET_ALIGN_NO_CONTRACT
    double inv[9], o[8];
    for (int k = 0; k < 9; k++)
        if (!std::isfinite(h_origin_curr[k])) return false;
    if (!inverse(e.h_origin_key, inv)) return false;
    if (!kf::chain(h_origin_curr, inv, G)) return false;
    if (!corners(G, o)) return false;
    for (int k = 0; k < 8; k++) start_px[k] = (float)o[k];
    return true;
}

inline bool grid_inside(const double G[9], int i) {
    HNET_ALIGN_NO_CONTRACT
    const double u = 20.0 + 40.0 * (double)(i & 7), v = 14.0 + 28.0 * (double)(i >> 3);
    const double X = (G[0] * u + G[1] * v) + G[2], Y = (G[3] * u + G[4] * v) + G[5], Z = (G[6] * u + G[7] * v) + G[8];
    const double x = X / Z, y = Y / Z;
    return Z > 0.0 && x >= 0.0 && x <= 319.0 && y >= 0.0 && y <= 223.0;
}

inline int grid_count(const double G[9]) {
    int n = 0;
    for (int i = 0; i < GRID_POINTS; i++) n += grid_inside(G, i) ? 1 : 0;
    return n;
}

inline void pick_none(Pick& p) {
    p.slot = -1; p.links = 0; p.grid = 0;
    for (int k = 0; k < 8; k++) p.start_px[k] = kf::quiet_nan();
}

/* whether the entry of `slot` may be a candidate at all, before any geometry */
inline bool eligible(const MapState& m, const Entry& e, int slot) { return e.valid != 0 && slot != m.cur_slot && e.links < m.cur_links; }

/* one eligible entry with a successful relative and its grid count, offered in the order of the slots: kept when it is better than what p holds */
inline void offer(Pick& p, int slot, const Entry& e, int grid, const float start_px[8], int min_grid) {
    if (grid < min_grid) return;
    if (p.slot >= 0 && !(e.links < p.links || (e.links == p.links && grid > p.grid))) return;
    p.slot = slot; p.links = e.links; p.grid = grid;
    for (int k = 0; k < 8; k++) p.start_px[k] = start_px[k];
}

inline void select(const MapState& m, const Entry* e, int capacity, const double h_origin_curr[9], int min_grid, Pick& p) {
    pick_none(p);
    for (int slot = 0; slot < capacity; slot++) {
        double G[9];
        float start[8];
        if (!eligible(m, e[slot], slot) || !relative(h_origin_curr, e[slot], G, start)) continue;
        offer(p, slot, e[slot], grid_count(G), start, min_grid);
    }
}

/* s and ns, m and nm may be the same objects, as may start_px / h_before and the fields of out; cand < 0: no candidate (entry is not read).  Returns
 * the attach flag.  out.rec is the caller's (see above). */
inline int decide_revisit(const kf::State& s, const MapState& m, const Entry* entry, int cand, int grid, const float* start_px, const double* h_before,
                          const pr::Record& rec, const Opts& o, kf::State& ns, MapState& nm, Revisit& out) {
    HNET_ALIGN_NO_CONTRACT
    double hb[9], hc[9], hx[9], cb[8], ca[8];
    float start[8], key[8];
    for (int k = 0; k < 9; k++) hb[k] = hc[k] = h_before[k];
    for (int k = 0; k < 8; k++) { start[k] = start_px[k]; key[k] = s.key_px[k]; }
    const kf::State keep = s;
    const MapState mkeep = m;
    int flags = 0, links = 0;
    double overlap = 0.0;
    if (cand < 0) {
        flags = RV_NO_CANDIDATE;
        grid = 0;
        cand = -1;
    } else {
        links = entry->links;
        overlap = (double)rec.px.n_valid / kf::FRAME_PIXELS;
        bool rec_finite = true;
        double worst = 0.0;
        for (int k = 0; k < 8; k++) {
            rec_finite = rec_finite && std::isfinite(rec.px.offsets_px[k]);
            const double d = std::fabs((double)rec.px.offsets_px[k] - (double)start[k]);
            worst = d > worst ? d : worst;
        }
        if (rec.px.flags & (pa::SINGULAR | pa::DEGENERATE | pa::FEW_PIXELS)) flags = RV_STOPPED;
        else if (o.max_mse > 0.0 && !(rec.px.mse <= o.max_mse)) flags = RV_MSE_ABOVE_MAX;
        else if (!rec_finite) flags = RV_NON_FINITE;
        else if (overlap < o.min_overlap) flags = RV_LOW_OVERLAP;
        else if (o.max_closure_px > 0.0 && !(worst <= o.max_closure_px)) flags = RV_CLOSURE_ABOVE_MAX;
        else if (!kf::homography(rec.px.offsets_px, hx) || !kf::chain(hx, entry->h_origin_key, hc)) flags = RV_CHAIN;
        else flags = RV_ATTACHED;
    }
    const bool attach = flags == RV_ATTACHED;
    ns = keep;
    nm = mkeep;
    for (int k = 0; k < 8; k++) out.closure_px[k] = 0.0;
    if (attach) {
        for (int k = 0; k < 8; k++) key[k] = rec.px.offsets_px[k];
        for (int k = 0; k < 8; k++) ns.key_px[k] = key[k];
        for (int k = 0; k < 9; k++) ns.h_origin_key[k] = entry->h_origin_key[k];
        ns.age = 0;
        nm.cur_slot = cand;
        nm.cur_links = links;
        corners(hb, cb);
        corners(hc, ca);
        for (int k = 0; k < 8; k++) out.closure_px[k] = ca[k] - cb[k];
    } else {
        for (int k = 0; k < 9; k++) hc[k] = hb[k];
    }
    for (int k = 0; k < 8; k++) { out.start_px[k] = start[k]; out.key_px[k] = key[k]; }
    for (int k = 0; k < 9; k++) { out.h_origin_before[k] = hb[k]; out.h_origin_curr[k] = hc[k]; }
    out.overlap = overlap;
    out.slot = cand; out.links = links; out.grid = grid; out.flags = flags; out.pad[0] = 0; out.pad[1] = 0;
    return attach ? 1 : 0;
}

}  /* namespace hnet_keyframe_map */

#endif /* HNET_KEYFRAME_MAP_H */
