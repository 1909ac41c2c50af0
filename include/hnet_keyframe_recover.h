/* hnet_keyframe_recover.h — recovering a lost camera INSIDE the track (include/hnet.h hnet_sessions_keyframe_track_recover): the deferred form
 * of the track's decision that lets the oriented relocalisation run between a LOST verdict and its re-key.  What the device
 * (csrc/kernels_keyframe_recover.hip) and the host reference (tests/cpp/keyframe_recover_ref.cpp) both compile, on top of include/hnet_keyframe.h (decide,
 * exactly as it is), include/hnet_keyframe_reloc.h and include/hnet_photo_search_oriented.h (the record of the search).  None of them is edited.
 *
 * The rule, per session.  T1 = decide(state, start, rec, opts) and T0 = decide(state, start, rec, opts with auto_rekey = 0), both from the ORIGINAL state.
 *   lost_of(flags): the LOST reason bits of a track record's flags.
 *   decide_deferred: not LOST (FIRST included): the new state, the record and the copy flag are T1's, active = 0 and the stash is zero.  LOST: the new
 *     state, the record and the copy flag (always 0) are T0's - the keyframe stays, key_px is the bridge, the age grows - active = 1, and T1 is kept aside
 *     in the stash: its state, the record's fields behind `rec` (rec itself is the same in both) and its copy flag.
 *   The oriented relocalisation then runs on T0's state, exactly as it is, for the active sessions.
 *   finish(outcome = the relocalise's rv.flags): RL_RETRACKED or RL_ATTACHED: the state is what the relocalise left, the record is T0's with RECOVERED
 *     or-ed into its flags; returns 0.  Anything else (RL_NO_CANDIDATE, a REJECTED reason): state and record become T1's from the stash; returns T1's copy
 *     flag, on which the caller copies the current frame over the keyframe and runs the map's note a second time.
 *   zero_reloc: the relocalise record of a session that needed no recovery: all zero except target = -2.
 * Choices the rule left open.  The map's note runs on T0's flags before the search (an ORIGIN_RESTARTED invalidates the entries before they are
 *   searched) and again on T1's flags for the unrecovered sessions; T1's flags hold ORIGIN_RESTARTED exactly when T0's do and the invalidation is
 *   idempotent, so the two notes leave the map as one note of T1 would.  No re-key is judged on a recovered frame: LOW_OVERLAP and MAX_AGE are the next
 *   track's.  A recovered record keeps rec, start_px and the bridge in key_px: it shows why the frame was lost; the session's key_px is the relocalise's.
 * Every body is non-contracting, everything is in double, nothing depends on the batch.
 */
#ifndef HNET_KEYFRAME_RECOVER_H
#define HNET_KEYFRAME_RECOVER_H

#include <cstddef>

#include "hnet_keyframe_reloc.h"
#include "hnet_photo_search_oriented.h"

namespace hnet_keyframe_recovery {

namespace kf = hnet_keyframe;
namespace km = hnet_keyframe_map;
namespace rl = hnet_keyframe_reloc;
namespace po = hnet_search_oriented;
namespace pa = hnet_align;
namespace pr = hnet_robust;

/* the flag this layer adds to a track record (= HNET_KF_RECOVERED) */
enum { RECOVERED = 2048 };
static_assert((RECOVERED & (kf::LOST | kf::ORIGIN_RESTARTED | kf::FIRST | kf::REKEYED | kf::BRIDGED | kf::GAP | kf::LOW_OVERLAP | kf::MAX_AGE)) == 0,
              "RECOVERED is a bit of its own");

/* = hnet_keyframe_recover_opts */
struct Opts { kf::Opts track; rl::Opts reloc; };
inline void default_opts(Opts& o) {
    kf::default_opts(o.track);         /* max_mse stays 0: the caller chooses it */
    rl::default_opts(o.reloc);
}

/* = hnet_keyframe_relocalise_oriented */
struct Reloc {
    km::Revisit rv;
    po::Record search;
    int32_t target, n_searched, n_found, pad;
};
/* = hnet_keyframe_recover */
struct Record { kf::Track track; Reloc reloc; };

/* T1 of a lost session, kept aside while the relocalisation runs: the state, the record's fields behind rec, the copy flag */
struct Stash {
    kf::State state;
    float start_px[pa::NX], key_px[pa::NX];
    double h_origin_curr[9], overlap;
    int32_t age, keyframes, flags, copy;
};

inline int lost_of(int track_flags) { return track_flags & kf::LOST; }

inline void stash_zero(Stash& st) {
    st.state.has_key = 0; st.state.age = 0; st.state.keyframes = 0; st.state.pad = 0;
    for (int k = 0; k < 8; k++) { st.state.key_px[k] = 0.0f; st.start_px[k] = 0.0f; st.key_px[k] = 0.0f; }
    for (int k = 0; k < 9; k++) { st.state.h_origin_key[k] = 0.0; st.h_origin_curr[k] = 0.0; }
    st.overlap = 0.0;
    st.age = 0; st.keyframes = 0; st.flags = 0; st.copy = 0;
}

/* the fields of a track record behind rec, to and from a stash */
inline void stash_fields(const kf::Track& t, Stash& st) {
    for (int k = 0; k < 8; k++) { st.start_px[k] = t.start_px[k]; st.key_px[k] = t.key_px[k]; }
    for (int k = 0; k < 9; k++) st.h_origin_curr[k] = t.h_origin_curr[k];
    st.overlap = t.overlap;
    st.age = t.age; st.keyframes = t.keyframes; st.flags = t.flags;
}
inline void unstash_fields(const Stash& st, kf::Track& t) {
    for (int k = 0; k < 8; k++) { t.start_px[k] = st.start_px[k]; t.key_px[k] = st.key_px[k]; }
    for (int k = 0; k < 9; k++) t.h_origin_curr[k] = st.h_origin_curr[k];
    t.overlap = st.overlap;
    t.age = st.age; t.keyframes = st.keyframes; t.flags = st.flags; t.pad = 0;
}

/* s and ns may be the same object; start_px must not be a field of out.  Returns the copy flag of what is committed now; out.rec is the caller's, as in
 * hnet_keyframe::decide.  Every byte of the stash and of out behind rec is written. */
inline int decide_deferred(const kf::State& s, const float* start_px, const pr::Record& rec, const kf::Opts& o, bool gap, kf::State& ns, kf::Track& out,
                           Stash& stash, int& active) {
    const kf::State keep = s;
    kf::State s1;
    const int copy1 = kf::decide(keep, start_px, rec, o, gap, s1, out);
    if (!lost_of(out.flags)) {
        ns = s1;
        stash_zero(stash);
        active = 0;
        return copy1;
    }
    stash.state = s1;
    stash_fields(out, stash);
    stash.copy = copy1;
    kf::Opts o0 = o;
    o0.auto_rekey = 0;
    active = 1;
    return kf::decide(keep, start_px, rec, o0, gap, ns, out);
}

inline bool recovered_by(int reloc_flags) { return (reloc_flags & (rl::RL_RETRACKED | rl::RL_ATTACHED)) != 0; }

/* after the relocalisation of an active session: `state` is what it left and `out` is T0's record.  Returns the copy flag of the second commit. */
inline int finish(int reloc_flags, const Stash& stash, kf::State& state, kf::Track& out) {
    if (recovered_by(reloc_flags)) {
        out.flags |= RECOVERED;
        return 0;
    }
    state = stash.state;
    unstash_fields(stash, out);
    return stash.copy;
}

/* the zero record as 32-bit words (the device writes it a word per lane) */
constexpr int RELOC_WORDS = (int)(sizeof(Reloc) / 4), RELOC_TARGET_WORD = (int)(offsetof(Reloc, target) / 4);
static_assert(sizeof(Reloc) % 4 == 0 && offsetof(Reloc, target) % 4 == 0, "the relocalise record is whole words");
inline uint32_t zero_reloc_word(int i) { return i == RELOC_TARGET_WORD ? (uint32_t)rl::TARGET_NONE : 0u; }
inline void zero_reloc(Reloc& r) {
    uint32_t w[RELOC_WORDS];
    for (int i = 0; i < RELOC_WORDS; i++) w[i] = zero_reloc_word(i);
    std::memcpy(&r, w, sizeof r);
}

}  /* namespace hnet_keyframe_recovery */

#endif /* HNET_KEYFRAME_RECOVER_H */
