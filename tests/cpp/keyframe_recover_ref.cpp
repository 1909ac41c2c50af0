// keyframe_recover_ref.cpp — the host reference of recovering a lost camera inside the track (include/hnet.h hnet_sessions_keyframe_track_recover;
// DESIGN 7u): decide_deferred, finish and the zero record of include/hnet_keyframe_recover.h, the very functions the device compiles, around
// keyframe_ref.cpp's start, keyframe_map_ref.cpp's note and photo_search_oriented_ref.cpp's relocalise; one session's whole call on the host, in the
// order of the device's launches.  Built as photo_search_oriented_ref.cpp is built (nothing may be contracted):
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -D__HIP_PLATFORM_AMD__ -I <rocm>/include -I cuahn_vio_amd/csrc -I include tests/cpp/keyframe_recover_ref.cpp
#include "photo_search_oriented_ref.cpp"

#include "hnet_keyframe_recover.h"

namespace kr = hnet_keyframe_recovery;

static_assert(sizeof(kr::Opts) == 208 && sizeof(kr::Reloc) == sizeof(photo_search_oriented_ref::Reloc) && sizeof(kr::Record) == 1720 + 2040 &&
              offsetof(kr::Record, reloc) == 1720 && sizeof(kr::Stash) == 280 && kr::RECOVERED == 2048, "the layouts of include/hnet.h");

namespace keyframe_recover_ref {

// one call for one session.  capacity 0: no map.  given_track / given_reloc: level-0 alignment records to decide on instead of the host alignment's.
// Returns 0: not lost, 1: lost and recovered, 2: lost and unrecovered.
inline int track(kf::State& s, uint8_t* keyframe, km::MapState* m, km::Entry* e, uint8_t* images, int capacity, const uint8_t* curr, const float* step_px,
                 const kr::Opts& o, const po::Hyp* hyps, int n_hyp, bool gap, const hnet_robust::Record* given_track, const hnet_robust::Record* given_reloc,
                 kr::Record& out) {
    hnet_robust::Record recs[hnet_align::MAX_LEVELS];
    float start[8];
    memset(&out, 0, sizeof out);
    memset(recs, 0, sizeof recs);
    for (int k = 0; k < 8; k++) start[k] = kf::quiet_nan();
    if (s.has_key) {
        const float zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        kf::compose(step_px ? step_px : zero, s.key_px, start);
        if (given_track) recs[0] = *given_track;
        else photo_robust_ref::align(keyframe, curr, start, o.track.align, o.track.levels, recs);
        out.track.rec = recs[0];
    }
    kr::Stash stash;
    int active = 0;
    const int copy = kr::decide_deferred(s, start, recs[0], o.track, gap, s, out.track, stash, active);
    if (copy) memcpy(keyframe, curr, photo_ref::NPIX);
    if (capacity > 0) {
        const int slot = km::note(out.track.flags, copy, s, *m, e, capacity);
        if (slot >= 0) memcpy(images + (size_t)slot * photo_ref::NPIX, curr, photo_ref::NPIX);
    }
    if (!active) {
        kr::zero_reloc(out.reloc);
        return 0;
    }
    photo_search_oriented_ref::Reloc rl_out;
    photo_search_oriented_ref::relocalise(s, keyframe, m, e, images, capacity, curr, o.reloc, hyps, n_hyp, given_reloc, rl_out);
    memcpy(&out.reloc, &rl_out, sizeof rl_out);
    const int copy2 = kr::finish(rl_out.rv.flags, stash, s, out.track);
    if (kr::recovered_by(rl_out.rv.flags)) return 1;
    if (copy2) memcpy(keyframe, curr, photo_ref::NPIX);
    if (capacity > 0) {
        const int slot = km::note(out.track.flags, copy2, s, *m, e, capacity);
        if (slot >= 0) memcpy(images + (size_t)slot * photo_ref::NPIX, curr, photo_ref::NPIX);
    }
    return 2;
}

}  // namespace keyframe_recover_ref

extern "C" {

void keyframe_recover_ref_default_opts(void* opts) { kr::default_opts(*static_cast<kr::Opts*>(opts)); }
int keyframe_recover_ref_lost_of(int flags) { return kr::lost_of(flags); }

// the deferred decision: the output record (rec copied, or zeros for a session without a keyframe), the new state, the stash and *active; returns the copy flag
int keyframe_recover_ref_decide(const void* state, const float* start_px, const void* rec, const void* opts, int gap, void* new_state, void* out, void* stash,
                                int* active) {
    const kf::State& s = *static_cast<const kf::State*>(state);
    kf::Track& o = *static_cast<kf::Track*>(out);
    if (s.has_key) memcpy(&o.rec, rec, sizeof o.rec);
    else memset(&o.rec, 0, sizeof o.rec);
    return kr::decide_deferred(s, start_px, *static_cast<const hnet_robust::Record*>(rec), *static_cast<const kf::Opts*>(opts), gap != 0,
                               *static_cast<kf::State*>(new_state), o, *static_cast<kr::Stash*>(stash), *active);
}

// state and track are updated in place; returns the second commit's copy flag
int keyframe_recover_ref_finish(int reloc_flags, const void* stash, void* state, void* track) {
    return kr::finish(reloc_flags, *static_cast<const kr::Stash*>(stash), *static_cast<kf::State*>(state), *static_cast<kf::Track*>(track));
}

void keyframe_recover_ref_zero_reloc(void* out) { kr::zero_reloc(*static_cast<kr::Reloc*>(out)); }

// one call of one session (keyframe_recover_ref::track); map_state / entries / images may be null with capacity 0; the given records may be null
int keyframe_recover_ref_track(void* state, uint8_t* keyframe, void* map_state, void* entries, uint8_t* images, int capacity, const uint8_t* curr,
                               const float* step_px, const void* opts, const void* hyps, int n_hyp, int gap, const void* given_track, const void* given_reloc,
                               void* out) {
    return keyframe_recover_ref::track(*static_cast<kf::State*>(state), keyframe, static_cast<km::MapState*>(map_state), static_cast<km::Entry*>(entries), images,
                                       capacity, curr, step_px, *static_cast<const kr::Opts*>(opts), static_cast<const po::Hyp*>(hyps), n_hyp, gap != 0,
                                       static_cast<const hnet_robust::Record*>(given_track), static_cast<const hnet_robust::Record*>(given_reloc),
                                       *static_cast<kr::Record*>(out));
}

}  // extern "C"
