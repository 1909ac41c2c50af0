// keyframe_map_ref.cpp — the host reference of the keyframe map and the revisit (include/hnet.h hnet_sessions_enable_keyframe_map,
// hnet_sessions_keyframe_revisit): note, relative, the grid count, select and decide_revisit of include/hnet_keyframe_map.h, the very functions
// the device compiles, around keyframe_ref.cpp's track and photo_robust_ref.cpp's alignment; one session's whole track-with-map and revisit on the host:
// its images, entries and states.  Built as keyframe_ref.cpp is built (nothing may be contracted):
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -D__HIP_PLATFORM_AMD__ -I <rocm>/include -I cuahn_vio_amd/csrc -I include tests/cpp/keyframe_map_ref.cpp
#include "keyframe_ref.cpp"

#include "hnet_keyframe_map.h"

namespace km = hnet_keyframe_map;

static_assert(sizeof(km::Entry) == 88 && sizeof(km::MapState) == 16 && sizeof(km::Revisit) == 1864 && sizeof(km::Opts) == 88,
              "the layouts of include/hnet.h and csrc/keyframe_map_dev.h");

extern "C" {

// the store slot or -1; map state and entries [capacity] are updated in place
int keyframe_map_ref_note(int track_flags, int copy, const void* new_state, void* map_state, void* entries, int capacity) {
    return km::note(track_flags, copy, *static_cast<const kf::State*>(new_state), *static_cast<km::MapState*>(map_state), static_cast<km::Entry*>(entries), capacity);
}

// h_origin_curr [9] of a state; returns whether the chain gave it
int keyframe_map_ref_origin_curr(const void* state, double* h) { return km::origin_curr(*static_cast<const kf::State*>(state), h) ? 1 : 0; }

// 1 and G [9], start_px [8] written, or 0
int keyframe_map_ref_relative(const double* h_origin_curr, const void* entry, double* G, float* start_px) {
    return km::relative(h_origin_curr, *static_cast<const km::Entry*>(entry), G, start_px) ? 1 : 0;
}

int keyframe_map_ref_grid_count(const double* G) { return km::grid_count(G); }

// the slot or -1; start_px [8] and the grid count written either way
int keyframe_map_ref_select(const void* map_state, const void* entries, int capacity, const double* h_origin_curr, int min_grid, float* start_px, int* grid) {
    km::Pick p;
    km::select(*static_cast<const km::MapState*>(map_state), static_cast<const km::Entry*>(entries), capacity, h_origin_curr, min_grid, p);
    memcpy(start_px, p.start_px, sizeof p.start_px);
    *grid = p.grid;
    return p.slot;
}

// the whole output record (rec copied, or zeros without a candidate) and the new states; returns the attach flag
int keyframe_map_ref_decide(const void* state, const void* map_state, const void* entries, int cand, int grid, const float* start_px, const double* h_before,
                            const void* rec, const void* opts, void* new_state, void* new_map_state, void* out) {
    km::Revisit& o = *static_cast<km::Revisit*>(out);
    if (cand >= 0) memcpy(&o.rec, rec, sizeof o.rec);
    else memset(&o.rec, 0, sizeof o.rec);
    return km::decide_revisit(*static_cast<const kf::State*>(state), *static_cast<const km::MapState*>(map_state),
                              cand >= 0 ? static_cast<const km::Entry*>(entries) + cand : nullptr, cand, grid, start_px, h_before,
                              *static_cast<const hnet_robust::Record*>(rec), *static_cast<const km::Opts*>(opts), *static_cast<kf::State*>(new_state),
                              *static_cast<km::MapState*>(new_map_state), o);
}

// one track of one session with a map: keyframe_ref_track, then note, then the new keyframe copied into images [capacity][71 680]
void keyframe_map_ref_track(void* state, uint8_t* keyframe, void* map_state, void* entries, uint8_t* images, int capacity, const uint8_t* curr,
                            const float* step_px, const void* opts, int gap, void* out) {
    kf::State& s = *static_cast<kf::State*>(state);
    keyframe_ref_track(state, keyframe, curr, step_px, opts, gap, out);
    const kf::Track& t = *static_cast<const kf::Track*>(out);
    const int copy = (t.flags & kf::REKEYED) ? 1 : 0;                      // (decide's copy flag: REKEYED is set exactly when curr became the keyframe)
    const int slot = km::note(t.flags, copy, s, *static_cast<km::MapState*>(map_state), static_cast<km::Entry*>(entries), capacity);
    if (slot >= 0) memcpy(images + (size_t)slot * photo_ref::NPIX, curr, photo_ref::NPIX);
}

// one revisit of one session: curr is the frame its last track saw.  Returns the attach flag; on an attach the candidate's image becomes the keyframe.
int keyframe_map_ref_revisit(void* state, uint8_t* keyframe, void* map_state, const void* entries, const uint8_t* images, int capacity, const uint8_t* curr,
                             const void* opts, void* out) {
    kf::State& s = *static_cast<kf::State*>(state);
    km::MapState& m = *static_cast<km::MapState*>(map_state);
    const km::Entry* e = static_cast<const km::Entry*>(entries);
    const km::Opts& o = *static_cast<const km::Opts*>(opts);
    km::Revisit& r = *static_cast<km::Revisit*>(out);
    hnet_robust::Record recs[hnet_align::MAX_LEVELS];
    double hb[9];
    km::Pick p;
    memset(recs, 0, sizeof recs);
    memset(&r.rec, 0, sizeof r.rec);
    if (s.has_key && km::origin_curr(s, hb)) km::select(m, e, capacity, hb, o.min_grid, p);
    else km::pick_none(p);
    if (p.slot >= 0) {
        photo_robust_ref::align(images + (size_t)p.slot * photo_ref::NPIX, curr, p.start_px, o.align, o.levels, recs);
        r.rec = recs[0];
    }
    const int attach = km::decide_revisit(s, m, p.slot >= 0 ? e + p.slot : nullptr, p.slot, p.grid, p.start_px, hb, recs[0], o, s, m, r);
    if (attach) memcpy(keyframe, images + (size_t)p.slot * photo_ref::NPIX, photo_ref::NPIX);
    return attach;
}

void keyframe_map_ref_default_opts(void* opts) { km::default_opts(*static_cast<km::Opts*>(opts)); }
int keyframe_map_ref_opts_valid(const void* opts) { return km::opts_valid(*static_cast<const km::Opts*>(opts)) ? 1 : 0; }

}  // extern "C"
