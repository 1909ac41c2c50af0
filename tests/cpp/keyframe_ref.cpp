// keyframe_ref.cpp — the host reference of tracking against a held keyframe (include/hnet.h hnet_sessions_keyframe_track): compose and decide
// of include/hnet_keyframe.h, the very functions the device compiles, around photo_robust_ref.cpp's alignment; one session's whole track on the host.
// Built as that file is built (nothing may be contracted):
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -D__HIP_PLATFORM_AMD__ -I <rocm>/include -I cuahn_vio_amd/csrc -I include tests/cpp/keyframe_ref.cpp
#include "photo_robust_ref.cpp"

#include "hnet_keyframe.h"

namespace kf = hnet_keyframe;

static_assert(sizeof(kf::State) == 120 && sizeof(kf::Track) == 1720 && sizeof(kf::Opts) == 88, "the layouts of include/hnet.h and csrc/keyframe_dev.h");

extern "C" {

// 1 and out [8] written, or 0 and nothing written
int keyframe_ref_compose(const float* step_px, const float* key_px, float* out_px) { return kf::compose(step_px, key_px, out_px) ? 1 : 0; }

// H(x) [9]; returns whether every entry is finite
int keyframe_ref_homography(const float* x, double* h) { return kf::homography(x, h) ? 1 : 0; }

// the whole output record (rec copied, or zeros for a session without a keyframe) and the new state; returns the copy flag
int keyframe_ref_decide(const void* state, const float* start_px, const void* rec, const void* opts, int gap, void* new_state, void* out) {
    const kf::State& s = *static_cast<const kf::State*>(state);
    kf::Track& o = *static_cast<kf::Track*>(out);
    if (s.has_key) memcpy(&o.rec, rec, sizeof o.rec);
    else memset(&o.rec, 0, sizeof o.rec);
    return kf::decide(s, start_px, *static_cast<const hnet_robust::Record*>(rec), *static_cast<const kf::Opts*>(opts), gap != 0, *static_cast<kf::State*>(new_state), o);
}

// one track of one session: state and keyframe [71 680] are read and updated, curr is the session's current frame, step_px null = no motion
void keyframe_ref_track(void* state, uint8_t* keyframe, const uint8_t* curr, const float* step_px, const void* opts, int gap, void* out) {
    kf::State& s = *static_cast<kf::State*>(state);
    const kf::Opts& o = *static_cast<const kf::Opts*>(opts);
    kf::Track& t = *static_cast<kf::Track*>(out);
    hnet_robust::Record recs[hnet_align::MAX_LEVELS];
    float start[8];
    memset(&t.rec, 0, sizeof t.rec);
    memset(recs, 0, sizeof recs);
    for (int k = 0; k < 8; k++) start[k] = kf::quiet_nan();
    if (s.has_key) {
        const float zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        kf::compose(step_px ? step_px : zero, s.key_px, start);
        photo_robust_ref::align(keyframe, curr, start, o.align, o.levels, recs);
        t.rec = recs[0];
    }
    if (kf::decide(s, start, recs[0], o, gap != 0, s, t)) memcpy(keyframe, curr, photo_ref::NPIX);
}

void keyframe_ref_default_opts(void* opts) { kf::default_opts(*static_cast<kf::Opts*>(opts)); }
int keyframe_ref_opts_valid(const void* opts) { return kf::opts_valid(*static_cast<const kf::Opts*>(opts)) ? 1 : 0; }

}  // extern "C"
