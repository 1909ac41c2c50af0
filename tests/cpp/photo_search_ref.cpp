// photo_search_ref.cpp — the host reference of the coarse search over integer translations and of the relocalisation (include/hnet.h
// hnet_op_photo_search, hnet_sessions_keyframe_relocalise): thumbnail, shift_sums, shift_score, the pick and finish of
// include/hnet_photo_search.h with pixels in ascending order, and offer and decide_relocalise of include/hnet_keyframe_reloc.h, the very functions the
// device compiles, around keyframe_map_ref.cpp's decide_revisit and photo_robust_ref.cpp's alignment; one session's whole relocalise on the host.
// Built as keyframe_map_ref.cpp is built (nothing may be contracted):
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -D__HIP_PLATFORM_AMD__ -I <rocm>/include -I cuahn_vio_amd/csrc -I include tests/cpp/photo_search_ref.cpp
#include "keyframe_map_ref.cpp"

#include "hnet_keyframe_reloc.h"

namespace ps = hnet_search;
namespace rl = hnet_keyframe_reloc;

static_assert(sizeof(ps::Opts) == 32 && sizeof(ps::Record) == 96 && sizeof(rl::Opts) == 120 && sizeof(rl::Reloc) == 1976,
              "the layouts of include/hnet.h and csrc/photo_search_dev.h");

namespace photo_search_ref {

// one session's relocalise: curr is the frame its last track saw; capacity 0 = no map (map_state, entries and images are not read).  given != nullptr:
// the level-0 record of the alignment is taken from there instead of being computed (the device's record under the host's rule).  Returns the attach flag;
// on an attach the candidate's image becomes the keyframe.
inline int relocalise(kf::State& s, uint8_t* keyframe, km::MapState* m, const km::Entry* e, const uint8_t* images, int capacity, const uint8_t* curr,
                      const rl::Opts& o, const hnet_robust::Record* given, rl::Reloc& out) {
    uint8_t tc[ps::TPIX], tk[ps::TPIX];
    std::vector<double> scores(ps::NSHIFT);
    ps::Record srec[rl::MAX_CANDIDATES];
    hnet_robust::Record recs[hnet_align::MAX_LEVELS];
    double hb[9];
    float start[8];
    rl::Pick p;
    rl::pick_none(p);
    memset(recs, 0, sizeof recs);
    memset(&out, 0, sizeof out);
    for (int k = 0; k < 9; k++) hb[k] = (k & 3) == 0 ? 1.0 : 0.0;
    for (int k = 0; k < 8; k++) start[k] = kf::quiet_nan();
    ps::thumbnail(curr, tc);
    if (s.has_key) {
        km::origin_curr(s, hb);
        for (int c = 0; c <= capacity; c++) {
            const uint8_t* src = keyframe;
            if (c >= 1) {
                if (!e[c - 1].valid || c - 1 == m->cur_slot) continue;
                src = images + (size_t)(c - 1) * photo_ref::NPIX;
            }
            ps::thumbnail(src, tk);
            ps::search(tk, tc, o.search, srec[c], scores.data());
            out.n_searched++;
            out.n_found += srec[c].flags == ps::FOUND ? 1 : 0;
            rl::offer(p, c, srec[c]);
        }
    }
    out.target = rl::target_of(p.index);
    const uint8_t* cand = nullptr;
    if (p.index >= 0) {
        out.search = srec[p.index];
        memcpy(start, srec[p.index].start_px, sizeof start);
        cand = p.index == 0 ? keyframe : images + (size_t)(p.index - 1) * photo_ref::NPIX;
        if (given) recs[0] = *given;
        else photo_robust_ref::align(cand, curr, start, o.align, o.levels, recs);
        out.rv.rec = recs[0];
    }
    if (p.index == 0) {
        rl::decide_relocalise(s, start, hb, recs[0], o, s, out.rv);
        return 0;
    }
    km::Opts mo;
    rl::revisit_opts(o, mo);
    km::MapState none = {-1, 0, 0, 0};
    km::MapState& ms = capacity > 0 ? *m : none;
    const int attach = km::decide_revisit(s, ms, p.index >= 1 ? e + (p.index - 1) : nullptr, p.index - 1, 0, start, hb, recs[0], mo, s, ms, out.rv);
    if (attach) memcpy(keyframe, cand, photo_ref::NPIX);
    return attach;
}

}  // namespace photo_search_ref

extern "C" {

void photo_search_ref_default_opts(void* opts) { ps::default_opts(*static_cast<ps::Opts*>(opts)); }
int photo_search_ref_opts_valid(const void* opts) { return ps::opts_valid(*static_cast<const ps::Opts*>(opts)) ? 1 : 0; }

// the thumbnail [1120] of a frame [71 680]
void photo_search_ref_thumbnail(const uint8_t* img, uint8_t* out) { ps::thumbnail(img, out); }

// the sums {n, sa, sb, sab, saa, sbb} of one shift of two thumbnails; returns whether it is scored, *score written then
int photo_search_ref_shift(const uint8_t* a, const uint8_t* b, int dx, int dy, int min_overlap, int32_t* sums, double* score) {
    ps::Sums s;
    ps::shift_sums(a, b, dx, dy, s);
    memcpy(sums, &s, sizeof s);
    return ps::shift_score(s, min_overlap, *score) ? 1 : 0;
}

int photo_search_ref_better(double si, int i, double sj, int j) { return ps::better(si, i, sj, j) ? 1 : 0; }

// the search of two thumbnails: record (every byte) and score table [2501]
void photo_search_ref_search(const uint8_t* a, const uint8_t* b, const void* opts, void* rec, double* scores) {
    ps::search(a, b, *static_cast<const ps::Opts*>(opts), *static_cast<ps::Record*>(rec), scores);
}

// hnet_op_photo_search on the host: frames [n][71 680] -> records [n], score tables [n][2501] (scores may be null)
void photo_search_ref_run(const uint8_t* img1, const uint8_t* img2, int n, const void* opts, void* out, double* scores) {
    std::vector<double> tmp(ps::NSHIFT);
    uint8_t a[ps::TPIX], b[ps::TPIX];
    for (int i = 0; i < n; i++) {
        ps::thumbnail(img1 + (size_t)i * photo_ref::NPIX, a);
        ps::thumbnail(img2 + (size_t)i * photo_ref::NPIX, b);
        ps::search(a, b, *static_cast<const ps::Opts*>(opts), static_cast<ps::Record*>(out)[i], scores ? scores + (size_t)i * ps::NSHIFT : tmp.data());
    }
}

void photo_search_ref_reloc_default_opts(void* opts) { rl::default_opts(*static_cast<rl::Opts*>(opts)); }
int photo_search_ref_reloc_opts_valid(const void* opts) { return rl::opts_valid(*static_cast<const rl::Opts*>(opts)) ? 1 : 0; }

// the pick over count search records (valid [count]: whether the candidate exists) -> the index or -1
int photo_search_ref_pick(const void* recs, const int32_t* valid, int count) {
    rl::Pick p;
    rl::pick_none(p);
    for (int c = 0; c < count; c++)
        if (valid[c]) rl::offer(p, c, static_cast<const ps::Record*>(recs)[c]);
    return p.index;
}

// decide_relocalise: the revisit-shaped record (rec copied) and the new state
void photo_search_ref_decide(const void* state, const float* start_px, const double* h_before, const void* rec, const void* opts, void* new_state, void* out) {
    km::Revisit& o = *static_cast<km::Revisit*>(out);
    memcpy(&o.rec, rec, sizeof o.rec);
    rl::decide_relocalise(*static_cast<const kf::State*>(state), start_px, h_before, *static_cast<const hnet_robust::Record*>(rec),
                          *static_cast<const rl::Opts*>(opts), *static_cast<kf::State*>(new_state), o);
}

// one relocalise of one session (photo_search_ref::relocalise); given_rec may be null
int photo_search_ref_relocalise(void* state, uint8_t* keyframe, void* map_state, const void* entries, const uint8_t* images, int capacity, const uint8_t* curr,
                                const void* opts, const void* given_rec, void* out) {
    return photo_search_ref::relocalise(*static_cast<kf::State*>(state), keyframe, static_cast<km::MapState*>(map_state), static_cast<const km::Entry*>(entries), images,
                                        capacity, curr, *static_cast<const rl::Opts*>(opts), static_cast<const hnet_robust::Record*>(given_rec),
                                        *static_cast<rl::Reloc*>(out));
}

}  // extern "C"
