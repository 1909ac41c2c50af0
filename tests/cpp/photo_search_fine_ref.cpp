// photo_search_fine_ref.cpp — the host reference of the fine stage of the search and of the relocalisation on top of it (include/hnet.h
// hnet_op_photo_search_fine, hnet_sessions_keyframe_relocalise_fine): the level-2 thumbnail, the warp, the masked sums, the order and finish of
// include/hnet_photo_search_fine.h, the very functions the device compiles, around photo_search_oriented_ref.cpp's coarse search and relocalise.
// Built as photo_search_oriented_ref.cpp is built (nothing may be contracted):
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -D__HIP_PLATFORM_AMD__ -I <rocm>/include -I cuahn_vio_amd/csrc -I include tests/cpp/photo_search_fine_ref.cpp
#include "photo_search_oriented_ref.cpp"

#include "hnet_photo_search_fine.h"

namespace pf = hnet_search_fine;

namespace photo_search_fine_ref {

// = hnet_keyframe_relocalise_fine
struct Reloc {
    photo_search_oriented_ref::Reloc base;
    pf::Part fine;
};
static_assert(sizeof(pf::Record) == 288 && sizeof(Reloc) == sizeof(photo_search_oriented_ref::Reloc) + 128 && offsetof(Reloc, fine) % 8 == 0, "the layouts of include/hnet.h");

// the whole search of one pair of frames: the coarse stage, then the fine stage on the level-2 thumbnails; scores [n_hyp][2501] and fine_scores [n_fine][81]
// may be null
inline void search(const uint8_t* img1, const uint8_t* img2, const ps::Opts& o, const po::Hyp* hyps, int n_hyp, const pf::Opts& fo, const po::Hyp* fine,
                   pf::Record& r, double* scores, double* fine_scores) {
    uint8_t a[ps::TPIX], b[ps::TPIX], fa[pf::FPIX], fb[pf::FPIX];
    ps::thumbnail(img1, a);
    ps::thumbnail(img2, b);
    po::search(a, b, o, hyps, n_hyp, r.coarse, scores, nullptr);
    pf::thumbnail(img1, fa);
    pf::thumbnail(img2, fb);
    pf::refine(fa, fb, r.coarse, o.min_overlap, n_hyp, fo, fine, r.fine, fine_scores);
}

// photo_search_oriented_ref::relocalise with the fine stage on the picked candidate: the alignment starts from the fine part's final start
inline int relocalise(kf::State& s, uint8_t* keyframe, km::MapState* m, const km::Entry* e, const uint8_t* images, int capacity, const uint8_t* curr,
                      const rl::Opts& o, const po::Hyp* hyps, int n_hyp, const pf::Opts& fo, const po::Hyp* fine, const hnet_robust::Record* given, Reloc& out) {
    uint8_t tc[ps::TPIX], tk[ps::TPIX], fa[pf::FPIX], fb[pf::FPIX];
    po::Record srec[rl::MAX_CANDIDATES];
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
            po::search(tk, tc, o.search, hyps, n_hyp, srec[c], nullptr, nullptr);
            out.base.n_searched++;
            out.base.n_found += srec[c].base.flags == ps::FOUND ? 1 : 0;
            rl::offer(p, c, srec[c].base);
        }
    }
    out.base.target = rl::target_of(p.index);
    const uint8_t* cand = nullptr;
    {                                              // without a pick: SKIPPED on the all-zero search record
        pf::Best none;
        pf::best_none(none);
        const ps::Sums zero = {0, 0, 0, 0, 0, 0};
        pf::finish(out.base.search, nullptr, fo.n_fine, false, none, zero, fo, out.fine);
    }
    if (p.index >= 0) {
        out.base.search = srec[p.index];
        cand = p.index == 0 ? keyframe : images + (size_t)(p.index - 1) * photo_ref::NPIX;
        pf::thumbnail(cand, fa);
        pf::thumbnail(curr, fb);
        pf::refine(fa, fb, out.base.search, o.search.min_overlap, n_hyp, fo, fine, out.fine, nullptr);
        memcpy(start, out.fine.start_px, sizeof start);
        if (given) recs[0] = *given;
        else photo_robust_ref::align(cand, curr, start, o.align, o.levels, recs);
        out.base.rv.rec = recs[0];
    }
    if (p.index == 0) {
        rl::decide_relocalise(s, start, hb, recs[0], o, s, out.base.rv);
        return 0;
    }
    km::Opts mo;
    rl::revisit_opts(o, mo);
    km::MapState none = {-1, 0, 0, 0};
    km::MapState& ms = capacity > 0 ? *m : none;
    const int attach = km::decide_revisit(s, ms, p.index >= 1 ? e + (p.index - 1) : nullptr, p.index - 1, 0, start, hb, recs[0], mo, s, ms, out.base.rv);
    if (attach) memcpy(keyframe, cand, photo_ref::NPIX);
    return attach;
}

}  // namespace photo_search_fine_ref

extern "C" {

void photo_search_fine_ref_default_opts(void* o) { pf::default_opts(*static_cast<pf::Opts*>(o)); }
int photo_search_fine_ref_opts_valid(const void* o) { return pf::opts_valid(*static_cast<const pf::Opts*>(o)) ? 1 : 0; }
int photo_search_fine_ref_yaw_table(double first_deg, double step_deg, int count, int n_fine, void* out) {
    return pf::fine_yaw_table(first_deg, step_deg, count, n_fine, static_cast<po::Hyp*>(out)) ? 1 : 0;
}
int photo_search_fine_ref_table_valid(const void* fine, int n_hyp, int n_fine) { return pf::fine_table_valid(static_cast<const po::Hyp*>(fine), n_hyp, n_fine) ? 1 : 0; }

// the level-2 thumbnail [4480] of a frame [71 680]
void photo_search_fine_ref_thumb(const uint8_t* img, uint8_t* out) { pf::thumbnail(img, out); }
// the warped template [4480] and its mask [4480] of a level-2 thumbnail under b [4]
void photo_search_fine_ref_warp(const uint8_t* t, const int32_t* b, uint8_t* w, uint8_t* m) { pf::warp_template(t, b, w, m); }
// the masked sums {n, sa, sb, sab, saa, sbb} of one level-2 shift; returns whether it is scored under min_overlap (of level 2), *score written then
int photo_search_fine_ref_shift(const uint8_t* a, const uint8_t* m, const uint8_t* b, int sx, int sy, int min_overlap, int32_t* sums, double* score) {
    ps::Sums s;
    pf::shift_sums(a, m, b, sx, sy, s);
    memcpy(sums, &s, sizeof s);
    return ps::shift_score(s, min_overlap, *score) ? 1 : 0;
}
int photo_search_fine_ref_better(double si, int i, double sk, int k) { return pf::better(si, i, sk, k) ? 1 : 0; }

// the fine stage of two level-2 thumbnails after a coarse record (160 bytes): the fine part (128 bytes, every byte) and scores [n_fine][81] (may be null)
void photo_search_fine_ref_refine(const uint8_t* t, const uint8_t* b, const void* coarse, int min_overlap, int n_hyp, const void* fopts, const void* fine, void* part,
                                  double* scores) {
    pf::refine(t, b, *static_cast<const po::Record*>(coarse), min_overlap, n_hyp, *static_cast<const pf::Opts*>(fopts), static_cast<const po::Hyp*>(fine),
               *static_cast<pf::Part*>(part), scores);
}

// hnet_op_photo_search_fine on the host: frames [n][71 680] -> records [n] of 288 bytes, fine score tables [n][n_fine][81] (may be null)
void photo_search_fine_ref_run(const uint8_t* img1, const uint8_t* img2, int n, const void* opts, const void* hyps, int n_hyp, const void* fopts, const void* fine,
                               void* out, double* scores) {
    const pf::Opts& fo = *static_cast<const pf::Opts*>(fopts);
    for (int i = 0; i < n; i++)
        photo_search_fine_ref::search(img1 + (size_t)i * photo_ref::NPIX, img2 + (size_t)i * photo_ref::NPIX, *static_cast<const ps::Opts*>(opts),
                                      static_cast<const po::Hyp*>(hyps), n_hyp, fo, static_cast<const po::Hyp*>(fine), static_cast<pf::Record*>(out)[i], nullptr,
                                      scores ? scores + (size_t)i * fo.n_fine * pf::NSHIFT : nullptr);
}

// one fine relocalise of one session (photo_search_fine_ref::relocalise); given_rec may be null
int photo_search_fine_ref_relocalise(void* state, uint8_t* keyframe, void* map_state, const void* entries, const uint8_t* images, int capacity, const uint8_t* curr,
                                     const void* opts, const void* hyps, int n_hyp, const void* fopts, const void* fine, const void* given_rec, void* out) {
    return photo_search_fine_ref::relocalise(*static_cast<kf::State*>(state), keyframe, static_cast<km::MapState*>(map_state), static_cast<const km::Entry*>(entries),
                                             images, capacity, curr, *static_cast<const rl::Opts*>(opts), static_cast<const po::Hyp*>(hyps), n_hyp,
                                             *static_cast<const pf::Opts*>(fopts), static_cast<const po::Hyp*>(fine),
                                             static_cast<const hnet_robust::Record*>(given_rec), *static_cast<photo_search_fine_ref::Reloc*>(out));
}

}  // extern "C"
