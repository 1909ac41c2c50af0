// photo_search_oriented_ref.cpp — the host reference of the coarse search under a table of orientation hypotheses and of the relocalisation on top of it
// (include/hnet.h hnet_op_photo_search_oriented, hnet_sessions_keyframe_relocalise_oriented): make_hyp, warp_template, the masked shift_sums,
// the winner over the table and finish of include/hnet_photo_search_oriented.h, the very functions the device compiles, around photo_search_ref.cpp's
// pick, decide_relocalise and decide_revisit and photo_robust_ref.cpp's alignment; one session's whole oriented relocalise on the host.
// Built as photo_search_ref.cpp is built (nothing may be contracted):
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -D__HIP_PLATFORM_AMD__ -I <rocm>/include -I cuahn_vio_amd/csrc -I include tests/cpp/photo_search_oriented_ref.cpp
#include "photo_search_ref.cpp"

#include "hnet_photo_search_oriented.h"

namespace po = hnet_search_oriented;

namespace photo_search_oriented_ref {

// = hnet_keyframe_relocalise_oriented
struct Reloc {
    km::Revisit rv;
    po::Record search;
    int32_t target, n_searched, n_found, pad;
};
static_assert(sizeof(po::Hyp) == 48 && sizeof(po::Record) == 160 && sizeof(Reloc) == sizeof(rl::Reloc) + 64, "the layouts of include/hnet.h");

// photo_search_ref::relocalise with the oriented search over the same candidates
inline int relocalise(kf::State& s, uint8_t* keyframe, km::MapState* m, const km::Entry* e, const uint8_t* images, int capacity, const uint8_t* curr,
                      const rl::Opts& o, const po::Hyp* hyps, int n_hyp, const hnet_robust::Record* given, Reloc& out) {
    uint8_t tc[ps::TPIX], tk[ps::TPIX];
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
            out.n_searched++;
            out.n_found += srec[c].base.flags == ps::FOUND ? 1 : 0;
            rl::offer(p, c, srec[c].base);
        }
    }
    out.target = rl::target_of(p.index);
    const uint8_t* cand = nullptr;
    if (p.index >= 0) {
        out.search = srec[p.index];
        memcpy(start, srec[p.index].base.start_px, sizeof start);
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

}  // namespace photo_search_oriented_ref

extern "C" {

int photo_search_oriented_ref_make_hyp(double angle_rad, double scale, void* hyp) { return po::make_hyp(angle_rad, scale, *static_cast<po::Hyp*>(hyp)) ? 1 : 0; }
int photo_search_oriented_ref_yaw_table(double first_deg, double step_deg, int count, void* hyps) {
    return po::yaw_table(first_deg, step_deg, count, static_cast<po::Hyp*>(hyps)) ? 1 : 0;
}
int photo_search_oriented_ref_table_valid(const void* hyps, int n_hyp) { return po::table_valid(static_cast<const po::Hyp*>(hyps), n_hyp) ? 1 : 0; }

// the warped template [1120] and its mask [1120] of a thumbnail [1120] under b [4]
void photo_search_oriented_ref_warp(const uint8_t* t, const int32_t* b, uint8_t* w, uint8_t* m) { po::warp_template(t, b, w, m); }

// the masked sums {n, sa, sb, sab, saa, sbb} of one shift; returns whether it is scored, *score written then
int photo_search_oriented_ref_shift(const uint8_t* a, const uint8_t* m, const uint8_t* b, int dx, int dy, int min_overlap, int32_t* sums, double* score) {
    ps::Sums s;
    po::shift_sums(a, m, b, dx, dy, s);
    memcpy(sums, &s, sizeof s);
    return ps::shift_score(s, min_overlap, *score) ? 1 : 0;
}

// the oriented search of two thumbnails: record (every byte), score tables [n_hyp][2501] and the entries' records [n_hyp] (either may be null)
void photo_search_oriented_ref_search(const uint8_t* a, const uint8_t* b, const void* opts, const void* hyps, int n_hyp, void* rec, double* scores, void* per_hyp) {
    po::search(a, b, *static_cast<const ps::Opts*>(opts), static_cast<const po::Hyp*>(hyps), n_hyp, *static_cast<po::Record*>(rec), scores,
               static_cast<ps::Record*>(per_hyp));
}

// hnet_op_photo_search_oriented on the host: frames [n][71 680] -> records [n], score tables [n][n_hyp][2501] (scores may be null)
void photo_search_oriented_ref_run(const uint8_t* img1, const uint8_t* img2, int n, const void* opts, const void* hyps, int n_hyp, void* out, double* scores) {
    uint8_t a[ps::TPIX], b[ps::TPIX];
    for (int i = 0; i < n; i++) {
        ps::thumbnail(img1 + (size_t)i * photo_ref::NPIX, a);
        ps::thumbnail(img2 + (size_t)i * photo_ref::NPIX, b);
        po::search(a, b, *static_cast<const ps::Opts*>(opts), static_cast<const po::Hyp*>(hyps), n_hyp, static_cast<po::Record*>(out)[i],
                   scores ? scores + (size_t)i * n_hyp * ps::NSHIFT : nullptr, nullptr);
    }
}

// one oriented relocalise of one session (photo_search_oriented_ref::relocalise); given_rec may be null
int photo_search_oriented_ref_relocalise(void* state, uint8_t* keyframe, void* map_state, const void* entries, const uint8_t* images, int capacity,
                                         const uint8_t* curr, const void* opts, const void* hyps, int n_hyp, const void* given_rec, void* out) {
    return photo_search_oriented_ref::relocalise(*static_cast<kf::State*>(state), keyframe, static_cast<km::MapState*>(map_state),
                                                 static_cast<const km::Entry*>(entries), images, capacity, curr, *static_cast<const rl::Opts*>(opts),
                                                 static_cast<const po::Hyp*>(hyps), n_hyp, static_cast<const hnet_robust::Record*>(given_rec),
                                                 *static_cast<photo_search_oriented_ref::Reloc*>(out));
}

}  // extern "C"
