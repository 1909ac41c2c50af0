// filters_keyframe_recover_ref.cpp — the host reference of recovering a lost camera inside the in-step keyframe track of hnet_filters (include/hnet.h
// hnet_filters_set_keyframe_recover) as a small shared library for the tests: include/hnet_keyframe_measure_recover.h's usable_recover,
// next_prev_ok_recover, measure_recover and hnet_ekf::iterated_update_keyframe_recovered behind a C interface on the hnet.h structs, on top of
// keyframe_recover_ref.cpp (the host alignment, the map's note and the oriented relocalise).  The loop is fed as tests/cpp/filters_keyframe_ref.cpp feeds
// iterated_update_keyframe_measured, which stands next to it in the same build (the twin property of tests/test_filters_keyframe_recover_cpu.py).
// Built as keyframe_recover_ref.cpp is built (nothing may be contracted), with -I include.
#include "keyframe_recover_ref.cpp"

#include "hnet.h"
#include "hnet_keyframe_measure_recover.h"

#include <vector>

using hnet_ekf::Innovation;
using hnet_ekf::PhotoRecord;
using hnet_ekf::State;
namespace kfm = hnet_kfm;
namespace kfmr = hnet_kfmr;

static_assert(sizeof(hnet_filter_state) == sizeof(double) + sizeof(State), "hnet_filter_state = t + hnet_ekf::State");
static_assert(sizeof(hnet_photo_residual) == sizeof(PhotoRecord), "hnet_photo_residual = hnet_ekf::PhotoRecord");
static_assert(sizeof(hnet_keyframe_measure) == sizeof(kfm::Record) && sizeof(hnet_keyframe_measure_opts) == sizeof(kfm::Opts), "7v's layouts");
static_assert(sizeof(hnet_keyframe_measure_recover) == sizeof(kfmr::Record) && offsetof(hnet_keyframe_measure_recover, reloc) == offsetof(kfmr::Record, reloc) &&
              offsetof(hnet_keyframe_measure_recover, reloc) == 2448 && sizeof(hnet_keyframe_measure_recover) == 2448 + 2040,
              "hnet_keyframe_measure_recover = hnet_kfmr::Record");
static_assert((int)HNET_KFM_FROM_RELOC == kfmr::FROM_RELOC && (int)HNET_KFM_REATTACHED == kfmr::REATTACHED && (int)HNET_KFMR_UNUSABLE == kfmr::UNUSABLE &&
              (int)HNET_KFM_UNUSABLE == kfm::UNUSABLE, "the flags of include/hnet.h");
static_assert(sizeof(hnet_keyframe_relocalise_opts) == sizeof(rl::Opts) && sizeof(kfm::Session) == 128, "the options and the session the tests carry");

namespace {
State load(const hnet_filter_state& r) { State s; std::memcpy(&s, &r.p[0], sizeof s); return s; }
void save(const State& s, hnet_filter_state& r) { std::memcpy(&r.p[0], &s, sizeof s); }
void to_record(const Innovation& a, int it, hnet_innovation& o) {
    std::memcpy(o.r, a.r, sizeof o.r);
    std::memcpy(o.s_diag, a.s_diag, sizeof o.s_diag);
    o.nis = a.nis;
    o.iteration = it;
    o.flag = a.flag;
}
PhotoRecord from_c(const hnet_photo_residual& r) { return PhotoRecord{r.sum, r.sum_inside, r.n_inside, r.flags}; }
hnet_photo_residual to_c(const PhotoRecord& r) { return hnet_photo_residual{r.sum, r.sum_inside, r.n_inside, r.flags}; }

// the network surface, the scripted photometric callable and the aligner of filters_keyframe_ref.cpp
struct FakeNet {
    const float* net72;
    int gate;
    double t_frame;
    int img_counter;
    int calls = 0;
    int it = -1;
    const float* cur = nullptr;
    struct M { const float* v; double operator()(int i, int j) const { return v[i * 8 + j]; } };
    struct V { const float* v; double operator()(int i, int) const { return v[i]; } };
    template <class P> void network_inference(const P&, int iteration) {
        cur = net72 + (size_t)iteration * 72;
        it = iteration;
        calls++;
    }
    double get_latest_inference_time() const { return gate ? t_frame : t_frame - 1.0; }
    V get_pred_mean() const { return V{cur}; }
    M get_pred_Cov() const { return M{cur + 8}; }
};
struct ScriptedPhoto {
    const FakeNet* net;
    const hnet_photo_residual* script;
    PhotoRecord operator()(const double*) { return from_c(script[net->it < 0 ? 0 : 1 + net->it]); }
};
struct Aligner {
    const uint8_t *keyframe, *curr;
    const hnet_robust::Opts* align;
    int levels;
    const hnet_photo_robust* stub;
    int stub_accepted;
    int calls = 0;
    void operator()(const float* start, hnet_robust::Record& out, int& accepted) {
        calls++;
        if (!stub) {
            hnet_robust::Record recs[hnet_align::MAX_LEVELS];
            std::memset(recs, 0, sizeof recs);
            photo_robust_ref::align(keyframe, curr, start, *align, levels, recs);
            out = recs[0];
            accepted = 0;
            for (int l = 0; l < levels; l++) accepted += recs[l].px.accepted;
        } else {
            std::memcpy(&out, stub, sizeof out);
            accepted = stub_accepted;
        }
    }
};
// the relocaliser: the first commit of a lost session (the map's note on T0's flags; a lost session copies nothing), then the host oriented relocalise
// on the caller's keyframe and map.  The trials its alignment accepted are counted by running that alignment again from the searched start: a RETRACKED
// relocalise leaves the keyframe image as it was, and no other outcome reads the count.
struct Relocaliser {
    uint8_t* keyframe;
    km::MapState* m;
    km::Entry* e;
    uint8_t* images;
    int capacity;
    const uint8_t* curr;
    const rl::Opts* o;
    const po::Hyp* hyps;
    int n_hyp;
    const hnet_robust::Record* given;
    int given_accepted;
    int calls = 0;
    void operator()(kf::State& st, const kf::Track& t0, int cp, kr::Reloc& out, int& accepted) {
        calls++;
        if (cp) std::memcpy(keyframe, curr, photo_ref::NPIX);
        if (capacity > 0) {
            const int slot = km::note(t0.flags, cp, st, *m, e, capacity);
            if (slot >= 0) std::memcpy(images + (size_t)slot * photo_ref::NPIX, curr, photo_ref::NPIX);
        }
        photo_search_oriented_ref::Reloc r;
        photo_search_oriented_ref::relocalise(st, keyframe, m, e, images, capacity, curr, *o, hyps, n_hyp, given, r);
        static_assert(sizeof r == sizeof out, "one layout");
        std::memcpy(&out, &r, sizeof out);
        accepted = 0;
        if (!(r.rv.flags & rl::RL_RETRACKED)) return;
        if (given) { accepted = given_accepted; return; }
        hnet_robust::Record recs[hnet_align::MAX_LEVELS];
        std::memset(recs, 0, sizeof recs);
        photo_robust_ref::align(keyframe, curr, r.search.base.start_px, o->align, o->levels, recs);
        for (int l = 0; l < o->levels; l++) accepted += recs[l].px.accepted;
    }
};
}  // namespace

extern "C" {

int filters_keyframe_recover_ref_usable(int had_key, int track_flags, int reloc_flags, int prev_ok) {
    return kfmr::usable_recover(had_key != 0, track_flags, reloc_flags, prev_ok);
}
int filters_keyframe_recover_ref_next_prev_ok(int track_flags) { return kfmr::next_prev_ok_recover(track_flags); }
int filters_keyframe_recover_ref_plain_usable(int had_key, int track_flags, int prev_ok) { return kfm::usable(had_key != 0, track_flags, prev_ok); }
int filters_keyframe_recover_ref_plain_next_prev_ok(int track_flags) { return kfm::next_prev_ok(track_flags); }

// -> 1 usable (z_px, r_px, out72 written; FROM_RELOC or-ed into *flags for a RETRACKED record), 0 unusable (the reason bit or-ed in, nothing else written)
int filters_keyframe_recover_ref_measure(int had_key, const float* key_px_prev, int prev_ok, const hnet_keyframe_track* track, int accepted_total,
                                         const hnet_keyframe_relocalise_oriented* reloc, int accepted_reloc, const hnet_keyframe_measure_opts* o, double k_net_cov,
                                         float* z_px, double* r_px, float* out72, int32_t* flags) {
    kf::Track t;
    kr::Reloc r;
    kfm::Opts mo;
    std::memcpy(&t, track, sizeof t);
    std::memcpy(&r, reloc, sizeof r);
    std::memcpy(&mo, o, sizeof mo);
    return kfmr::measure_recover(had_key != 0, key_px_prev, prev_ok, t, accepted_total, r, accepted_reloc, mo, k_net_cov, z_px, r_px, out72, *flags) ? 1 : 0;
}
// hnet_kfm::measure in this build
int filters_keyframe_recover_ref_plain_measure(int had_key, const float* key_px_prev, int prev_ok, const hnet_keyframe_track* track, int accepted_total,
                                               const hnet_keyframe_measure_opts* o, double k_net_cov, float* z_px, double* r_px, float* out72, int32_t* flags) {
    kf::Track t;
    kfm::Opts mo;
    std::memcpy(&t, track, sizeof t);
    std::memcpy(&mo, o, sizeof mo);
    return kfm::measure(had_key != 0, key_px_prev, prev_ok, t, accepted_total, mo, k_net_cov, z_px, r_px, out72, *flags) ? 1 : 0;
}
int filters_keyframe_recover_ref_relative_z(const float* key_px_prev, const float* key_px_curr, float* z_px) { return kfm::relative_z(key_px_prev, key_px_curr, z_px) ? 1 : 0; }
void filters_keyframe_recover_ref_step(const hnet_filter_state* st, float* step_px) {
    const State s = load(*st);
    for (int k = 0; k < 8; k++) step_px[k] = kfm::step_entry(s, k);
}
// hnet_ekf::innovation of the packed measurement {z_px | (float)(r_px / k_net_cov)} on the state, with the state's own prior
int filters_keyframe_recover_ref_innovation(const hnet_filter_state* st, const hnet_filter_params* p, const float* z_px, const double* r_px, hnet_innovation* out) {
    const State s = load(*st);
    double prior_px[8], prior_cam[8], mean[8], cov[64];
    hnet_ekf::prior_pixels(s, prior_px, prior_cam);
    for (int i = 0; i < 8; i++) mean[i] = (double)z_px[i];
    for (int e = 0; e < 64; e++) cov[e] = (double)hnet_refine::cov72_entry(r_px[e], p->k_net_cov);
    Innovation a;
    const bool ok = hnet_ekf::innovation(s, mean, cov, prior_cam, p->k_net_cov, a);
    to_record(a, 0, *out);
    return ok ? 1 : 0;
}

// hnet_ekf::iterated_update_keyframe_recovered (measured = 0) or iterated_update_keyframe_measured (measured = 1, on rout's measure part; its reloc part is
// left as it came) fed with net72 [iters][72] and the scripted records script [1 + iters].  measure: null = the feature off; reloc: null = recovery off.
// session [128 bytes]: hnet_kfm::Session, read and advanced.  keyframe [71 680], map_state, entries [capacity], images [capacity][71 680] (null with
// capacity 0) and curr: what the host alignment, the map's note and the relocalise run on, all advanced as hnet_sessions_keyframe_track_recover advances
// them; align_rec non-null: the stub record and accepted_total in place of the track's alignment.  out [iters], prec [1 + iters], rout: the records.
// Returns the updates applied, -1 - applied when a singular S ended the loop or the keyframe update.  counts [3]: network, aligner and relocaliser calls.
int filters_keyframe_recover_ref_iterated(int measured, hnet_filter_state* st, const hnet_filter_params* p, int iters, const float* net72, int gate, double max_nis,
                                          const hnet_photo_residual* script, double max_ratio, int min_inside, const hnet_keyframe_measure_opts* measure,
                                          const hnet_keyframe_relocalise_opts* reloc, const void* hyps, int n_hyp, int gap, void* session, uint8_t* keyframe,
                                          void* map_state, void* entries, uint8_t* images, int capacity, const uint8_t* curr, const hnet_photo_robust* align_rec,
                                          int accepted_total, hnet_innovation* out, hnet_photo_residual* prec, hnet_keyframe_measure_recover* rout, int* counts) {
    State s = load(*st);
    FakeNet net{net72, gate, st->t, gate ? 11 : 0};
    ScriptedPhoto photo{&net, script};
    kfm::Opts mo;
    rl::Opts ro;
    if (measure) std::memcpy(&mo, measure, sizeof mo);
    else kfm::default_opts(mo);
    if (reloc) std::memcpy(&ro, reloc, sizeof ro);
    else rl::default_opts(ro);
    Aligner align{keyframe, curr, &mo.track.align, mo.track.levels, align_rec, accepted_total};
    km::MapState* ms = static_cast<km::MapState*>(map_state);
    km::Entry* en = static_cast<km::Entry*>(entries);
    Relocaliser relocaliser{keyframe, ms, en, images, capacity, curr, &ro, static_cast<const po::Hyp*>(hyps), n_hyp, nullptr, 0};
    kfm::Session ks;
    std::memcpy(&ks, session, sizeof ks);
    double prior[8];
    std::vector<Innovation> rec(iters);
    std::vector<PhotoRecord> pr(1 + iters);
    kfmr::Record rr;
    std::memcpy(&rr, rout, sizeof rr);
    int cp = 0, cp2 = 0, done;
    if (measured)
        done = hnet_ekf::iterated_update_keyframe_measured(s, net, iters, p->k_net_cov, prior, st->t, max_nis, rec.data(), photo, max_ratio, min_inside, pr.data(),
                                                           measure ? &mo : nullptr, gap != 0, ks, align, rr.m, &cp);
    else
        done = hnet_ekf::iterated_update_keyframe_recovered(s, net, iters, p->k_net_cov, prior, st->t, max_nis, rec.data(), photo, max_ratio, min_inside, pr.data(),
                                                            measure ? &mo : nullptr, reloc ? &ro : nullptr, gap != 0, ks, align, relocaliser, rr, &cp, &cp2);
    // the commits the loop leaves to its caller: of a session that was not lost, decide's; of an unrecovered one, T1's (the relocaliser made the first)
    if (measure && keyframe) {
        const bool lost_then = relocaliser.calls > 0;
        const int c = lost_then ? cp2 : cp;
        const bool commit = !lost_then || !kr::recovered_by(rr.reloc.rv.flags);
        if (commit) {
            if (c) std::memcpy(keyframe, curr, photo_ref::NPIX);
            if (capacity > 0) {
                const int slot = km::note(rr.m.track.flags, c, ks.key, *ms, en, capacity);
                if (slot >= 0) std::memcpy(images + (size_t)slot * photo_ref::NPIX, curr, photo_ref::NPIX);
            }
        }
    }
    save(s, *st);
    std::memcpy(session, &ks, sizeof ks);
    bool singular = (rr.m.flags & kfm::S_SINGULAR) != 0;
    for (int it = 0; it < iters; it++) {
        to_record(rec[it], it, out[it]);
        singular |= rec[it].flag == hnet_ekf::INNOV_SINGULAR;
    }
    for (int k = 0; k <= iters; k++) prec[k] = to_c(pr[k]);
    std::memcpy(rout, &rr, sizeof rr);
    if (counts) { counts[0] = net.calls; counts[1] = align.calls; counts[2] = relocaliser.calls; }
    return singular ? -1 - done : done;
}

}  // extern "C"
